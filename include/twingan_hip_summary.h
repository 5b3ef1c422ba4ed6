/* Training summaries on the device (twingan_amd/csrc/reduce.hip, preprocess.hip): the statistics and TensorFlow histogram of a
 * table of tensors, and sample grids as uint8 images.  Same library and conventions as twingan_hip.h: int-returning entry
 * points, TG_OK or a TG_E* code with the text in tg_last_error(), every launch enqueued on `stream` without host
 * synchronisation, workspaces passed in with a size query. */
#ifndef TWINGAN_HIP_SUMMARY_H_
#define TWINGAN_HIP_SUMMARY_H_

#include "twingan_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* TensorFlow's default histogram buckets (TF 1.8 core/lib/histogram/histogram.cc InitDefaultBuckets): in double,
 * `v = 1e-12; while (v < 1e20) { push v; v *= 1.1; }` gives the TG_SUMMARY_POS_LIMITS positive limits L[k]; the full list is
 * [-DBL_MAX, -L[773] .. -L[0], 0.0, L[0] .. L[773], DBL_MAX].  A value goes to bucket upper_bound(limits, v): limits are
 * exclusive upper edges, both zeros land in the bucket whose limit is L[0]. */
#define TG_SUMMARY_POS_LIMITS 774
#define TG_SUMMARY_BUCKETS 1551

/* The result of one tensor.  Every field is defined over the FINITE v = float(x) * scale only (NaN and +-inf are counted in
 * `nonfinite` and otherwise left out); with num == 0: min = FLT_MAX, max = -FLT_MAX, the sums 0. */
typedef struct TgSummaryStats {
  double sum, sum_squares; /* of double(v) and double(v)^2, both exact in double; added in a fixed order */
  float min, max;
  uint32_t num, zeros, nonfinite; /* zeros: v == 0, either sign */
  uint32_t reserved;
} TgSummaryStats;

/* The bucket limits, computed on the host and nowhere else: limits[TG_SUMMARY_BUCKETS] as above (what a HistogramProto's
 * bucket_limit holds) and pos_limits_f32[TG_SUMMARY_POS_LIMITS], each L[k] rounded UP to the nearest float -- for a float v,
 * v < L[k] exactly when v < pos_limits_f32[k], so the kernel compares floats and agrees with TF's double comparison.  Either
 * pointer may be NULL.  TG_ENOSUP if a rounded limit is not strictly above its L[k] or not above its predecessor (the
 * kernel's treatment of negative values relies on both).  Replaces histogram.cc InitDefaultBuckets behind tf.summary.histogram
 * (model/model_inheritor.py:1056-1058). */
int tg_summary_limits(double* limits, float* pos_limits_f32);

/* Job table of tg_summary_multi, as tg_ema_table_*: filled on the host one job at a time, copied to the device by the caller.
 * A job is one tensor: `base` of `dtype` (TG_F32 | TG_BF16 | TG_F16), `rows` rows of `row_valid` elements that start
 * `row_stride` elements apart (row_stride > row_valid: a conv kernel stored with a padded input-channel count; the padding is
 * never read; a dense tensor is rows = 1), and `out`, its index into the result arrays.  Jobs are filled in the order job = 0,
 * 1, ...: *total_blocks (0 before the first) accumulates the grid.  TG_EINVAL names the argument: a NULL pointer, an unknown
 * dtype, rows / row_valid < 1, row_stride < row_valid, out < 0, rows * row_valid >= 2^32, a grid beyond 2^31 - 1 blocks. */
size_t tg_summary_table_bytes(int njobs);
int tg_summary_table_fill(const void* base, int dtype, int64_t rows, int64_t row_valid, int64_t row_stride, int out, int job,
                          void* table_host, int32_t* total_blocks);

/* Bytes of tg_summary_multi's workspace (the per-workgroup partial results) for a table of total_blocks. */
size_t tg_summary_workspace_bytes(int total_blocks);

/* The statistics and histogram of every tensor of a table: replaces the tf.summary.histogram of every variable
 * (model/model_inheritor.py:1056-1058), of every gradient and its norm (deployment/model_deploy.py:506-530,
 * image_generation.py:611-619) and of the end points, with their tf.nn.zero_fraction (model_inheritor.py:721-726), that the
 * reference's summary op evaluates on the host.  v = float(x) * scale in fp32, times scale_dev[0] as well when scale_dev is set
 * (the unscaling of an fp16 run's gradients from a device scalar); with scale == 1 and no scale_dev, v = float(x).  Job j
 * writes stats[out_j] and buckets[out_j * TG_SUMMARY_BUCKETS ...]; the buckets of ALL nout rows are zeroed first, stats rows
 * no job names are left alone, a job whose out is not below nout is skipped.  limits_dev: tg_summary_limits' pos_limits_f32
 * in device memory.  Three launches (zero, the per-workgroup pass, the ordered finish); counts go through integer atomics,
 * sums, minima and maxima through the workspace in a fixed order: results are bit-identical from launch to launch.  Reads each element once.  TG_EINVAL names the argument:
 * a NULL pointer but scale_dev, njobs / total_blocks / nout < 1, workspace_bytes below tg_summary_workspace_bytes(total_blocks). */
int tg_summary_multi(const void* table_device, int njobs, int total_blocks, int nout, float scale, const float* scale_dev,
                     const float* limits_dev, TgSummaryStats* stats, uint32_t* buckets, void* workspace, size_t workspace_bytes,
                     void* stream);

/* Job table of tg_image_grid_u8: job `job` is an NHWC batch [n, h, w, c] at `src` (dtype as above, c 1 or 3; h and w are the
 * launch's) whose image i goes to grid cell (row i, column `col`).  TG_EINVAL names the argument. */
size_t tg_image_grid_table_bytes(int njobs);
int tg_image_grid_table_fill(const void* src, int dtype, int n, int c, int col, int job, void* table_host);

/* Fills the uint8 grid [rows * h, cols * w, 3] in one launch: replaces util_io.save_float_image / imsave over the grids of
 * twingan.py:606-678 (image_generation.py:694-714, util_io.py:121-142).  Each byte is clip(trunc(float(x) * 255.0f), 0, 255)
 * with the product in fp32; this project's definition where numpy's astype(int32) is the platform's: NaN -> 0, products at or
 * above 255 (+inf, those beyond int32) -> 255, negative ones (-inf) -> 0.  c == 1 is replicated to three channels.  Images
 * i >= rows of a job are dropped; cells no job names are 0; of two jobs with one column the earlier wins.  Every byte of the
 * grid is written exactly once, nothing outside it.  TG_EINVAL names the argument: a NULL pointer, njobs / rows / cols / h / w
 * < 1, a grid of 2^31 pixels or more. */
int tg_image_grid_u8(const void* table_device, int njobs, int rows, int cols, int h, int w, uint8_t* grid, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TWINGAN_HIP_SUMMARY_H_ */
