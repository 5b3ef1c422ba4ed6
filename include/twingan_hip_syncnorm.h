/* Cross-replica batch statistics for the data-parallel trainer (twingan_amd/csrc/norm.hip): the normaliser of
 * tg_norm_act_fwd / tg_norm_act_bwd split at the two points where a statistic group's numbers have to meet the other
 * clones' (Config.cross_replica_norm; this project's own rule -- the reference's clones keep their own statistics,
 * deployment/model_deploy.py).  Every clone holds `count` = h * w pixels of each of the n statistic groups (EQUAL counts on
 * all clones); between the calls below the caller all-gathers one small fp32 tensor, [n][k][c] -> [replicas][n][k][c] in
 * rank order (k = 3 forward, 2 backward):
 *
 *   forward    tg_norm_moments -> gather -> tg_norm_moments_merge -> tg_norm_act_fwd (twingan_hip.h; tg_pool2x2_fwd after it
 *              for a pooled output)
 *   backward   tg_norm_act_bwd_sums -> gather -> tg_norm_act_bwd_apply
 *
 * The result is what ONE clone computes on the clones' batches concatenated along the group's pixels.  Every sum over
 * chunks and over replicas is taken in a fixed order (no atomics but the single add per parameter of `accumulate`), so
 * clones that gathered the same rows hold bit-identical statistics.  Same library and conventions as twingan_hip.h:
 * int-returning entry points, TG_OK or a TG_E* code with the text in tg_last_error(), every launch enqueued on `stream`
 * without host synchronisation.  Shapes as the fused path: the vector path for c = (16 bytes / element size) * 2^k <= 64
 * vectors, the scalar path for any other c <= 256 (tg_norm_moments alone: any c <= 2048 its statistics kernel takes), pixel
 * norm on the vector path only; NF_NOSTATS (constant statistics) has nothing to share and is refused with TG_EINVAL. */
#ifndef TWINGAN_HIP_SYNCNORM_H_
#define TWINGAN_HIP_SYNCNORM_H_

#include "twingan_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The moments of y[g, :, :, ch] (`dtype`, [n, h, w, c]) over (h, w), fp32 [n][3][c]:
 *   moments[g][0][ch] + moments[g][1][ch] = mean   an fp32 pair: the value and what rounding it to fp32 dropped
 *   moments[g][2][ch] = M2 = sum (y - mean)^2     M2 itself, not a value recovered from an rstd
 * Two launches: the shifted partial sums of tg_instance_norm_partials (K = y[g, 0, 0, ch]) into `ws` (fp32
 * [n * tg_norm_chunks(n, h, w) * 2 * c], scratch), then one workgroup per group adds the chunks in a fixed order, in double:
 * mean = K + S1 / hw, M2 = S2 - S1 * S1 / hw (clamped at 0).  The pair is there for the merge: a mean rounded to fp32
 * (error e_r, up to half an ulp) would enter the merged variance as 2 count sum_r (mean_r - mean) e_r, which is 1e-3 of
 * rstd where the mean is thousands of standard deviations and a replica holds a few dozen pixels. */
int tg_norm_moments(const void* y, float* moments, float* ws, int n, int h, int w, int c, int dtype, void* stream);

/* Chan's rule over `replicas` rows of equal count, in rank order 0 .. replicas-1: gathered fp32 [replicas][n][3][c] (the
 * clones' `moments`) ->
 *   mean = (sum_r mean_r) / replicas
 *   M2   = sum_r M2_r + count * sum_r (mean_r - mean)^2,   var = M2 / (replicas * count)   (biased)
 *   rstd = rsqrt(var + eps)
 * (the sums in double, one thread per value) written to mean[n * c] / rstd[n * c], the form tg_norm_act_fwd takes.
 * `count`: the pixels of one group on one replica (h * w of tg_norm_moments); replicas * count < 2^31.  Raw sums and sums
 * of squares never meet: the rows are centred. */
int tg_norm_moments_merge(const float* gathered, int replicas, int64_t count, float* mean, float* rstd, int n, int c,
                          float eps, void* stream);

/* Pass 1 of tg_norm_act_bwd on this clone's pixels, same arguments (mean / rstd: the MERGED statistics the forward
 * used): local[g][0][ch] = S1 = sum gu, local[g][1][ch] = S2 = sum gu * yhat, fp32 [n][2][c], the per-chunk sums (`ws`,
 * fp32 [n * tg_norm_chunks(n, h, w) * 2 * c], scratch) added in a fixed order.  The parameter gradients are LOCAL sums -- the
 * trainer's gradient all-reduce adds the clones' -- produced as tg_norm_act_bwd produces them: ggamma[c] / gbeta[c]
 * (+ ggamma2 / gbeta2 for groups >= split) written, or with accumulate != 0 added (one add per parameter, groups in
 * order); with per_image_params they are rows [n][c] and written.  Any of them may be NULL. */
int tg_norm_act_bwd_sums(const void* gz, const void* gz_pooled, const void* y, const float* pn_scale, const float* mean,
                         const float* rstd, const float* gamma, const float* beta, const float* gamma2, const float* beta2,
                         int split, int per_image_params, float* ggamma, float* gbeta, float* ggamma2, float* gbeta2,
                         float* ws, float* local, int n, int h, int w, int c, int flags, float lrelu_alpha, int accumulate,
                         int dtype, void* stream);

/* Pass 2 of tg_norm_act_bwd: gy = gamma * rstd * (gu - S1 / N - yhat * S2 / N) with S1 / S2 the sum of the `replicas` rows
 * of gathered fp32 [replicas][n][2][c] (the clones' `local`), added in rank order in every workgroup's prologue, and
 * N = replicas * h * w (< 2^31), the group's pixels on all clones.  Writes gy ([n, h, w, c], `dtype`) and nothing else. */
int tg_norm_act_bwd_apply(const void* gz, const void* gz_pooled, const void* y, const float* pn_scale, const float* mean,
                          const float* rstd, const float* gamma, const float* beta, const float* gamma2, const float* beta2,
                          int split, int per_image_params, void* gy, const float* gathered, int replicas, int n, int h,
                          int w, int c, int flags, float lrelu_alpha, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TWINGAN_HIP_SYNCNORM_H_ */
