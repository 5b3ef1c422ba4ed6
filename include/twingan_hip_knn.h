/* Exact nearest-neighbour search over latent embeddings on the device (twingan_amd/csrc/attention.hip): the search the
 * reference's blog runs over the rows its --do_output --output_single_file branch exports (model/model_inheritor.py:1172-1180,
 * twingan.py:685-729) and leaves to the reader.  Same library and conventions as twingan_hip.h: int-returning entry points,
 * TG_OK or a TG_E* code with the text in tg_last_error(), every launch enqueued on `stream` without host synchronisation,
 * workspaces passed in with a size query. */
#ifndef TWINGAN_HIP_KNN_H_
#define TWINGAN_HIP_KNN_H_

#include "twingan_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TG_KNN_MAX_K 32
#define TG_KNN_L2 0     /* squared L2: t = (|q|^2 + |g|^2) - 2 q.g in fp32, in that order; t < 0 -> 0 */
#define TG_KNN_COSINE 1 /* 1 - q.g / (sqrt(|q|^2) sqrt(|g|^2)) in fp32; a zero denominator -> 1 */

/* out_f32[r] = sum_i x[r, i]^2 of the row-major [rows, d] matrix `x` of `dtype` (TG_F32 | TG_BF16 | TG_F16), in fp32, by the
 * very reduction tg_knn_topk applies to the dot product of the row with itself (TG_F32: one fmaf chain over d; 16-bit: the
 * MFMA chain, the norm being the diagonal of a 32-row tile against itself).  So the result depends on the row's values alone
 * -- not on the launch, the pointer's alignment or the row's position --, and the squared L2 distance of a row to a bitwise
 * copy of it is exactly 0.  TG_EINVAL: a NULL pointer, rows / d < 1, an unknown dtype. */
int tg_knn_sqnorm(const void* x, int64_t rows, int d, int dtype, float* out_f32, void* stream);

/* How tg_knn_topk covers a gallery chunk of n rows for q queries: the chunk is cut into tiles of 128 rows, and *splits
 * workgroups per query tile each walk a contiguous run of tiles: splits = min(tiles, 256, ceil(1024 / ceil(q / 32))) -- one
 * for a chunk of at most 128 rows, more the fewer queries there are to fill the device with.  The rule reads nothing but
 * (q, n); d and k are validated.  TG_EINVAL: q / n / d < 1, k outside 1 .. TG_KNN_MAX_K, a NULL `splits`. */
int tg_knn_plan(int64_t q, int64_t n, int d, int k, int* splits);

/* Bytes of tg_knn_topk's workspace for that plan: the split's partial tables (splits * q * k distances and chunk-local
 * indices) and the squared norms of the q queries and the n gallery rows.  0 for arguments tg_knn_plan refuses. */
size_t tg_knn_workspace_bytes(int64_t q, int64_t n, int d, int k);

/* The k nearest gallery rows of every query.  `queries` [q, d] and `gallery` [n, d] are row-major in `dtype`; `dist` [q, k]
 * fp32 and `idx` [q, k] int64 are IN/OUT: on return row i holds the k best of (what it held) U (this chunk's rows, numbered
 * index_offset + row), so a gallery of any size is streamed chunk by chunk; a fresh table is dist = +inf, idx = -1.
 *   order      ascending by (distance, index): equal distances resolve to the lower index.  A pair whose distance is NaN is
 *              never selected (nor is a NaN entry of the incoming table kept); a pair at +inf never displaces the filler, so
 *              unfilled slots stay +inf / -1.
 *   query_ids  int64 [q] or NULL: the gallery row whose index == query_ids[i] is skipped for query i (leave-one-out).
 *   arithmetic norms as tg_knn_sqnorm.  TG_BF16 / TG_F16: dot products on v_mfma_f32_32x32x16 with fp32 accumulation, 32 of
 *              d per step from 0 upwards, the tail zero-filled; TG_F32: one fmaf chain over d per pair.  Neither depends on
 *              the tile, chunk or split a pair falls in: results are bit-identical however the gallery is chunked or split.
 *   launches   the norm passes (16-bit with q <= 64: the queries' only -- the tile kernel takes the gallery's norms in its own
 *              loop, by the same chain), the tile kernel (every split writes an ordered partial table to `ws`), the ordered
 *              merge of the incoming table with the partials.  No atomics.
 * `ws`: 4-byte aligned, ws_bytes >= tg_knn_workspace_bytes(q, n, d, k).  Reads queries, gallery, query_ids; writes dist, idx
 * and ws, nothing else.  TG_EINVAL names the argument: a NULL pointer but query_ids, what tg_knn_plan refuses, an unknown
 * dtype or metric, index_offset < 0, a misaligned or short workspace. */
int tg_knn_topk(const void* queries, int64_t q, const void* gallery, int64_t n, int d, int dtype, int metric, int k,
                int64_t index_offset, const int64_t* query_ids, float* dist, int64_t* idx, void* ws, size_t ws_bytes,
                void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TWINGAN_HIP_KNN_H_ */
