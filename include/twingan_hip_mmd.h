/* Kernel two-sample statistics over embeddings on the device (twingan_amd/csrc/attention.hip): the block sums of a polynomial
 * kernel's Gram matrix, from which the unbiased MMD^2 of Binkowski et al. ("Demystifying MMD GANs") -- with the cubic kernel
 * the KID -- is a few host additions (twingan_amd/evaluate.py KernelDistance).  The reference has no such metric; the Gram
 * matrix is never written.  Same library and conventions as twingan_hip.h: int-returning entry points, TG_OK or a TG_E* code
 * with the text in tg_last_error(), every launch enqueued on `stream` without host synchronisation, workspaces passed in with
 * a size query. */
#ifndef TWINGAN_HIP_MMD_H_
#define TWINGAN_HIP_MMD_H_

#include "twingan_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TG_MMD_MAX_DEGREE 4

/* Bytes of tg_mmd_block_sums' workspace: one fp64 sum per unit of 32 x 32 pairs, ceil(m / 32) * ceil(n / 32) * 8.  `d` and
 * `block` are validated.  0 for arguments tg_mmd_block_sums refuses (m / n outside 1 .. 2^20, d outside 1 .. 2^30, a bad block). */
size_t tg_mmd_workspace_bytes(int64_t m, int64_t n, int d, int block);

/* sums[I][J] = sum of (double) p(i, j) over the rows i of block I of `a` and the rows j of block J of `b`.  `a` [m, d] and
 * `b` [n, d] are row-major in `dtype` (TG_F32 | TG_BF16 | TG_F16) and may be the same matrix; `sums` is fp64
 * [ceil(m / block), ceil(n / block)], row-major, overwritten; a block is `block` consecutive rows (a multiple of 32, >= 32),
 * the last one of a side may be short.
 *   pair value  in fp32, a function of the two rows' values alone: s = the dot product by the very chain of tg_knn_topk
 *               (TG_BF16 / TG_F16: v_mfma_f32_32x32x16 with fp32 accumulation, 32 of d per step from 0 upwards, the tail
 *               zero-filled; TG_F32: one fmaf chain over d); t = fmaf(gamma, s, coef0); p = t, then degree - 1 times
 *               p = p * t, degree in 1 .. TG_MMD_MAX_DEGREE.
 *   left out    with skip_same_index != 0 the pairs with a_index0 + i == b_index0 + j (a set against itself: the diagonal,
 *               wherever the two row ranges put it).
 *   sums        every pair value is widened to fp64 before it is added.  The order of addition is a function of (m, n, d,
 *               block, dtype) alone: the same call twice gives the same bits.  No atomics.
 *   non-finite  NaN / +-inf follow IEEE and reach exactly the block sums whose blocks hold the offending row.
 *   launches    the pair kernel (every unit of 32 x 32 pairs writes its fp64 sum to `ws`), then the ordered merge of each
 *               block's units into `sums`.
 * `ws`: 8-byte aligned, ws_bytes >= tg_mmd_workspace_bytes(m, n, d, block).  Reads a, b; writes sums and ws, nothing else.
 * TG_EINVAL names the argument: a NULL pointer, m / n outside 1 .. 2^20, d outside 1 .. 2^30, an unknown dtype, degree
 * outside 1 .. TG_MMD_MAX_DEGREE, block < 32 or not a multiple of 32, a negative a_index0 / b_index0, a misaligned or short
 * workspace. */
int tg_mmd_block_sums(const void* a, int64_t m, const void* b, int64_t n, int d, int dtype, int degree, float gamma, float coef0,
                      int block, int64_t a_index0, int64_t b_index0, int skip_same_index, double* sums, void* ws, size_t ws_bytes,
                      void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TWINGAN_HIP_MMD_H_ */
