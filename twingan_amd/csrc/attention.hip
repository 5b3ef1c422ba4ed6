// SAGAN self-attention (libs/self_attention.py:24-70) as gfx950 kernels behind the C ABI:
//     f, g = tanh(conv1x1(x))  [N, c/8],  h = conv1x1(x)  [N, c]        (the 1x1 convs are tg_conv2d_* / tg_pointwise_*)
//     s = f g^T  [N, N],  beta = softmax(s, axis=-1),  o = beta h,  y = sa_gamma * o + x           (N = H*W per image)
// built from three primitives, each of which is its own derivative family, so that the layer is differentiable TWICE
// on these kernels (the discriminators sit under the WGAN-GP gradient penalty):
//   * tg_batched_gemm      C[b] = alpha * op(A[b]) op(B[b]) (+ C[b])   -- bf16: v_mfma_f32_32x32x16_bf16, 128 x 64 x 32
//                          workgroup tiles staged through LDS; an operand whose reduction axis is contiguous in memory is
//                          read with ds_read_b128, the other kind with the LDS transpose read ds_read_b64_tr_b16 (row
//                          strides 320 / 192 B keep a half-wave's 4 x 32-byte segments on distinct banks); fp32: one
//                          thread per output element (the exact-parity path, small maps)
//   * tg_softmax_rows_{fwd,bwd,bwd_bwd}   row softmax, its backward dS = P (dP - sum(dP P)) and that map's gradient in P
//   * tg_tanh_{fwd,bwd}, tg_mul3, tg_dot, tg_scale_dev   the pointwise pieces and the sa_gamma scale / reduction
// Replaces tf.matmul x2, tf.nn.softmax, tf.nn.tanh and the gamma * o + layer arithmetic of libs/self_attention.py:57-69.
#include "tg_common.h"
#include "../../include/twingan_hip_knn.h"
#include "../../include/twingan_hip_mmd.h"

namespace {

struct BgGeom {
  int m, n, k;
  int lda, ldb, ldc;
  long long sa, sb, sc;      // batch strides in elements
  float alpha;
  int accumulate, c_f32, vec;
};

typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;

__device__ __forceinline__ bf16x8 lds_tr8(const unsigned char* p, int second) {
  typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p + second));
  s16x8 v;
  v[0] = lo[0]; v[1] = lo[1]; v[2] = lo[2]; v[3] = lo[3];
  v[4] = hi[0]; v[5] = hi[1]; v[6] = hi[2]; v[7] = hi[3];
  return __builtin_bit_cast(bf16x8, v);
}

// one 16-byte vector (8 elements along the contiguous axis) of a [rows][cols] global matrix, zero outside
__device__ __forceinline__ bf16x8 gload8(const bf16* base, int row, int col, int rows, int cols, int ld, bool vec) {
  bf16x8 v;
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = (bf16)0.f;
  if (row >= rows || col >= cols) return v;
  const bf16* p = base + (size_t)row * ld + col;
  if (vec) return *reinterpret_cast<const bf16x8*>(p);      // cols % 8 == 0: the vector is entirely inside
#pragma unroll
  for (int j = 0; j < 8; ++j)
    if (col + j < cols) v[j] = p[j];
  return v;
}

constexpr int BM = 128, BN = 64, BK = 32;
constexpr int A_KC_STRIDE = 80, B_KC_STRIDE = 80;        // bytes per row of a K-contiguous tile [rows][32 k] (+16 pad)
constexpr int A_KS_STRIDE = 320, B_KS_STRIDE = 192;      // bytes per k row of a K-strided tile [32 k][128 | 64 cols] (+64 pad)

// AKC / BKC: op(A)'s / op(B)'s reduction axis is contiguous in memory (A stored [m][k] / B stored [n][k])
template <bool AKC, bool BKC, bool F16 = false>
__global__ __launch_bounds__(256) void bgemm_mfma_kernel(const bf16* __restrict__ A, const bf16* __restrict__ B,
                                                         void* __restrict__ C, const BgGeom g) {
  __shared__ __attribute__((aligned(16))) unsigned char sA[AKC ? BM * A_KC_STRIDE : BK * A_KS_STRIDE];
  __shared__ __attribute__((aligned(16))) unsigned char sB[BKC ? BN * B_KC_STRIDE : BK * B_KS_STRIDE];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
  const bf16* Ab = A + (size_t)blockIdx.z * g.sa;
  const bf16* Bb = B + (size_t)blockIdx.z * g.sb;
  const bool vec = g.vec != 0;

  f32x16 acc[2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[i][j] = 0.f;

  bf16x8 ra[2], rb;
  auto load_tiles = [&](int k0) __attribute__((always_inline)) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int v = tid + s * 256;
      if constexpr (AKC) ra[s] = gload8(Ab, m0 + (v >> 2), k0 + (v & 3) * 8, g.m, g.k, g.lda, vec);
      else ra[s] = gload8(Ab, k0 + (v >> 4), m0 + (v & 15) * 8, g.k, g.m, g.lda, vec);
    }
    if constexpr (BKC) rb = gload8(Bb, n0 + (tid >> 2), k0 + (tid & 3) * 8, g.n, g.k, g.ldb, vec);
    else rb = gload8(Bb, k0 + (tid >> 3), n0 + (tid & 7) * 8, g.k, g.n, g.ldb, vec);
  };
  auto store_tiles = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int v = tid + s * 256;
      if constexpr (AKC) *reinterpret_cast<bf16x8*>(sA + (v >> 2) * A_KC_STRIDE + (v & 3) * 16) = ra[s];
      else *reinterpret_cast<bf16x8*>(sA + (v >> 4) * A_KS_STRIDE + (v & 15) * 16) = ra[s];
    }
    if constexpr (BKC) *reinterpret_cast<bf16x8*>(sB + (tid >> 2) * B_KC_STRIDE + (tid & 3) * 16) = rb;
    else *reinterpret_cast<bf16x8*>(sB + (tid >> 3) * B_KS_STRIDE + (tid & 7) * 16) = rb;
  };

  // fragment addresses: row / column index i = lane & 31, k group kg = lane >> 5 (8 consecutive k);
  // transpose reads: 16-lane group q = lane >> 4 -> column half q & 1, lane s = lane & 15 -> k row +(s >> 2), columns 4 (s & 3)
  const int i32 = lane & 31, kg = lane >> 5, q = lane >> 4, s16 = lane & 15;
  const int a_kc = (wid * 32 + i32) * A_KC_STRIDE + kg * 16;
  const int a_ks = (kg * 8 + (s16 >> 2)) * A_KS_STRIDE + (wid * 32 + (q & 1) * 16 + (s16 & 3) * 4) * 2;
  const int b_kc = i32 * B_KC_STRIDE + kg * 16;
  const int b_ks = (kg * 8 + (s16 >> 2)) * B_KS_STRIDE + ((q & 1) * 16 + (s16 & 3) * 4) * 2;

  load_tiles(0);
  for (int k0 = 0; k0 < g.k; k0 += BK) {
    __syncthreads();      // the previous tile's fragment reads are done
    store_tiles();
    __syncthreads();
    if (k0 + BK < g.k) load_tiles(k0 + BK);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 af;
      if constexpr (AKC) af = *reinterpret_cast<const bf16x8*>(sA + a_kc + ks * 32);
      else af = lds_tr8(sA + a_ks + ks * 16 * A_KS_STRIDE, 4 * A_KS_STRIDE);
#pragma unroll
      for (int nb = 0; nb < 2; ++nb) {
        bf16x8 bfr;
        if constexpr (BKC) bfr = *reinterpret_cast<const bf16x8*>(sB + b_kc + nb * 32 * B_KC_STRIDE + ks * 32);
        else bfr = lds_tr8(sB + b_ks + nb * 64 + ks * 16 * B_KS_STRIDE, 4 * B_KS_STRIDE);
        acc[nb] = mfma_32x32x16<F16>(af, bfr, acc[nb]);
      }
    }
  }

  // acc[nb][r]: row m0 + 32 wid + (r & 3) + 8 (r >> 2) + 4 (lane >> 5), column n0 + 32 nb + (lane & 31)
#pragma unroll
  for (int nb = 0; nb < 2; ++nb) {
    const int col = n0 + nb * 32 + i32;
    if (col >= g.n) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = m0 + wid * 32 + (r & 3) + 8 * (r >> 2) + 4 * kg;
      if (row >= g.m) continue;
      const size_t off = (size_t)blockIdx.z * g.sc + (size_t)row * g.ldc + col;
      float v = g.alpha * acc[nb][r];
      if (g.c_f32) {
        float* c = reinterpret_cast<float*>(C) + off;
        *c = g.accumulate ? *c + v : v;
      } else {
        if constexpr (F16) {
          f16* c = reinterpret_cast<f16*>(C) + off;
          *c = (f16)(g.accumulate ? (float)*c + v : v);
        } else {
          bf16* c = reinterpret_cast<bf16*>(C) + off;
          *c = (bf16)(g.accumulate ? (float)*c + v : v);
        }
      }
    }
  }
}

// any dtype, any shape: one thread per output element (fp32 exact-parity path)
template <typename T>
__global__ void bgemm_simple_kernel(const T* __restrict__ A, const T* __restrict__ B, void* __restrict__ C, const BgGeom g,
                                    int ta, int tb) {
  const long long total = (long long)g.m * g.n;
  const T* Ab = A + (size_t)blockIdx.y * g.sa;
  const T* Bb = B + (size_t)blockIdx.y * g.sb;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int row = (int)(i / g.n), col = (int)(i - (long long)row * g.n);
    float acc = 0.f;
    for (int k = 0; k < g.k; ++k) {
      const float a = ld(Ab + (ta ? (size_t)k * g.lda + row : (size_t)row * g.lda + k));
      const float b = ld(Bb + (tb ? (size_t)col * g.ldb + k : (size_t)k * g.ldb + col));
      acc = fmaf(a, b, acc);
    }
    const size_t off = (size_t)blockIdx.y * g.sc + (size_t)row * g.ldc + col;
    const float v = g.alpha * acc;
    if (g.c_f32) {
      float* c = reinterpret_cast<float*>(C) + off;
      *c = g.accumulate ? *c + v : v;
    } else {
      T* c = reinterpret_cast<T*>(C) + off;
      st(c, g.accumulate ? ld(c) + v : v);
    }
  }
}

// ---- row softmax -------------------------------------------------------------------------------------------------
// block = one row of `cols` elements
template <typename T>
__global__ __launch_bounds__(256) void softmax_rows_fwd_kernel(const T* __restrict__ s, T* __restrict__ p, int cols) {
  __shared__ float red[4];
  const T* row = s + (size_t)blockIdx.x * cols;
  T* out = p + (size_t)blockIdx.x * cols;
  float mx = -3.0e38f;
  for (int c = threadIdx.x; c < cols; c += 256) mx = fmaxf(mx, ld(row + c));
  // block max through the sum helper's scratch
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  __syncthreads();
  float sum = 0.f;
  for (int c = threadIdx.x; c < cols; c += 256) sum += __expf(ld(row + c) - mx);
  sum = block_sum(sum, red);
  const float inv = 1.f / sum;
  for (int c = threadIdx.x; c < cols; c += 256) st(out + c, __expf(ld(row + c) - mx) * inv);
}

// ds = p * (dp - sum_j dp_j p_j)
template <typename T>
__global__ __launch_bounds__(256) void softmax_rows_bwd_kernel(const T* __restrict__ p, const T* __restrict__ dp,
                                                               T* __restrict__ ds, int cols) {
  __shared__ float red[4];
  const size_t base = (size_t)blockIdx.x * cols;
  float t = 0.f;
  for (int c = threadIdx.x; c < cols; c += 256) t = fmaf(ld(dp + base + c), ld(p + base + c), t);
  t = block_sum(t, red);
  for (int c = threadIdx.x; c < cols; c += 256) st(ds + base + c, ld(p + base + c) * (ld(dp + base + c) - t));
}

// gradient of L = sum_j v_j ds_j (ds as above) with respect to p:  v_j (dp_j - t) - dp_j u,  t = sum dp p, u = sum v p
template <typename T>
__global__ __launch_bounds__(256) void softmax_rows_bwd_bwd_kernel(const T* __restrict__ p, const T* __restrict__ dp,
                                                                   const T* __restrict__ v, T* __restrict__ gp, int cols) {
  __shared__ float red[4];
  const size_t base = (size_t)blockIdx.x * cols;
  float t = 0.f, u = 0.f;
  for (int c = threadIdx.x; c < cols; c += 256) {
    const float pc = ld(p + base + c);
    t = fmaf(ld(dp + base + c), pc, t);
    u = fmaf(ld(v + base + c), pc, u);
  }
  t = block_sum(t, red);
  u = block_sum(u, red);
  for (int c = threadIdx.x; c < cols; c += 256) {
    const float d = ld(dp + base + c);
    st(gp + base + c, ld(v + base + c) * (d - t) - d * u);
  }
}

// ---- pointwise pieces ----------------------------------------------------------------------------------------------
template <typename T>
__global__ void tanh_fwd_kernel(const T* __restrict__ x, T* __restrict__ y, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    st(y + i, tanhf(ld(x + i)));
}
template <typename T>      // gx = g * (1 - y^2)
__global__ void tanh_bwd_kernel(const T* __restrict__ g, const T* __restrict__ y, T* __restrict__ gx, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float yy = ld(y + i);
    st(gx + i, ld(g + i) * (1.f - yy * yy));
  }
}
template <typename T>      // out = scale * a * b * c
__global__ void mul3_kernel(const T* __restrict__ a, const T* __restrict__ b, const T* __restrict__ c, T* __restrict__ out,
                            float scale, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    st(out + i, scale * ld(a + i) * ld(b + i) * (c ? ld(c + i) : 1.f));
}
template <typename T>      // out = x * s[0]  (s: device fp32 scalar)
__global__ void scale_dev_kernel(const T* __restrict__ x, const float* __restrict__ s, T* __restrict__ out, int64_t n) {
  const float k = s[0];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    st(out + i, ld(x + i) * k);
}
// part[block] = sum over the block's range of a * b (fixed order); dot_final sums the partials
template <typename T>
__global__ __launch_bounds__(256) void dot_partial_kernel(const T* __restrict__ a, const T* __restrict__ b,
                                                          float* __restrict__ part, int64_t n, int64_t per) {
  __shared__ float red[4];
  const int64_t lo = (int64_t)blockIdx.x * per, hi = lo + per < n ? lo + per : n;
  float t = 0.f;
  for (int64_t i = lo + threadIdx.x; i < hi; i += 256) t = fmaf(ld(a + i), ld(b + i), t);
  t = block_sum(t, red);
  if (threadIdx.x == 0) part[blockIdx.x] = t;
}
__global__ __launch_bounds__(256) void dot_final_kernel(const float* __restrict__ part, int nparts, float* __restrict__ out) {
  __shared__ float red[4];
  float t = 0.f;
  for (int i = threadIdx.x; i < nparts; i += 256) t += part[i];
  t = block_sum(t, red);
  if (threadIdx.x == 0) out[0] = t;
}

// ---- nearest-neighbour search over embeddings (include/twingan_hip_knn.h) -------------------------------------------------
// A workgroup owns a tile of queries and walks gallery tiles of 128 rows.  16-bit: the bgemm staging above with both operands
// K-contiguous ([rows][32 k] at 80 B a row, ds_read_b128 fragments), wave w holds the 32 QB x 32 dot products of the tile's
// columns 32 w ..; fp32: one thread per pair.  Either way a pair's reduction over d is one fixed chain.  Selection is shared:
// per query a list of k (distance, chunk-local index), ascending, in LDS as [slot][query] (a thread walks its own query's
// column: no bank conflict); the list's last slot is the filter every candidate meets first.  What passes is staged, 32
// columns at a time, and the query's own thread inserts in column order -- the order does not matter to the result, since
// (distance, index) is a total order, but a fixed one costs nothing.  Every split's list goes to the workspace, and
// knn_merge_kernel folds the incoming table and the partials, split by split, into the in/out table.
constexpr int KNN_K = TG_KNN_MAX_K;
constexpr int KNN_GT = 128;      // gallery rows per tile
constexpr int KNN_SW = 33;       // floats per staged row of 32 columns (+1: a thread per row scans without conflicts)
constexpr int KNN_ROW = 80;      // bytes per staged operand row, as A_KC_STRIDE

struct KnnGeom {
  int q, n, d, k, metric, splits, tiles, vec;
  int64_t index_offset;
  const int64_t* query_ids;
  const float* qn;
  const float* gn;
  float* part_d;
  int* part_i;
};

template <typename I>
__device__ __forceinline__ bool knn_less(float d1, I i1, float d2, I i2) { return d1 < d2 || (d1 == d2 && i1 < i2); }

__device__ __forceinline__ float knn_distance(int metric, float qn, float gn, float dot) {
  if (metric == TG_KNN_L2) {
    const float t = (qn + gn) - 2.f * dot;
    return t < 0.f ? 0.f : t;      // not fmaxf: a NaN stays a NaN
  }
  const float den = sqrtf(qn) * sqrtf(gn);
  return den == 0.f ? 1.f : 1.f - dot / den;
}

// (d, gi) into the ascending list whose slot j is at [j * stride]; false when it does not beat the last slot (NaN never does)
template <typename I>
__device__ __forceinline__ bool knn_insert(float* ld_, I* li, int stride, int k, float d, I gi) {
  if (!knn_less<I>(d, gi, ld_[(k - 1) * stride], li[(k - 1) * stride])) return false;
  int j = k - 1;
  while (j > 0 && knn_less<I>(d, gi, ld_[(j - 1) * stride], li[(j - 1) * stride])) {
    ld_[j * stride] = ld_[(j - 1) * stride];
    li[j * stride] = li[(j - 1) * stride];
    --j;
  }
  ld_[j * stride] = d;
  li[j * stride] = gi;
  return true;
}

// the query's own thread: the 32 staged columns of its row, NaN = not a candidate, column c = chunk row `first` + c
__device__ __forceinline__ void knn_scan(const float* stage_row, float* ld_, int* li, int stride, int k, int first, int skip) {
#pragma unroll 1
  for (int c = 0; c < 32; ++c) {
    const float v = stage_row[c];
    if (v == v && first + c != skip) knn_insert<int>(ld_, li, stride, k, v, first + c);
  }
}

// gload8 for a dense [rows][d] matrix whose tail (d % 8 != 0, or a base that is not 16-byte aligned) is read without a branch
// per element: the address is clamped into the row and the value selected afterwards
__device__ __forceinline__ bf16x8 knn_load8(const bf16* base, int row, int col, int rows, int d, bool vec) {
  bf16x8 v;
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = (bf16)0.f;
  if (row >= rows || col >= d) return v;
  const bf16* p = base + (size_t)row * d;
  if (vec) return *reinterpret_cast<const bf16x8*>(p + col);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const bf16 x = p[col + j < d ? col + j : d - 1];
    v[j] = col + j < d ? x : (bf16)0.f;
  }
  return v;
}

// The staged 16-bit dot products that the search and the kernel two-sample sums (include/twingan_hip_mmd.h) share: the 32 QB
// rows q0 .. of Q [q][d] against the 128 rows g0 .. of G [n][d], 32 of d per step from 0 upwards through sA / sB (rows of
// KNN_ROW bytes, the next step's vectors in flight), rows and columns outside the matrices and the tail of d zero-filled.
// On return acc[qb][r] of wave w, lane (i32, kg) is row 32 qb + (r & 3) + 8 (r >> 2) + 4 kg against column 32 w + i32, and
// with GN accn holds the wave's 32 columns against themselves (their squared norms on the diagonal).  Every thread of the
// workgroup of 256 calls it; the first barrier of the loop is also the one that ends the caller's previous use of sA / sB.
template <int QB, bool F16, bool GN>
__device__ __forceinline__ void pair_tile_dots(const bf16* __restrict__ Q, const bf16* __restrict__ G, int q0, int g0, int q, int n,
                                               int d, bool vec, unsigned char* sA, unsigned char* sB, f32x16 (&acc)[QB], f32x16& accn) {
  constexpr int BM = 32 * QB;
  constexpr int AV = (BM * 4 + 255) / 256;      // 16-byte vectors of the query tile per thread
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, i32 = lane & 31, kg = lane >> 5;
  const int a_frag = i32 * KNN_ROW + kg * 16, b_frag = (wid * 32 + i32) * KNN_ROW + kg * 16;
#pragma unroll
  for (int i = 0; i < QB; ++i)
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[i][j] = 0.f;
#pragma unroll
  for (int j = 0; j < 16; ++j) accn[j] = 0.f;

  bf16x8 ra[AV], rb[2];
  auto load_tiles = [&](int k0) __attribute__((always_inline)) {
#pragma unroll
    for (int s = 0; s < AV; ++s) {
      const int v = tid + s * 256;
      if (v < BM * 4) ra[s] = knn_load8(Q, q0 + (v >> 2), k0 + (v & 3) * 8, q, d, vec);
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int v = tid + s * 256;
      rb[s] = knn_load8(G, g0 + (v >> 2), k0 + (v & 3) * 8, n, d, vec);
    }
  };
  load_tiles(0);
  for (int k0 = 0; k0 < d; k0 += 32) {
    __syncthreads();      // the previous step's fragment reads (or the caller's previous use of the tiles) are done with
#pragma unroll
    for (int s = 0; s < AV; ++s) {
      const int v = tid + s * 256;
      if (v < BM * 4) *reinterpret_cast<bf16x8*>(sA + (v >> 2) * KNN_ROW + (v & 3) * 16) = ra[s];
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int v = tid + s * 256;
      *reinterpret_cast<bf16x8*>(sB + (v >> 2) * KNN_ROW + (v & 3) * 16) = rb[s];
    }
    __syncthreads();
    if (k0 + 32 < d) load_tiles(k0 + 32);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const bf16x8 bfr = *reinterpret_cast<const bf16x8*>(sB + b_frag + ks * 32);
      if constexpr (GN) accn = mfma_32x32x16<F16>(bfr, bfr, accn);
#pragma unroll
      for (int qb = 0; qb < QB; ++qb) {
        const bf16x8 af = *reinterpret_cast<const bf16x8*>(sA + a_frag + qb * 32 * KNN_ROW + ks * 32);
        acc[qb] = mfma_32x32x16<F16>(af, bfr, acc[qb]);
      }
    }
  }
}

// the fp32 dot product of two rows: one fmaf chain over d, shared likewise
template <typename T>
__device__ __forceinline__ float pair_dot_chain(const T* __restrict__ qp, const T* __restrict__ gp, int d) {
  float dot = 0.f;
  for (int i = 0; i < d; ++i) dot = fmaf(ld(qp + i), ld(gp + i), dot);
  return dot;
}

template <int BM>
__device__ __forceinline__ void knn_write_partial(const KnnGeom& g, const float* listD, const int* listI, int q0, int split) {
  for (int i = threadIdx.x; i < g.k * BM; i += 256) {
    const int j = i / BM, row = i - j * BM;
    if (q0 + row >= g.q) continue;
    const size_t off = ((size_t)split * g.q + (q0 + row)) * g.k + j;
    g.part_d[off] = listD[j * BM + row];
    g.part_i[off] = listI[j * BM + row];
  }
}

template <int QB, bool F16>
__global__ __launch_bounds__(256, 2) void knn_mfma_kernel(const bf16* __restrict__ Q, const bf16* __restrict__ G, const KnnGeom g) {
  constexpr int BM = 32 * QB;
  constexpr int A_BYTES = BM * KNN_ROW, B_BYTES = KNN_GT * KNN_ROW, STAGE_BYTES = BM * KNN_SW * 4;
  constexpr int S_BYTES = A_BYTES + B_BYTES > STAGE_BYTES ? A_BYTES + B_BYTES : STAGE_BYTES;
  __shared__ __attribute__((aligned(16))) unsigned char smem[S_BYTES];      // operand tiles; the staged distances after the k loop
  __shared__ float listD[KNN_K * BM];
  __shared__ int listI[KNN_K * BM];
  __shared__ float sQn[BM];
  // QB < 4 (few queries: the search is bound by reading the gallery once): the gallery norms come from this loop too -- the
  // B fragment against itself, the diagonal of the wave's 32 x 32 block, the very chain of knn_sqnorm_mfma_kernel -- instead of
  // from a pass of their own over the gallery; with 128 queries a fifth MFMA a step costs more than that pass
  constexpr bool GN = QB < 4;
  __shared__ float sGn[KNN_GT];
  unsigned char* sA = smem;
  unsigned char* sB = smem + A_BYTES;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, i32 = lane & 31, kg = lane >> 5;
  const int q0 = blockIdx.x * BM, split = blockIdx.y;
  // tiles < 2^24 and splits <= 256: the products fit 32 bits
  const int t_lo = (int)((unsigned)split * (unsigned)g.tiles / (unsigned)g.splits);
  const int t_hi = (int)((unsigned)(split + 1) * (unsigned)g.tiles / (unsigned)g.splits);
  const bool vec = g.vec != 0;
  int skip = -1;      // thread `row` of the tile: the chunk row that is the query itself (query_ids)

  for (int i = tid; i < KNN_K * BM; i += 256) {
    listD[i] = INFINITY;
    listI[i] = -1;
  }
  if (tid < BM) {
    const bool in = q0 + tid < g.q;
    sQn[tid] = in ? g.qn[q0 + tid] : 0.f;
    const int64_t self = in && g.query_ids ? g.query_ids[q0 + tid] - g.index_offset : -1;
    skip = self >= 0 && self < g.n ? (int)self : -1;
  }
  __syncthreads();

  for (int t = t_lo; t < t_hi; ++t) {
    const int g0 = t * KNN_GT;
    f32x16 acc[QB], accn;
    pair_tile_dots<QB, F16, GN>(Q, G, q0, g0, g.q, g.n, g.d, vec, sA, sB, acc, accn);

    // acc[qb][r]: query row 32 qb + (r & 3) + 8 (r >> 2) + 4 kg, gallery column g0 + 32 wid + i32.  The waves take turns to
    // stage their 32 columns of distances (NaN: no such gallery row); each query's thread filters and inserts.  Eight
    // barriers a tile, against two per 32 of d in the loop above.
    const int gcol = g0 + wid * 32 + i32;
    const bool gvalid = gcol < g.n;
    float gnv = 0.f;
    if constexpr (GN) {      // column i's norm is element (i, i): lane (i, kg = (i >> 2) & 1), register 4 (i >> 3) + (i & 3)
      // registers 4 a + c of the lanes with kg == b hold rows 8 a + 4 b + c: two selects on the lane's own a and c
      const int a = i32 >> 3, c = i32 & 3;
      f32x4 quad;
#pragma unroll
      for (int j = 0; j < 4; ++j) quad[j] = a == 0 ? accn[j] : a == 1 ? accn[4 + j] : a == 2 ? accn[8 + j] : accn[12 + j];
      const float v = c == 0 ? quad[0] : c == 1 ? quad[1] : c == 2 ? quad[2] : quad[3];
      if (kg == ((i32 >> 2) & 1)) sGn[wid * 32 + i32] = v;
    } else if (gvalid) {
      gnv = g.gn[gcol];
    }
    float* stage = reinterpret_cast<float*>(smem);
    __syncthreads();      // every fragment read of smem is done; the tile's norms are in sGn
    if constexpr (GN) gnv = sGn[wid * 32 + i32];
#pragma unroll 1
    for (int w = 0; w < 4; ++w) {
      if (wid == w) {
#pragma unroll
        for (int qb = 0; qb < QB; ++qb)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int row = qb * 32 + (r & 3) + 8 * (r >> 2) + 4 * kg;
            const float dv = knn_distance(g.metric, sQn[row], gnv, acc[qb][r]);
            stage[row * KNN_SW + i32] = gvalid ? dv : NAN;
          }
      }
      __syncthreads();
      if (tid < BM && q0 + tid < g.q) knn_scan(stage + tid * KNN_SW, listD + tid, listI + tid, BM, g.k, g0 + w * 32, skip);
      __syncthreads();
    }
  }
  __syncthreads();
  knn_write_partial<BM>(g, listD, listI, q0, split);
}

// any dtype: 8 queries x 32 gallery rows per step, one thread per pair, one fmaf chain over d (the fp32 exact-parity path)
template <typename T>
__global__ __launch_bounds__(256) void knn_valu_kernel(const T* __restrict__ Q, const T* __restrict__ G, const KnnGeom g) {
  constexpr int BM = 8;
  __shared__ float stage[BM * KNN_SW];
  __shared__ float listD[KNN_K * BM];
  __shared__ int listI[KNN_K * BM];
  const int tid = threadIdx.x, qr = tid >> 5, c = tid & 31;
  const int q0 = blockIdx.x * BM, split = blockIdx.y;
  // tiles < 2^24 and splits <= 256: the products fit 32 bits
  const int t_lo = (int)((unsigned)split * (unsigned)g.tiles / (unsigned)g.splits);
  const int t_hi = (int)((unsigned)(split + 1) * (unsigned)g.tiles / (unsigned)g.splits);
  for (int i = tid; i < KNN_K * BM; i += 256) {
    listD[i] = INFINITY;
    listI[i] = -1;
  }
  const bool qin = q0 + qr < g.q;
  const T* qp = Q + (size_t)(qin ? q0 + qr : 0) * g.d;
  const float qnv = qin ? g.qn[q0 + qr] : 0.f;
  const int64_t self = qin && g.query_ids ? g.query_ids[q0 + qr] - g.index_offset : -1;
  const int skip = self >= 0 && self < g.n ? (int)self : -1;
  __syncthreads();
  for (int t = t_lo; t < t_hi; ++t)
    for (int sub = 0; sub < KNN_GT / 32; ++sub) {
      const int first = t * KNN_GT + sub * 32;
      if (first >= g.n) break;
      const int gcol = first + c;
      float dv = NAN;
      if (qin && gcol < g.n && gcol != skip) {
        const T* gp = G + (size_t)gcol * g.d;
        dv = knn_distance(g.metric, qnv, g.gn[gcol], pair_dot_chain(qp, gp, g.d));
      }
      stage[qr * KNN_SW + c] = dv;
      __syncthreads();
      if (tid < BM) knn_scan(stage + tid * KNN_SW, listD + tid, listI + tid, BM, g.k, first, -1);
      __syncthreads();
    }
  knn_write_partial<BM>(g, listD, listI, q0, split);
}

// one thread per query: the incoming table, then every split's partial list in split order, through the same insertion
__global__ __launch_bounds__(64) void knn_merge_kernel(const KnnGeom g, float* __restrict__ dist, int64_t* __restrict__ idx) {
  __shared__ float mD[KNN_K * 64];
  __shared__ int64_t mI[KNN_K * 64];
  const int t = threadIdx.x;
  const int64_t qrow = (int64_t)blockIdx.x * 64 + t;
  if (qrow >= g.q) return;
  for (int j = 0; j < g.k; ++j) {
    mD[j * 64 + t] = INFINITY;
    mI[j * 64 + t] = -1;
  }
  for (int j = 0; j < g.k; ++j) knn_insert<int64_t>(mD + t, mI + t, 64, g.k, dist[qrow * g.k + j], idx[qrow * g.k + j]);
  for (int s = 0; s < g.splits; ++s)
    for (int j = 0; j < g.k; ++j) {
      const size_t off = ((size_t)s * g.q + qrow) * g.k + j;
      const int li = g.part_i[off];
      // a partial list ascends: after its first filler, or its first entry that does not get in, nothing of it does
      if (li < 0 || !knn_insert<int64_t>(mD + t, mI + t, 64, g.k, g.part_d[off], g.index_offset + li)) break;
    }
  for (int j = 0; j < g.k; ++j) {
    dist[qrow * g.k + j] = mD[j * 64 + t];
    idx[qrow * g.k + j] = mI[j * 64 + t];
  }
}

// Squared norms by the SAME reduction as the search's dot product of the row with itself, so that the squared L2 distance
// of a row to a bitwise copy of it is exactly 0.  fp32: the one fmaf chain.
__global__ __launch_bounds__(256) void knn_sqnorm_f32_kernel(const float* __restrict__ x, float* __restrict__ out, int64_t rows, int d) {
  const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (row >= rows) return;
  const float* p = x + (size_t)row * d;
  float acc = 0.f;
  for (int i = 0; i < d; ++i) acc = fmaf(p[i], p[i], acc);
  out[row] = acc;
}

// 16-bit: a wave takes 32 rows and runs the search's MFMA chain on them against themselves, both operands one register (lane
// l: row l % 32, k 8 (l / 32) .. of the step's 16); row i's norm is the diagonal element (i, i) of the 32 x 32 result, which
// lives in lane (i, kg = (i >> 2) & 1) at register 4 (i >> 3) + (i & 3).  32 MACs per element read: the price of the exact 0.
template <bool F16>
__global__ __launch_bounds__(256) void knn_sqnorm_mfma_kernel(const bf16* __restrict__ x, float* __restrict__ out, int rows, int d, int vec) {
  const int lane = threadIdx.x & 63, i32 = lane & 31, kg = lane >> 5;
  const int r0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 32;
  if (r0 >= rows) return;      // a whole wave
  f32x16 acc;
#pragma unroll
  for (int j = 0; j < 16; ++j) acc[j] = 0.f;
  const int dpad = (d + 31) & ~31;      // as many steps as the search runs
  for (int k0 = 0; k0 < dpad; k0 += 16) {
    const bf16x8 a = knn_load8(x, r0 + i32, k0 + kg * 8, rows, d, vec != 0);
    acc = mfma_32x32x16<F16>(a, a, acc);
  }
  const int rsel = 4 * (i32 >> 3) + (i32 & 3);
  float v = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r)
    if (r == rsel) v = acc[r];
  if (kg == ((i32 >> 2) & 1) && r0 + i32 < rows) out[r0 + i32] = v;
}

constexpr int64_t KNN_MAX_ROWS = (1ll << 31) - 1024;

int knn_plan(int64_t q, int64_t n, int d, int k, int* splits, int* tiles) {
  TG_CHECK(q >= 1 && q <= KNN_MAX_ROWS, TG_EINVAL, "tg_knn: q = %lld outside 1 .. 2^31 - 1024", (long long)q);
  TG_CHECK(n >= 1 && n <= KNN_MAX_ROWS, TG_EINVAL, "tg_knn: n = %lld outside 1 .. 2^31 - 1024", (long long)n);
  TG_CHECK(d >= 1 && d <= (1 << 30), TG_EINVAL, "tg_knn: d = %d outside 1 .. 2^30", d);
  TG_CHECK(k >= 1 && k <= TG_KNN_MAX_K, TG_EINVAL, "tg_knn: k = %d outside 1 .. %d", k, TG_KNN_MAX_K);
  const int64_t t = (n + KNN_GT - 1) / KNN_GT, q32 = (q + 31) / 32, want = (1024 + q32 - 1) / q32;
  int64_t s = want < 256 ? want : 256;
  if (s > t) s = t;
  *tiles = (int)t;
  *splits = (int)s;
  return TG_OK;
}

void knn_sqnorm_launch(const void* x, int64_t rows, int d, int dtype, float* out, hipStream_t s) {
  if (dtype == TG_F32) {
    hipLaunchKernelGGL(knn_sqnorm_f32_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, (const float*)x, out, rows, d);
    return;
  }
  const int vec = d % 8 == 0 && tg_aligned16(x) ? 1 : 0;
  const dim3 grid((unsigned)((rows + 127) / 128));
  if (dtype == TG_F16)
    hipLaunchKernelGGL(knn_sqnorm_mfma_kernel<true>, grid, dim3(256), 0, s, (const bf16*)x, out, (int)rows, d, vec);
  else
    hipLaunchKernelGGL(knn_sqnorm_mfma_kernel<false>, grid, dim3(256), 0, s, (const bf16*)x, out, (int)rows, d, vec);
}

// ---- kernel two-sample block sums (include/twingan_hip_mmd.h) --------------------------------------------------------------
// The search's sibling: the same staged dot products (pair_tile_dots / pair_dot_chain), and an epilogue that turns each into
// the polynomial kernel's value and adds it up instead of selecting.  The unit of summation is 32 x 32 pairs -- one wave's
// MFMA block, and since a block of the result is a multiple of 32 rows on either side a unit never straddles two blocks.
// Every pair value is widened to fp64 as it is added: lane, then the unit's lanes in lane order through LDS, one fp64 per
// unit to the workspace; mmd_merge_kernel adds a block's units in a fixed order.  No atomics, nothing depends on arrival.
struct MmdGeom {
  int m, n, d, degree, vec, skip, tm, tn;      // tm x tn units
  float gamma, coef0;
  int64_t delta;      // b_index0 - a_index0: with `skip` the pair (i, j) with i - j == delta is left out
  double* unit;       // [tm][tn]
};

__device__ __forceinline__ float mmd_pair(const MmdGeom& g, float s) {
  const float t = fmaf(g.gamma, s, g.coef0);
  float p = t;
  for (int k = 1; k < g.degree; ++k) p = p * t;
  return p;
}

__device__ __forceinline__ bool mmd_takes(const MmdGeom& g, int row, int col) {
  return row < g.m && col < g.n && !(g.skip && (int64_t)row - (int64_t)col == g.delta);
}

constexpr int MMD_QB = 4;        // 128 rows of `a` per workgroup, as the search's widest tile
constexpr int MMD_RW = 17;       // doubles per lane of the reduction buffer (16 units of a workgroup + 1: no bank conflicts)

template <bool F16>
__global__ __launch_bounds__(256, 2) void mmd_mfma_kernel(const bf16* __restrict__ A, const bf16* __restrict__ B, const MmdGeom g) {
  constexpr int A_BYTES = 32 * MMD_QB * KNN_ROW, B_BYTES = KNN_GT * KNN_ROW;
  static_assert(64 * MMD_RW * 8 <= A_BYTES + B_BYTES, "the reduction buffer reuses the operand tiles");
  __shared__ __attribute__((aligned(16))) unsigned char smem[A_BYTES + B_BYTES];      // operand tiles; the lanes' sums afterwards
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, i32 = lane & 31, kg = lane >> 5;
  const int a0 = blockIdx.x * (32 * MMD_QB), b0 = blockIdx.y * KNN_GT;
  f32x16 acc[MMD_QB], accn;
  pair_tile_dots<MMD_QB, F16, false>(A, B, a0, b0, g.m, g.n, g.d, g.vec != 0, smem, smem + A_BYTES, acc, accn);

  // acc[qb][r]: row a0 + 32 qb + (r & 3) + 8 (r >> 2) + 4 kg of `a`, row b0 + 32 wid + i32 of `b`; unit (qb, wid)
  double* red = reinterpret_cast<double*>(smem);
  const int col = b0 + wid * 32 + i32;
  __syncthreads();      // every fragment read of smem is done
#pragma unroll
  for (int qb = 0; qb < MMD_QB; ++qb) {
    double sum = 0.0;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = a0 + qb * 32 + (r & 3) + 8 * (r >> 2) + 4 * kg;
      const float p = mmd_pair(g, acc[qb][r]);
      sum += mmd_takes(g, row, col) ? (double)p : 0.0;      // a select: what a zero-filled row made of a NaN stays out
    }
    red[lane * MMD_RW + qb * 4 + wid] = sum;
  }
  __syncthreads();
  if (tid < 4 * MMD_QB) {
    const int ur = a0 / 32 + (tid >> 2), uc = b0 / 32 + (tid & 3);
    if (ur < g.tm && uc < g.tn) {
      double sum = 0.0;
      for (int l = 0; l < 64; ++l) sum += red[l * MMD_RW + tid];
      g.unit[(size_t)ur * g.tn + uc] = sum;
    }
  }
}

// fp32, the exact-parity path: a workgroup per unit, thread (r8, c) takes rows r8, r8 + 8, r8 + 16, r8 + 24 against column c
__global__ __launch_bounds__(256) void mmd_valu_kernel(const float* __restrict__ A, const float* __restrict__ B, const MmdGeom g) {
  __shared__ double red[256 + 16];
  const int tid = threadIdx.x, c = tid & 31, r8 = tid >> 5;
  const int col = blockIdx.y * 32 + c;
  double sum = 0.0;
  if (col < g.n) {
    const float* bp = B + (size_t)col * g.d;
#pragma unroll 1
    for (int k = 0; k < 4; ++k) {
      const int row = blockIdx.x * 32 + r8 + 8 * k;
      if (mmd_takes(g, row, col)) sum += (double)mmd_pair(g, pair_dot_chain(A + (size_t)row * g.d, bp, g.d));
    }
  }
  red[tid] = sum;
  __syncthreads();
  if (tid < 16) {
    double part = 0.0;
    for (int i = 0; i < 16; ++i) part += red[tid * 16 + i];
    red[256 + tid] = part;
  }
  __syncthreads();
  if (tid == 0) {
    double total = 0.0;
    for (int i = 0; i < 16; ++i) total += red[256 + i];
    g.unit[(size_t)blockIdx.x * g.tn + blockIdx.y] = total;
  }
}

// block (I, J) of the result: its bu x bu units (fewer at the edges), row-major, dealt to 64 threads, the threads' sums in order
__global__ __launch_bounds__(64) void mmd_merge_kernel(const MmdGeom g, int bu, int nbj, double* __restrict__ sums) {
  __shared__ double red[64];
  const int t = threadIdx.x;
  const int r_lo = blockIdx.x * bu, c_lo = blockIdx.y * bu;
  const int rows = (g.tm - r_lo < bu ? g.tm - r_lo : bu), cols = (g.tn - c_lo < bu ? g.tn - c_lo : bu);
  const int64_t count = (int64_t)rows * cols;
  double sum = 0.0;
  for (int64_t u = t; u < count; u += 64) sum += g.unit[(size_t)(r_lo + u / cols) * g.tn + (c_lo + u % cols)];
  red[t] = sum;
  __syncthreads();
  if (t == 0) {
    double total = 0.0;
    for (int i = 0; i < 64; ++i) total += red[i];
    sums[(size_t)blockIdx.x * nbj + blockIdx.y] = total;
  }
}

constexpr int64_t MMD_MAX_ROWS = 1ll << 20;

int mmd_plan(int64_t m, int64_t n, int d, int block, int* tm, int* tn) {
  TG_CHECK(m >= 1 && m <= MMD_MAX_ROWS, TG_EINVAL, "tg_mmd: m = %lld outside 1 .. 2^20", (long long)m);
  TG_CHECK(n >= 1 && n <= MMD_MAX_ROWS, TG_EINVAL, "tg_mmd: n = %lld outside 1 .. 2^20", (long long)n);
  TG_CHECK(d >= 1 && d <= (1 << 30), TG_EINVAL, "tg_mmd: d = %d outside 1 .. 2^30", d);
  TG_CHECK(block >= 32 && block % 32 == 0, TG_EINVAL, "tg_mmd: block = %d is not a multiple of 32 that is >= 32", block);
  *tm = (int)((m + 31) / 32);
  *tn = (int)((n + 31) / 32);
  return TG_OK;
}

}  // namespace

extern "C" {

int tg_batched_gemm(const void* a, const void* b, void* c, int batch, int m, int n, int k, int ta, int tb, int lda, int ldb,
                    int ldc, int64_t stride_a, int64_t stride_b, int64_t stride_c, float alpha, int accumulate, int dtype,
                    int c_is_f32, void* stream) {
  TG_CHECK(a && b && c && batch > 0 && m > 0 && n > 0 && k > 0, TG_EINVAL, "tg_batched_gemm: bad arguments");
  TG_CHECK(dtype == TG_F32 || dtype == TG_BF16 || dtype == TG_F16, TG_EINVAL, "tg_batched_gemm: dtype %d", dtype);
  BgGeom g;
  g.m = m; g.n = n; g.k = k; g.lda = lda; g.ldb = ldb; g.ldc = ldc;
  g.sa = stride_a; g.sb = stride_b; g.sc = stride_c;
  g.alpha = alpha; g.accumulate = accumulate; g.c_f32 = c_is_f32 || dtype == TG_F32;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == TG_F32) {
    g.vec = 0;
    const dim3 grid(tg_grid_for((int64_t)m * n, 256, 4096), batch);
    hipLaunchKernelGGL(bgemm_simple_kernel<float>, grid, dim3(256), 0, s, (const float*)a, (const float*)b, c, g, ta, tb);
    TG_LAUNCH_CHECK("tg_batched_gemm(f32)");
    return TG_OK;
  }
  // 16-byte vector staging needs every contiguous run to be a multiple of 8 elements at a 16-byte aligned address
  const int ca = ta ? m : k, cb = tb ? k : n;      // contiguous extents of A and B
  g.vec = (ca % 8 == 0 && cb % 8 == 0 && lda % 8 == 0 && ldb % 8 == 0 && stride_a % 8 == 0 && stride_b % 8 == 0 &&
           tg_aligned16(a) && tg_aligned16(b)) ? 1 : 0;
  const dim3 grid((n + BN - 1) / BN, (m + BM - 1) / BM, batch);
  const bool akc = !ta, bkc = tb != 0;
  tg_note_kernel("bgemm_mfma_kernel<%d,%d>", (int)akc, (int)bkc);
#define TG_BG_LAUNCH(A_, B_)                                                                                            \
  do {                                                                                                                \
    if (dtype == TG_F16)                                                                                              \
      hipLaunchKernelGGL((bgemm_mfma_kernel<A_, B_, true>), grid, dim3(256), 0, s, (const bf16*)a, (const bf16*)b, c, g); \
    else                                                                                                              \
      hipLaunchKernelGGL((bgemm_mfma_kernel<A_, B_>), grid, dim3(256), 0, s, (const bf16*)a, (const bf16*)b, c, g);     \
  } while (0)
  if (akc && bkc) TG_BG_LAUNCH(true, true);
  else if (akc) TG_BG_LAUNCH(true, false);
  else if (bkc) TG_BG_LAUNCH(false, true);
  else TG_BG_LAUNCH(false, false);
#undef TG_BG_LAUNCH
  TG_LAUNCH_CHECK("tg_batched_gemm");
  return TG_OK;
}

int tg_softmax_rows_fwd(const void* s, void* p, int64_t rows, int cols, int dtype, void* stream) {
  TG_CHECK(s && p && rows > 0 && cols > 0, TG_EINVAL, "tg_softmax_rows_fwd: bad arguments");
  TG_DISPATCH_DTYPE(dtype, "tg_softmax_rows_fwd", {
    hipLaunchKernelGGL(softmax_rows_fwd_kernel<T>, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, (const T*)s, (T*)p, cols);
  });
  TG_LAUNCH_CHECK("tg_softmax_rows_fwd");
  return TG_OK;
}

int tg_softmax_rows_bwd(const void* p, const void* dp, void* ds, int64_t rows, int cols, int dtype, void* stream) {
  TG_CHECK(p && dp && ds && rows > 0 && cols > 0, TG_EINVAL, "tg_softmax_rows_bwd: bad arguments");
  TG_DISPATCH_DTYPE(dtype, "tg_softmax_rows_bwd", {
    hipLaunchKernelGGL(softmax_rows_bwd_kernel<T>, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, (const T*)p,
                       (const T*)dp, (T*)ds, cols);
  });
  TG_LAUNCH_CHECK("tg_softmax_rows_bwd");
  return TG_OK;
}

int tg_softmax_rows_bwd_bwd(const void* p, const void* dp, const void* v, void* gp, int64_t rows, int cols, int dtype,
                            void* stream) {
  TG_CHECK(p && dp && v && gp && rows > 0 && cols > 0, TG_EINVAL, "tg_softmax_rows_bwd_bwd: bad arguments");
  TG_DISPATCH_DTYPE(dtype, "tg_softmax_rows_bwd_bwd", {
    hipLaunchKernelGGL(softmax_rows_bwd_bwd_kernel<T>, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, (const T*)p,
                       (const T*)dp, (const T*)v, (T*)gp, cols);
  });
  TG_LAUNCH_CHECK("tg_softmax_rows_bwd_bwd");
  return TG_OK;
}

int tg_tanh_fwd(const void* x, void* y, int64_t numel, int dtype, void* stream) {
  TG_CHECK(x && y && numel > 0, TG_EINVAL, "tg_tanh_fwd: bad arguments");
  TG_DISPATCH_DTYPE(dtype, "tg_tanh_fwd", {
    hipLaunchKernelGGL(tanh_fwd_kernel<T>, dim3(tg_grid_for(numel, 256)), dim3(256), 0, (hipStream_t)stream, (const T*)x, (T*)y, numel);
  });
  TG_LAUNCH_CHECK("tg_tanh_fwd");
  return TG_OK;
}

int tg_tanh_bwd(const void* g, const void* y, void* gx, int64_t numel, int dtype, void* stream) {
  TG_CHECK(g && y && gx && numel > 0, TG_EINVAL, "tg_tanh_bwd: bad arguments");
  TG_DISPATCH_DTYPE(dtype, "tg_tanh_bwd", {
    hipLaunchKernelGGL(tanh_bwd_kernel<T>, dim3(tg_grid_for(numel, 256)), dim3(256), 0, (hipStream_t)stream, (const T*)g,
                       (const T*)y, (T*)gx, numel);
  });
  TG_LAUNCH_CHECK("tg_tanh_bwd");
  return TG_OK;
}

int tg_mul3(const void* a, const void* b, const void* c, void* out, float scale, int64_t numel, int dtype, void* stream) {
  TG_CHECK(a && b && out && numel > 0, TG_EINVAL, "tg_mul3: bad arguments");
  TG_DISPATCH_DTYPE(dtype, "tg_mul3", {
    hipLaunchKernelGGL(mul3_kernel<T>, dim3(tg_grid_for(numel, 256)), dim3(256), 0, (hipStream_t)stream, (const T*)a,
                       (const T*)b, (const T*)c, (T*)out, scale, numel);
  });
  TG_LAUNCH_CHECK("tg_mul3");
  return TG_OK;
}

int tg_scale_dev(const void* x, const float* scalar, void* out, int64_t numel, int dtype, void* stream) {
  TG_CHECK(x && scalar && out && numel > 0, TG_EINVAL, "tg_scale_dev: bad arguments");
  TG_DISPATCH_DTYPE(dtype, "tg_scale_dev", {
    hipLaunchKernelGGL(scale_dev_kernel<T>, dim3(tg_grid_for(numel, 256)), dim3(256), 0, (hipStream_t)stream, (const T*)x,
                       scalar, (T*)out, numel);
  });
  TG_LAUNCH_CHECK("tg_scale_dev");
  return TG_OK;
}

// out[0] = sum a * b; ws: >= 1024 floats of scratch (two-stage, fixed order)
int tg_dot(const void* a, const void* b, float* out, float* ws, int64_t numel, int dtype, void* stream) {
  TG_CHECK(a && b && out && ws && numel > 0, TG_EINVAL, "tg_dot: bad arguments");
  int nparts = (int)((numel + 16383) / 16384);
  if (nparts > 1024) nparts = 1024;
  const int64_t per = (numel + nparts - 1) / nparts;
  TG_DISPATCH_DTYPE(dtype, "tg_dot", {
    hipLaunchKernelGGL(dot_partial_kernel<T>, dim3(nparts), dim3(256), 0, (hipStream_t)stream, (const T*)a, (const T*)b, ws,
                       numel, per);
  });
  hipLaunchKernelGGL(dot_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, ws, nparts, out);
  TG_LAUNCH_CHECK("tg_dot");
  return TG_OK;
}

// ---- include/twingan_hip_knn.h ---------------------------------------------------------------------------------------------
int tg_knn_sqnorm(const void* x, int64_t rows, int d, int dtype, float* out_f32, void* stream) {
  TG_CHECK(x && out_f32, TG_EINVAL, "tg_knn_sqnorm: NULL pointer");
  TG_CHECK(rows >= 1 && rows <= KNN_MAX_ROWS && d >= 1 && d <= (1 << 30), TG_EINVAL, "tg_knn_sqnorm: rows = %lld, d = %d",
           (long long)rows, d);
  TG_CHECK(dtype == TG_F32 || dtype == TG_BF16 || dtype == TG_F16, TG_EINVAL, "tg_knn_sqnorm: dtype %d", dtype);
  knn_sqnorm_launch(x, rows, d, dtype, out_f32, (hipStream_t)stream);
  TG_LAUNCH_CHECK("tg_knn_sqnorm");
  return TG_OK;
}

int tg_knn_plan(int64_t q, int64_t n, int d, int k, int* splits) {
  TG_CHECK(splits, TG_EINVAL, "tg_knn_plan: splits is NULL");
  int tiles = 0;
  return knn_plan(q, n, d, k, splits, &tiles);
}

size_t tg_knn_workspace_bytes(int64_t q, int64_t n, int d, int k) {
  int splits = 0, tiles = 0;
  if (knn_plan(q, n, d, k, &splits, &tiles) != TG_OK) return 0;
  return 4 * (2 * (size_t)splits * (size_t)q * (size_t)k + (size_t)q + (size_t)n);
}

int tg_knn_topk(const void* queries, int64_t q, const void* gallery, int64_t n, int d, int dtype, int metric, int k,
                int64_t index_offset, const int64_t* query_ids, float* dist, int64_t* idx, void* ws, size_t ws_bytes,
                void* stream) {
  TG_CHECK(queries && gallery && dist && idx && ws, TG_EINVAL, "tg_knn_topk: NULL pointer");
  TG_CHECK(dtype == TG_F32 || dtype == TG_BF16 || dtype == TG_F16, TG_EINVAL, "tg_knn_topk: dtype %d", dtype);
  TG_CHECK(metric == TG_KNN_L2 || metric == TG_KNN_COSINE, TG_EINVAL, "tg_knn_topk: metric %d", metric);
  TG_CHECK(index_offset >= 0, TG_EINVAL, "tg_knn_topk: index_offset %lld < 0", (long long)index_offset);
  KnnGeom g;
  const int rc = knn_plan(q, n, d, k, &g.splits, &g.tiles);
  if (rc != TG_OK) return rc;
  const size_t parts = (size_t)g.splits * (size_t)q * (size_t)k;
  TG_CHECK((reinterpret_cast<uintptr_t>(ws) & 3u) == 0, TG_EINVAL, "tg_knn_topk: workspace not 4-byte aligned");
  TG_CHECK(ws_bytes >= 4 * (2 * parts + (size_t)q + (size_t)n), TG_EINVAL, "tg_knn_topk: workspace of %zu bytes, %zu needed", ws_bytes,
           4 * (2 * parts + (size_t)q + (size_t)n));
  g.q = (int)q; g.n = (int)n; g.d = d; g.k = k; g.metric = metric;
  g.index_offset = index_offset;
  g.query_ids = query_ids;
  g.part_i = reinterpret_cast<int*>(ws);
  g.part_d = reinterpret_cast<float*>(ws) + parts;
  float* qn = g.part_d + parts;
  float* gn = qn + q;
  g.qn = qn;
  g.gn = gn;
  g.vec = (d % 8 == 0 && tg_aligned16(queries) && tg_aligned16(gallery)) ? 1 : 0;
  hipStream_t s = (hipStream_t)stream;
  knn_sqnorm_launch(queries, q, d, dtype, qn, s);
  const int qb = q <= 32 ? 1 : q <= 64 ? 2 : 4;      // query tile of 32, 64 or 128: no MFMA rows for queries that are not there
  if (dtype == TG_F32 || qb == 4) knn_sqnorm_launch(gallery, n, d, dtype, gn, s);      // else the tile kernel takes them itself
  if (dtype == TG_F32) {
    hipLaunchKernelGGL(knn_valu_kernel<float>, dim3((unsigned)((q + 7) / 8), g.splits), dim3(256), 0, s, (const float*)queries,
                       (const float*)gallery, g);
  } else {
    const dim3 grid((unsigned)((q + 32 * qb - 1) / (32 * qb)), g.splits);
    tg_note_kernel("knn_mfma_kernel<%d>", qb);
#define TG_KNN_LAUNCH(QB_)                                                                                                  \
  do {                                                                                                                    \
    if (dtype == TG_F16)                                                                                                  \
      hipLaunchKernelGGL((knn_mfma_kernel<QB_, true>), grid, dim3(256), 0, s, (const bf16*)queries, (const bf16*)gallery, g);  \
    else                                                                                                                  \
      hipLaunchKernelGGL((knn_mfma_kernel<QB_, false>), grid, dim3(256), 0, s, (const bf16*)queries, (const bf16*)gallery, g); \
  } while (0)
    if (qb == 1) TG_KNN_LAUNCH(1);
    else if (qb == 2) TG_KNN_LAUNCH(2);
    else TG_KNN_LAUNCH(4);
#undef TG_KNN_LAUNCH
  }
  hipLaunchKernelGGL(knn_merge_kernel, dim3((unsigned)((q + 63) / 64)), dim3(64), 0, s, g, dist, idx);
  TG_LAUNCH_CHECK("tg_knn_topk");
  return TG_OK;
}

// ---- include/twingan_hip_mmd.h ---------------------------------------------------------------------------------------------
size_t tg_mmd_workspace_bytes(int64_t m, int64_t n, int d, int block) {
  int tm = 0, tn = 0;
  if (mmd_plan(m, n, d, block, &tm, &tn) != TG_OK) return 0;
  return (size_t)tm * tn * sizeof(double);
}

int tg_mmd_block_sums(const void* a, int64_t m, const void* b, int64_t n, int d, int dtype, int degree, float gamma, float coef0,
                      int block, int64_t a_index0, int64_t b_index0, int skip_same_index, double* sums, void* ws, size_t ws_bytes,
                      void* stream) {
  MmdGeom g;
  const int rc = mmd_plan(m, n, d, block, &g.tm, &g.tn);
  if (rc != TG_OK) return rc;
  TG_CHECK(a && b && sums && ws, TG_EINVAL, "tg_mmd_block_sums: NULL pointer");
  TG_CHECK(dtype == TG_F32 || dtype == TG_BF16 || dtype == TG_F16, TG_EINVAL, "tg_mmd_block_sums: dtype %d", dtype);
  TG_CHECK(degree >= 1 && degree <= TG_MMD_MAX_DEGREE, TG_EINVAL, "tg_mmd_block_sums: degree = %d outside 1 .. %d", degree,
           TG_MMD_MAX_DEGREE);
  TG_CHECK(a_index0 >= 0, TG_EINVAL, "tg_mmd_block_sums: a_index0 %lld < 0", (long long)a_index0);
  TG_CHECK(b_index0 >= 0, TG_EINVAL, "tg_mmd_block_sums: b_index0 %lld < 0", (long long)b_index0);
  const size_t need = (size_t)g.tm * g.tn * sizeof(double);
  TG_CHECK((reinterpret_cast<uintptr_t>(ws) & 7u) == 0, TG_EINVAL, "tg_mmd_block_sums: workspace not 8-byte aligned");
  TG_CHECK(ws_bytes >= need, TG_EINVAL, "tg_mmd_block_sums: workspace of %zu bytes, %zu needed", ws_bytes, need);
  hipStream_t s = (hipStream_t)stream;
  g.m = (int)m; g.n = (int)n; g.d = d; g.degree = degree;
  g.gamma = gamma; g.coef0 = coef0;
  g.skip = skip_same_index ? 1 : 0;
  g.delta = b_index0 - a_index0;
  g.unit = (double*)ws;
  g.vec = d % 8 == 0 && tg_aligned16(a) && tg_aligned16(b) ? 1 : 0;
  if (dtype == TG_F32) {
    tg_note_kernel("mmd_valu_kernel");
    hipLaunchKernelGGL(mmd_valu_kernel, dim3(g.tm, g.tn), dim3(256), 0, s, (const float*)a, (const float*)b, g);
  } else {
    const dim3 grid((g.tm + MMD_QB - 1) / MMD_QB, (g.tn + 3) / 4);
    tg_note_kernel("mmd_mfma_kernel");
    if (dtype == TG_F16)
      hipLaunchKernelGGL(mmd_mfma_kernel<true>, grid, dim3(256), 0, s, (const bf16*)a, (const bf16*)b, g);
    else
      hipLaunchKernelGGL(mmd_mfma_kernel<false>, grid, dim3(256), 0, s, (const bf16*)a, (const bf16*)b, g);
  }
  const int bu = block / 32, nbi = (g.tm + bu - 1) / bu, nbj = (g.tn + bu - 1) / bu;
  hipLaunchKernelGGL(mmd_merge_kernel, dim3(nbi, nbj), dim3(64), 0, s, g, bu, nbj, sums);
  TG_LAUNCH_CHECK("tg_mmd_block_sums");
  return TG_OK;
}

}  // extern "C"
