// Minibatch-stddev (forward, backward, double backward), loss reductions, WGAN-GP tail, the small
// dense layer, the fused Adam step and the other --optimizer rules' apply.
#include "tg_common.h"
#include "../../include/twingan_hip_optim.h"
#include "../../include/twingan_hip_summary.h"

namespace {

// The n (<= 16) samples of V consecutive positions, all requested before any is used: a runtime-length load/use
// loop is one L2 round trip per sample (3 such loops made these single-workgroup kernels 20-90 us).
constexpr int MB_NMAX = 16;
// A thread's POSITION vector is 8 bytes (4 positions of a 16-bit type, 2 of fp32), not 16: the [16, 4, 4, 256] tensor then
// spreads over 1024 threads instead of 512 -- these kernels' time is the per-thread chain (16 samples x V conversions,
// sums, a division or two per position), not bytes; with 16-byte vectors half of the forward's 1024 threads idled and the
// backward kernels needed 226-256 VGPRs.
template <typename T, int V>
struct alignas(sizeof(T) * V) MbVec {
  T e[V];
  __device__ __forceinline__ float get(int i) const { return (float)e[i]; }
  __device__ __forceinline__ void set(int i, float x) { e[i] = (T)x; }
};
template <typename T> constexpr int mb_v() { return 8 / (int)sizeof(T); }
template <typename T, int V> __device__ __forceinline__ MbVec<T, V> mb_ld(const T* p) {
  return *reinterpret_cast<const MbVec<T, V>*>(p);
}
template <typename T, int V> __device__ __forceinline__ void mb_st(T* p, const MbVec<T, V>& v) {
  *reinterpret_cast<MbVec<T, V>*>(p) = v;
}
template <typename T, int V>
__device__ __forceinline__ void mb_load_samples(const T* __restrict__ x, int n, int P, int p, MbVec<T, V> (&xv)[MB_NMAX]) {
#pragma unroll
  for (int i = 0; i < MB_NMAX; ++i) xv[i] = mb_ld<T, V>(x + (int64_t)(i < n ? i : n - 1) * P + p);
}


// out[px][0..c) = src[px][0..c), out[px][c] = val, out[px][c+1..cpad) = 0 over nvec 16-byte vectors of the padded tensor,
// U vectors per thread in flight (a load -> store loop of one vector per trip is one L2 round trip per trip; U = 9 with
// 1024 threads takes the [16, 4, 4, 264] tensor in ONE trip)
template <typename T, int U = 4>
__device__ __forceinline__ void mb_copy_with_stat(const T* __restrict__ src, T* __restrict__ out, int64_t nvec, int c,
                                                  int cpad, float val) {
  constexpr int V = Vec16<T>::N;
  const int cvp = cpad / V;
  for (int64_t i0 = threadIdx.x; i0 < nvec; i0 += (int64_t)blockDim.x * U) {
    Vec16<T> o[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      int64_t i = i0 + (int64_t)u * blockDim.x;
      i = i < nvec ? i : nvec - 1;
      const int cb = (int)(i % cvp) * V;
      const int64_t px = i / cvp;
      if (cb < c) {
        o[u] = ldv(src + px * c + cb);
      } else {
#pragma unroll
        for (int j = 0; j < V; ++j) o[u].set(j, (cb + j == c) ? val : 0.f);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = i0 + (int64_t)u * blockDim.x;
      if (i < nvec) stv(out + (i / cvp) * cpad + (int)(i % cvp) * V, o[u]);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// Minibatch stddev, nets/pggan_utils.py:353-366.  x[n][p], p = hw*c.  Single workgroup: the tensor
// is [B,4,4,C] (64 K elements at B=16, C=256).
//   stat = mean_p sqrt(var_n(x[:,p]) + eps)          (biased variance over the batch)
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(1024) void mbstd_fwd_kernel(const T* __restrict__ x, T* __restrict__ out,
                                                         float* __restrict__ stat, int n, int hw, int c, int cpad,
                                                         float eps) {
  __shared__ float red[16];
  const int P = hw * c;
  // one workgroup per statistic group of n images (blockIdx.x): the reference computes the statistic per
  // discriminator call; several calls batched along N keep their own statistic
  x += (int64_t)blockIdx.x * n * P;
  out += (int64_t)blockIdx.x * n * hw * cpad;
  if (stat) stat += blockIdx.x;
  float acc = 0.f;
  constexpr int V = mb_v<T>();
  if (P % V == 0 && n <= 32) {
    // a thread owns V consecutive positions and keeps the n samples' vectors in flight together
    for (int p = threadIdx.x * V; p < P; p += blockDim.x * V) {
      float mu[V], var[V];
#pragma unroll
      for (int j = 0; j < V; ++j) mu[j] = var[j] = 0.f;
      if (n <= MB_NMAX) {
        MbVec<T, V> xs[MB_NMAX];
        mb_load_samples<T, V>(x, n, P, p, xs);
#pragma unroll
        for (int i = 0; i < MB_NMAX; ++i)
          if (i < n) {
#pragma unroll
            for (int j = 0; j < V; ++j) mu[j] += xs[i].get(j);
          }
#pragma unroll
        for (int j = 0; j < V; ++j) mu[j] /= (float)n;
#pragma unroll
        for (int i = 0; i < MB_NMAX; ++i)
          if (i < n) {
#pragma unroll
            for (int j = 0; j < V; ++j) {
              const float d = xs[i].get(j) - mu[j];
              var[j] = fmaf(d, d, var[j]);
            }
          }
      } else {
        for (int i = 0; i < n; ++i) {
          const MbVec<T, V> xv = mb_ld<T, V>(x + (int64_t)i * P + p);
#pragma unroll
          for (int j = 0; j < V; ++j) mu[j] += xv.get(j);
        }
#pragma unroll
        for (int j = 0; j < V; ++j) mu[j] /= (float)n;
        for (int i = 0; i < n; ++i) {
          const MbVec<T, V> xv = mb_ld<T, V>(x + (int64_t)i * P + p);
#pragma unroll
          for (int j = 0; j < V; ++j) {
            const float d = xv.get(j) - mu[j];
            var[j] = fmaf(d, d, var[j]);
          }
        }
      }
#pragma unroll
      for (int j = 0; j < V; ++j) acc += sqrtf(var[j] / (float)n + eps);
    }
  } else {
    for (int p = threadIdx.x; p < P; p += blockDim.x) {
      float mu = 0.f;
      for (int i = 0; i < n; ++i) mu += ld(x + (int64_t)i * P + p);
      mu /= (float)n;
      float var = 0.f;
      for (int i = 0; i < n; ++i) {
        const float d = ld(x + (int64_t)i * P + p) - mu;
        var = fmaf(d, d, var);
      }
      acc += sqrtf(var / (float)n + eps);
    }
  }
  const float val = block_sum(acc, red) / (float)P;
  if (threadIdx.x == 0 && stat) stat[0] = val;
  const int64_t total = (int64_t)n * hw * cpad;
  constexpr int V16 = Vec16<T>::N;
  if (c % V16 == 0 && cpad % V16 == 0) {
    mb_copy_with_stat<T, 9>(x, out, total / V16, c, cpad, val);
  } else {
    for (int64_t i = threadIdx.x; i < total; i += blockDim.x) {
      const int ch = (int)(i % cpad);
      const int64_t px = i / cpad;
      float v = 0.f;
      if (ch < c)
        v = ld(x + px * c + ch);
      else if (ch == c)
        v = val;
      st(out + i, v);
    }
  }
}

// gx[n][p] = gout[n][hw][ch<c] + G * (x - mu_p) / (N * sigma_p * P),  G = sum over (n,hw) of gout[..., c]
// 256-thread workgroups, gridDim.y of them per statistic group, one 8-byte position vector per thread and trip (four
// workgroups cover the [16, 4, 4, 256] bf16 tensor; each sums G for itself).  History: the single 1024-thread workgroup
// with 16-byte vectors spilled 168-392 bytes per thread to scratch and took 24-52 us for 400 KB of traffic
// (profiles/r03_z_shapes_eager_step.json); two 256-thread workgroups with 16-byte vectors 256 VGPRs and 15 us.
// The first trip's loads are requested BEFORE the reduction of G, whose barrier they do not depend on.
template <typename T>
__global__ __launch_bounds__(256) void mbstd_bwd_kernel(const T* __restrict__ gout, const T* __restrict__ x,
                                                        T* __restrict__ gx, int n, int hw, int c, int cpad, float eps) {
  __shared__ float red[16];
  const int P = hw * c;
  gout += (int64_t)blockIdx.x * n * hw * cpad;
  x += (int64_t)blockIdx.x * n * P;
  gx += (int64_t)blockIdx.x * n * P;
  constexpr int V = mb_v<T>();
  const bool fast = c % V == 0 && cpad % V == 0 && n <= MB_NMAX;
  MbVec<T, V> xs[MB_NMAX], gs[MB_NMAX];
  const int pstep = gridDim.y * blockDim.x * V;
  const int pfirst = (blockIdx.y * blockDim.x + threadIdx.x) * V;
  if (fast) {      // dead threads (pfirst >= P) read position 0: harmless, never used
    const int p = pfirst < P ? pfirst : 0;
    const int px = p / c, ch = p - px * c;
    mb_load_samples<T, V>(x, n, P, p, xs);
#pragma unroll
    for (int i = 0; i < MB_NMAX; ++i) gs[i] = mb_ld<T, V>(gout + ((int64_t)(i < n ? i : n - 1) * hw + px) * cpad + ch);
  }
  float acc = 0.f;
  for (int i = threadIdx.x; i < n * hw; i += blockDim.x) acc += ld(gout + (int64_t)i * cpad + c);
  const float G = block_sum(acc, red);
  if (fast) {
    for (int p = pfirst; p < P; p += pstep) {
      float mu[V], var[V], k[V];
      if (p != pfirst) {
        const int px = p / c, ch = p - px * c;
        mb_load_samples<T, V>(x, n, P, p, xs);
#pragma unroll
        for (int i = 0; i < MB_NMAX; ++i) gs[i] = mb_ld<T, V>(gout + ((int64_t)(i < n ? i : n - 1) * hw + px) * cpad + ch);
      }
#pragma unroll
      for (int j = 0; j < V; ++j) mu[j] = var[j] = 0.f;
#pragma unroll
      for (int i = 0; i < MB_NMAX; ++i)
        if (i < n) {
#pragma unroll
          for (int j = 0; j < V; ++j) mu[j] += xs[i].get(j);
        }
#pragma unroll
      for (int j = 0; j < V; ++j) mu[j] /= (float)n;
#pragma unroll
      for (int i = 0; i < MB_NMAX; ++i)
        if (i < n) {
#pragma unroll
          for (int j = 0; j < V; ++j) {
            const float d = xs[i].get(j) - mu[j];
            var[j] = fmaf(d, d, var[j]);
          }
        }
#pragma unroll
      for (int j = 0; j < V; ++j) k[j] = G / ((float)n * sqrtf(var[j] / (float)n + eps) * (float)P);
#pragma unroll
      for (int i = 0; i < MB_NMAX; ++i)
        if (i < n) {
          MbVec<T, V> o;
#pragma unroll
          for (int j = 0; j < V; ++j) o.set(j, gs[i].get(j) + k[j] * (xs[i].get(j) - mu[j]));
          mb_st<T, V>(gx + (int64_t)i * P + p, o);
        }
    }
    return;
  }
  if (c % V == 0 && cpad % V == 0 && n <= 32) {
    for (int p = pfirst; p < P; p += pstep) {
      float mu[V], var[V], k[V];
#pragma unroll
      for (int j = 0; j < V; ++j) mu[j] = var[j] = 0.f;
      for (int i = 0; i < n; ++i) {
        const MbVec<T, V> xv = mb_ld<T, V>(x + (int64_t)i * P + p);
#pragma unroll
        for (int j = 0; j < V; ++j) mu[j] += xv.get(j);
      }
#pragma unroll
      for (int j = 0; j < V; ++j) mu[j] /= (float)n;
      for (int i = 0; i < n; ++i) {
        const MbVec<T, V> xv = mb_ld<T, V>(x + (int64_t)i * P + p);
#pragma unroll
        for (int j = 0; j < V; ++j) {
          const float d = xv.get(j) - mu[j];
          var[j] = fmaf(d, d, var[j]);
        }
      }
#pragma unroll
      for (int j = 0; j < V; ++j) k[j] = G / ((float)n * sqrtf(var[j] / (float)n + eps) * (float)P);
      const int px = p / c, ch = p - px * c;
      for (int i = 0; i < n; ++i) {
        const MbVec<T, V> xv = mb_ld<T, V>(x + (int64_t)i * P + p);
        const MbVec<T, V> gv = mb_ld<T, V>(gout + ((int64_t)i * hw + px) * cpad + ch);
        MbVec<T, V> o;
#pragma unroll
        for (int j = 0; j < V; ++j) o.set(j, gv.get(j) + k[j] * (xv.get(j) - mu[j]));
        mb_st<T, V>(gx + (int64_t)i * P + p, o);
      }
    }
    return;
  }
  for (int p = blockIdx.y * blockDim.x + threadIdx.x; p < P; p += gridDim.y * blockDim.x) {
    float mu = 0.f;
    for (int i = 0; i < n; ++i) mu += ld(x + (int64_t)i * P + p);
    mu /= (float)n;
    float var = 0.f;
    for (int i = 0; i < n; ++i) {
      const float d = ld(x + (int64_t)i * P + p) - mu;
      var = fmaf(d, d, var);
    }
    const float sigma = sqrtf(var / (float)n + eps);
    const float k = G / ((float)n * sigma * (float)P);
    const int px = p / c, ch = p - px * c;
    for (int i = 0; i < n; ++i) {
      const float d = ld(x + (int64_t)i * P + p) - mu;
      st(gx + (int64_t)i * P + p, ld(gout + ((int64_t)i * hw + px) * cpad + ch) + k * d);
    }
  }
}

// Double backward.  With c_n = x_n - mu, sigma = sqrt(mean c^2 + eps), gx_n = gpass_n + G c_n /(N sigma P):
//   d/dG      : T = sum_{n,p} v_np c_np / (N sigma_p P)  -> ggout[..., c] = T for every (n,hw); ggout[..., <c] = v
//   d/dx_mp   : (G/(N P)) * [ (v_m - mean_n v)/sigma - (sum_n v_n c_n) c_m / (N sigma^3) ]
// 1024 threads, 8-byte position vectors (one trip at [16, 4, 4, 256]), first trip's loads ahead of the reduction of G (see
// mbstd_bwd_kernel); the per-element divisions by sigma / sigma^3 are multiplications by per-POSITION reciprocals (two
// fp32 divisions per element were most of this kernel's instructions: 35 us for 400 KB)
template <typename T, int NTHR>      // NTHR: 1024 for the 16-bit types, 512 for fp32 (its 128-VGPR budget at 1024 spilled)
__global__ __launch_bounds__(NTHR) void mbstd_bwd_bwd_kernel(const T* __restrict__ v, const T* __restrict__ gout,
                                                            const T* __restrict__ x, T* __restrict__ ggout,
                                                            T* __restrict__ gx2, int n, int hw, int c, int cpad,
                                                            float eps) {
  __shared__ float red[16];
  const int P = hw * c;
  v += (int64_t)blockIdx.x * n * P;
  gout += (int64_t)blockIdx.x * n * hw * cpad;
  x += (int64_t)blockIdx.x * n * P;
  if (ggout) ggout += (int64_t)blockIdx.x * n * hw * cpad;
  if (gx2) gx2 += (int64_t)blockIdx.x * n * P;
  constexpr int V = mb_v<T>();
  const bool fast = P % V == 0 && n <= MB_NMAX;
  MbVec<T, V> xs[MB_NMAX], vs[MB_NMAX];
  const int pfirst = threadIdx.x * V;
  if (fast) {      // dead threads (pfirst >= P) read position 0: harmless, never used
    mb_load_samples<T, V>(x, n, P, pfirst < P ? pfirst : 0, xs);
    mb_load_samples<T, V>(v, n, P, pfirst < P ? pfirst : 0, vs);
  }
  float acc = 0.f;
  for (int i = threadIdx.x; i < n * hw; i += blockDim.x) acc += ld(gout + (int64_t)i * cpad + c);
  const float G = block_sum(acc, red);
  float tacc = 0.f;
  if (fast) {
    for (int p = pfirst; p < P; p += blockDim.x * V) {
      if (p != pfirst) {
        mb_load_samples<T, V>(x, n, P, p, xs);
        mb_load_samples<T, V>(v, n, P, p, vs);
      }
      float mu[V], vm[V], var[V], vc[V], sigma[V];
#pragma unroll
      for (int j = 0; j < V; ++j) mu[j] = vm[j] = var[j] = vc[j] = 0.f;
#pragma unroll
      for (int i = 0; i < MB_NMAX; ++i)
        if (i < n) {
#pragma unroll
          for (int j = 0; j < V; ++j) {
            mu[j] += xs[i].get(j);
            vm[j] += vs[i].get(j);
          }
        }
#pragma unroll
      for (int j = 0; j < V; ++j) {
        mu[j] /= (float)n;
        vm[j] /= (float)n;
      }
#pragma unroll
      for (int i = 0; i < MB_NMAX; ++i)
        if (i < n) {
#pragma unroll
          for (int j = 0; j < V; ++j) {
            const float d = xs[i].get(j) - mu[j];
            var[j] = fmaf(d, d, var[j]);
            vc[j] = fmaf(vs[i].get(j), d, vc[j]);
          }
        }
#pragma unroll
      for (int j = 0; j < V; ++j) {
        sigma[j] = sqrtf(var[j] / (float)n + eps);
        tacc += vc[j] / ((float)n * sigma[j] * (float)P);
      }
      if (gx2) {
        const float k = G / ((float)n * (float)P);
        float is[V], cf[V];      // 1 / sigma,  sum_n(v c) / (N sigma^3)
#pragma unroll
        for (int j = 0; j < V; ++j) {
          is[j] = 1.f / sigma[j];
          cf[j] = vc[j] * is[j] * is[j] * is[j] / (float)n;
        }
#pragma unroll
        for (int i = 0; i < MB_NMAX; ++i)
          if (i < n) {
            MbVec<T, V> o;
#pragma unroll
            for (int j = 0; j < V; ++j) {
              const float d = xs[i].get(j) - mu[j];
              o.set(j, k * ((vs[i].get(j) - vm[j]) * is[j] - cf[j] * d));
            }
            mb_st<T, V>(gx2 + (int64_t)i * P + p, o);
          }
      }
    }
  }
  for (int p = threadIdx.x; p < P && !fast; p += blockDim.x) {
    float mu = 0.f, vm = 0.f;
    for (int i = 0; i < n; ++i) {
      mu += ld(x + (int64_t)i * P + p);
      vm += ld(v + (int64_t)i * P + p);
    }
    mu /= (float)n;
    vm /= (float)n;
    float var = 0.f, vc = 0.f;
    for (int i = 0; i < n; ++i) {
      const float d = ld(x + (int64_t)i * P + p) - mu;
      var = fmaf(d, d, var);
      vc = fmaf(ld(v + (int64_t)i * P + p), d, vc);
    }
    const float sigma = sqrtf(var / (float)n + eps);
    tacc += vc / ((float)n * sigma * (float)P);
    if (gx2) {
      const float k = G / ((float)n * (float)P);
      for (int i = 0; i < n; ++i) {
        const float d = ld(x + (int64_t)i * P + p) - mu;
        const float vi = ld(v + (int64_t)i * P + p);
        st(gx2 + (int64_t)i * P + p, k * ((vi - vm) / sigma - vc * d / ((float)n * sigma * sigma * sigma)));
      }
    }
  }
  const float Tt = block_sum(tacc, red);
  if (ggout) {
    const int64_t total = (int64_t)n * hw * cpad;
    constexpr int V16 = Vec16<T>::N;
    if (c % V16 == 0 && cpad % V16 == 0) {
      mb_copy_with_stat<T, 9>(v, ggout, total / V16, c, cpad, Tt);
    } else {
      for (int64_t i = threadIdx.x; i < total; i += blockDim.x) {
        const int ch = (int)(i % cpad);
        const int64_t px = i / cpad;
        float o = 0.f;
        if (ch < c)
          o = ld(v + px * c + ch);
        else if (ch == c)
          o = Tt;
        st(ggout + i, o);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// reductions
// ------------------------------------------------------------------------------------------------
// MODE 0: sum(x)  1: sum|x-y|;  PART: out[blockIdx.x] = this workgroup's sum;  direct (a ONE-workgroup launch that does not
// accumulate): out[0] is written, not added to -- the launch needs no zero fill before it;  vec = 0: an operand does not
// start on a 16-byte boundary (a view into a larger buffer), every element takes the scalar loop
template <typename T, int MODE, bool PART = false>
__global__ void sum_kernel(const T* __restrict__ x, const T* __restrict__ y, float* __restrict__ out, int64_t numel,
                           float scale, int direct = 0, int vec = 1) {
  __shared__ float red[8];
  constexpr int V = Vec16<T>::N;
  const int64_t nvec = vec ? numel / V : 0, stride = (int64_t)gridDim.x * blockDim.x;
  float acc = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += stride) {
    Vec16<T> a = ldv(x + i * V);
    if (MODE == 0) {
#pragma unroll
      for (int j = 0; j < V; ++j) acc += a.get(j);
    } else {
      Vec16<T> b = ldv(y + i * V);
#pragma unroll
      for (int j = 0; j < V; ++j) acc += fabsf(a.get(j) - b.get(j));
    }
  }
  for (int64_t i = nvec * V + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < numel; i += stride)
    acc += MODE == 0 ? ld(x + i) : fabsf(ld(x + i) - ld(y + i));
  const float tot = block_sum(acc, red);
  if (threadIdx.x == 0) {
    if constexpr (PART) out[blockIdx.x] = tot;
    else if (direct) out[0] = tot * scale;
    else atomicAdd(out, tot * scale);
  }
}

// out[0] (+)= scale * (part[0] + part[1] + ... in index order)
__global__ void ordered_scalar_sum_kernel(const float* __restrict__ part, int n, float* __restrict__ out, float scale,
                                          int accumulate) {
  if (blockIdx.x || threadIdx.x) return;
  float t = 0.f;
  for (int i = 0; i < n; ++i) t += part[i];
  out[0] = accumulate ? out[0] + t * scale : t * scale;
}

// An fp32 value is +-inf or NaN exactly when its exponent bits are all ones.
__device__ __forceinline__ int nonfinite_bits(float x) {
  return (__builtin_bit_cast(uint32_t, x) & 0x7f800000u) == 0x7f800000u;
}
// The loss gradients' rule: a piecewise-constant derivative says nothing about a non-finite argument,
// and a 0 there would hide the overflow from tg_nonfinite_check -- the gradient of such an element is NaN, by selection.
__device__ __forceinline__ float nan_where_nonfinite(float grad, float arg) {
  return nonfinite_bits(arg) ? __builtin_nanf("") : grad;
}

template <typename T>
__global__ void abs_diff_bwd_kernel(const T* __restrict__ a, const T* __restrict__ b, const float* __restrict__ gscale,
                                    T* __restrict__ ga, T* __restrict__ gb, int64_t numel, float scale) {
  const float g = (gscale ? gscale[0] : 1.f) * scale;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < numel; i += (int64_t)gridDim.x * blockDim.x) {
    const float d = ld(a + i) - ld(b + i);
    const float s = nan_where_nonfinite(d > 0.f ? g : (d < 0.f ? -g : 0.f), d);
    if (ga) st(ga + i, s);
    if (gb) st(gb + i, -s);
  }
}

// out[b] = sum over sample b of x^2;  grid = (chunks, batch), out pre-zeroed;  vec = 0: x + b * per is not 16-byte aligned
// for every sample (per no multiple of the vector width, or x itself unaligned), every element takes the scalar loop
template <typename T>
__global__ void sample_sumsq_kernel(const T* __restrict__ x, float* __restrict__ out, int64_t per, int vec) {
  __shared__ float red[8];
  constexpr int V = Vec16<T>::N;
  const T* base = x + (int64_t)blockIdx.y * per;
  const int64_t nvec = vec ? per / V : 0, stride = (int64_t)gridDim.x * blockDim.x;
  float acc = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += stride) {
    Vec16<T> a = ldv(base + i * V);
#pragma unroll
    for (int j = 0; j < V; ++j) acc = fmaf(a.get(j), a.get(j), acc);
  }
  for (int64_t i = nvec * V + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < per; i += stride) {
    const float a = ld(base + i);
    acc = fmaf(a, a, acc);
  }
  const float tot = block_sum(acc, red);
  if (threadIdx.x == 0) atomicAdd(out + blockIdx.y, tot);
}

// image_generation.py:431-436
__global__ void gp_penalty_kernel(const float* __restrict__ ss, float* __restrict__ loss, float* __restrict__ coef,
                                  int batch, float lambda) {
  __shared__ float red[8];
  float acc = 0.f;
  for (int b = threadIdx.x; b < batch; b += blockDim.x) {
    const float slope = sqrtf(ss[b]);
    const float d = slope - 1.f;
    acc += d * d;
    // slope == 0: coef = 0, this project's choice; a NaN or infinite slope takes the formula and stays non-finite
    if (coef) coef[b] = slope == 0.f ? 0.f : lambda * 2.f * d / (slope * (float)batch);
  }
  const float tot = block_sum(acc, red);
  if (threadIdx.x == 0 && loss) loss[0] = lambda * tot / (float)batch;
}

// Prediction losses on the tiny fp32 [B,1] discriminator outputs (image_generation.py:331-400).
//   mode 0: x                      (WGAN means)
//   mode 1: relu(a + b*x)          (hinge: a = 1, b = +1 for fakes / -1 for reals)
//   mode 2: sigmoid cross entropy against label a in {0,1}: max(x,0) - x*a + log(1 + exp(-|x|))
//   mode 3: x^2                    (WGAN drift term)
__device__ __forceinline__ float pred_loss_f(float x, int mode, float a, float b) {
  if (mode == 1) {      // not fmaxf: a NaN stays a NaN (np.maximum's rule)
    const float z = a + b * x;
    return z < 0.f ? 0.f : z;
  }
  if (mode == 2) return fmaxf(x, 0.f) - x * a + log1pf(expf(-fabsf(x)));
  if (mode == 3) return x * x;
  return x;
}
__device__ __forceinline__ float pred_loss_df_finite(float x, int mode, float a, float b) {
  if (mode == 1) return (a + b * x) > 0.f ? b : 0.f;
  if (mode == 2) return 1.f / (1.f + expf(-x)) - a;       // sigmoid(x) - label
  if (mode == 3) return 2.f * x;
  return 1.f;
}
__device__ __forceinline__ float pred_loss_df(float x, int mode, float a, float b) {
  return nan_where_nonfinite(pred_loss_df_finite(x, mode, a, b), x);
}
__global__ void pred_loss_fwd_kernel(const float* __restrict__ x, float* __restrict__ out, int n, int mode, float a,
                                     float b, float scale, int accumulate) {
  __shared__ float red[8];
  float acc = 0.f;
  for (int i = threadIdx.x; i < n; i += blockDim.x) acc += pred_loss_f(x[i], mode, a, b);
  const float tot = block_sum(acc, red);
  if (threadIdx.x == 0) out[0] = (accumulate ? out[0] : 0.f) + scale * tot;
}
__global__ void pred_loss_bwd_kernel(const float* __restrict__ x, const float* __restrict__ gscale, float* __restrict__ gx,
                                     int n, int mode, float a, float b, float scale) {
  const float g = (gscale ? gscale[0] : 1.f) * scale;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    gx[i] = g * pred_loss_df(x[i], mode, a, b);
}

// ---- the loss tail of one batched discriminator call in ONE launch each way (image_generation.py:331-400).  pred holds
// `groups` predictions of group_size rows ([real; cyc; prime] ...); job j adds coef * mean_i f_mode(x_i; a, b) over group
// `group` to term `term`.  Jobs and gradient pointers travel by value in the kernel arguments (a hipGraph records them).
constexpr int PRED_MAX_JOBS = 12, PRED_MAX_TERMS = 8;
struct PredJobs {
  TgPredJob j[PRED_MAX_JOBS];
  int n;
};
struct PredGrads {
  const float* g[PRED_MAX_TERMS];      // d loss / d term t: a device fp32 scalar each (NULL: that term has no gradient)
};
__global__ __launch_bounds__(256) void pred_losses_fwd_kernel(const float* __restrict__ x, int gs, PredJobs jobs, float* __restrict__ terms,
                                                              int nterms) {
  __shared__ float red[8];
  __shared__ float acc_t[PRED_MAX_TERMS];
  if (threadIdx.x < PRED_MAX_TERMS) acc_t[threadIdx.x] = 0.f;
  __syncthreads();
  for (int j = 0; j < jobs.n; ++j) {      // in job order: a fixed summation order
    const TgPredJob J = jobs.j[j];
    float acc = 0.f;
    for (int i = threadIdx.x; i < gs; i += blockDim.x) acc += pred_loss_f(x[J.group * gs + i], J.mode, J.a, J.b);
    const float tot = block_sum(acc, red);
    if (threadIdx.x == 0) acc_t[J.term] += J.coef * tot / (float)gs;
    __syncthreads();
  }
  if (threadIdx.x < nterms) terms[threadIdx.x] = acc_t[threadIdx.x];
}
__global__ void pred_losses_bwd_kernel(const float* __restrict__ x, int gs, int groups, PredJobs jobs, PredGrads gr,
                                       float* __restrict__ gx) {
  const int n = gs * groups;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int grp = i / gs;
    const float xi = x[i];
    float g = 0.f;
    for (int j = 0; j < jobs.n; ++j) {
      const TgPredJob J = jobs.j[j];
      if (J.group == grp && gr.g[J.term]) g += gr.g[J.term][0] * (J.coef / (float)gs) * pred_loss_df(xi, J.mode, J.a, J.b);
    }
    gx[i] = g;
  }
}
// out[0] = sum_i x_i[0] over up to 24 device fp32 scalars (tf.add_n over the loss collection), in argument order
struct ScalarPtrs {
  const float* p[24];
  int n;
};
__global__ void sum_scalars_kernel(ScalarPtrs a, float* __restrict__ out) {
  if (blockIdx.x || threadIdx.x) return;
  float t = 0.f;
  for (int i = 0; i < a.n; ++i) t += a.p[i][0];
  out[0] = t;
}

// out[0] = E[x^2] - E[x]^2 from sum = s1[0] and the per-sample sums of squares ss[batch]  (DRAGAN,
// image_generation.py:445: the VARIANCE over every element of the minibatch)
// tf.losses.cosine_distance(l2n(expected), l2n(embedding), axis=-1, weights=w) (twingan.py:515-519):
//   out = (w / B) * sum_b (1 - e_b . p_b / (|e_b| |p_b|)),  norms clamped as tf.nn.l2_normalize does (sum x^2 >= 1e-12).
// One workgroup walks the rows in order: a handful of [B, D] rows, fixed summation order.
__global__ __launch_bounds__(256) void cosine_distance_fwd_kernel(const float* __restrict__ e, const float* __restrict__ p,
                                                                  float* __restrict__ out, int b, int d, float scale) {
  __shared__ float red[4];
  float tot = 0.f;
  for (int r = 0; r < b; ++r) {
    float dot = 0.f, se = 0.f, sp = 0.f;
    for (int c = threadIdx.x; c < d; c += 256) {
      const float x = e[(size_t)r * d + c], y = p[(size_t)r * d + c];
      dot = fmaf(x, y, dot);
      se = fmaf(x, x, se);
      sp = fmaf(y, y, sp);
    }
    dot = block_sum(dot, red);
    se = block_sum(se, red);
    sp = block_sum(sp, red);
    tot += 1.f - dot * rsqrtf(fmaxf(se, 1e-12f)) * rsqrtf(fmaxf(sp, 1e-12f));
  }
  if (threadIdx.x == 0) out[0] = tot * scale;
}

// d out / d p[b, c] = -(w / B) * g * (ehat_c - phat_c (ehat . phat)) / |p|   (|p|^2 >= 1e-12; below it phat = p * 1e6)
__global__ __launch_bounds__(256) void cosine_distance_bwd_kernel(const float* __restrict__ e, const float* __restrict__ p,
                                                                  const float* __restrict__ gscale, float* __restrict__ gp,
                                                                  int d, float scale) {
  __shared__ float red[4];
  const int r = blockIdx.x;
  float dot = 0.f, se = 0.f, sp = 0.f;
  for (int c = threadIdx.x; c < d; c += 256) {
    const float x = e[(size_t)r * d + c], y = p[(size_t)r * d + c];
    dot = fmaf(x, y, dot);
    se = fmaf(x, x, se);
    sp = fmaf(y, y, sp);
  }
  dot = block_sum(dot, red);
  se = block_sum(se, red);
  sp = block_sum(sp, red);
  const float ie = rsqrtf(fmaxf(se, 1e-12f)), ip = rsqrtf(fmaxf(sp, 1e-12f));
  const float cosv = dot * ie * ip, k = -scale * gscale[0];
  const bool clamped = sp < 1e-12f;
  for (int c = threadIdx.x; c < d; c += 256) {
    const float eh = e[(size_t)r * d + c] * ie, ph = p[(size_t)r * d + c] * ip;
    gp[(size_t)r * d + c] = k * (clamped ? eh * ip : (eh - ph * cosv) * ip);
  }
}

__global__ void var_from_sums_kernel(const float* __restrict__ s1, const float* __restrict__ ss, float* __restrict__ out,
                                     int batch, float inv_numel) {
  __shared__ float red[8];
  float acc = 0.f;
  for (int i = threadIdx.x; i < batch; i += blockDim.x) acc += ss[i];
  const float tot = block_sum(acc, red);
  if (threadIdx.x == 0) {
    const float m = s1[0] * inv_numel;
    const float v = tot * inv_numel - m * m;
    out[0] = v < 0.f ? 0.f : v;      // not fmaxf: a NaN stays a NaN
  }
}

// ---- the fully connected layer of a network's tail (layers.fully_connected, nets/pggan_utils.py:323-327) as ONE launch each
// way: y[B,N] = x[B,K] @ w[K,N] + b[N] with x in the activations' storage type (the cast, the GEMM and the bias add were
// three launches), and gx = g @ w^T (in x's type), gw (+)= x^T @ g, gb (+)= sum_b g (four launches).  B <= 64-ish rows,
// K = 256, N = 1 (the discriminators' prediction) .. 16: one WAVE per output element forward (lanes split K), one THREAD
// per k backward (it owns row k of gw and column k of gx).
template <typename T>
__global__ void fc_fwd_kernel(const T* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b,
                              float* __restrict__ y, int m, int n, int k) {
  const int64_t total = (int64_t)m * n;
  const int lane = threadIdx.x & 63;
  const int64_t w0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t i = w0; i < total; i += nw) {
    const int col = (int)(i % n), row = (int)(i / n);
    float acc = 0.f;
    for (int kk = lane; kk < k; kk += 64) acc = fmaf(ld(x + (int64_t)row * k + kk), w[(int64_t)kk * n + col], acc);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (lane == 0) y[i] = acc + (b ? b[col] : 0.f);
  }
}
template <typename T>
__global__ void fc_bwd_kernel(const T* __restrict__ x, const float* __restrict__ w, const float* __restrict__ g,
                              T* __restrict__ gx, float* __restrict__ gw, float* __restrict__ gb, int m, int n, int k,
                              int acc_w, int acc_b) {
  const int kk = blockIdx.x * blockDim.x + threadIdx.x;
  if (kk < k) {
    for (int row = 0; gx && row < m; ++row) {      // gx[row, kk] = sum_col g[row, col] * w[kk, col]
      float a = 0.f;
      for (int col = 0; col < n; ++col) a = fmaf(g[(int64_t)row * n + col], w[(int64_t)kk * n + col], a);
      st(gx + (int64_t)row * k + kk, a);
    }
    for (int col = 0; gw && col < n; ++col) {      // gw[kk, col] (+)= sum_row x[row, kk] * g[row, col], rows in order
      float a = 0.f;
      for (int row = 0; row < m; ++row) a = fmaf(ld(x + (int64_t)row * k + kk), g[(int64_t)row * n + col], a);
      gw[(int64_t)kk * n + col] = (acc_w ? gw[(int64_t)kk * n + col] : 0.f) + a;
    }
  }
  if (gb && kk < n) {                              // gb[col] (+)= sum_row g[row, col]
    float a = 0.f;
    for (int row = 0; row < m; ++row) a += g[(int64_t)row * n + kk];
    gb[kk] = (acc_b ? gb[kk] : 0.f) + a;
  }
}

// C[m,n] (+)= op(A)[m,k] @ op(B)[k,n] + bias[n]; one thread per output element
__global__ void small_gemm_kernel(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ bias,
                                  float* __restrict__ c, int m, int n, int k, int ta, int tb, int accumulate) {
  const int64_t total = (int64_t)m * n;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int col = (int)(i % n), row = (int)(i / n);
    float acc = 0.f;
    for (int kk = 0; kk < k; ++kk) {
      const float av = ta ? a[(int64_t)kk * m + row] : a[(int64_t)row * k + kk];
      const float bv = tb ? b[(int64_t)col * k + kk] : b[(int64_t)kk * n + col];
      acc = fmaf(av, bv, acc);
    }
    if (bias) acc += bias[col];
    c[i] = (accumulate ? c[i] : 0.f) + acc;
  }
}

// Same GEMM with one WAVE per output element (lanes split K, butterfly sum): the discriminator's fully connected
// layer is [B,256] x [256,1] -- a thread per output walks K = 256 as one dependent chain (18 us).
__global__ void small_gemm_wave_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                       const float* __restrict__ bias, float* __restrict__ c, int m, int n, int k, int ta,
                                       int tb, int accumulate) {
  const int64_t total = (int64_t)m * n;
  const int lane = threadIdx.x & 63;
  const int64_t w0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t i = w0; i < total; i += nw) {
    const int col = (int)(i % n), row = (int)(i / n);
    float acc = 0.f;
    for (int kk = lane; kk < k; kk += 64) {
      const float av = ta ? a[(int64_t)kk * m + row] : a[(int64_t)row * k + kk];
      const float bv = tb ? b[(int64_t)col * k + kk] : b[(int64_t)kk * n + col];
      acc = fmaf(av, bv, acc);
    }
    acc = wave_sum(acc);
    if (lane == 0) {
      if (bias) acc += bias[col];
      c[i] = (accumulate ? c[i] : 0.f) + acc;
    }
  }
}

// TF-1.x Adam (model/model_inheritor.py:537-542): epsilon OUTSIDE the bias-corrected sqrt.  One element, shared by
// both loops of apply_kernel so that every instantiation writes the same bits: the two multiply-adds are spelled as the fused
// operations the compiler's contraction made of `b1 * m + (1 - b1) * g` and `b2 * v + (1 - b2) * g * g`, so their
// rounding does not depend on the loop they are inlined into.  gi = g * gscale, formed by the caller.
__device__ __forceinline__ float adam_element(float th, float gi, float& m, float& v, float lr_t, float b1, float b2, float eps) {
  const float mi = fmaf(b1, m, (1.f - b1) * gi);
  const float vi = fmaf(b2, v, (1.f - b2) * gi * gi);
  m = mi;
  v = vi;
  return th - lr_t * mi / (sqrtf(vi) + eps);
}

// tf.train.ExponentialMovingAverage's assign_moving_average (TF 1.8 moving_averages.py): avg -= (avg - var) * (1 - decay),
// the product and the subtraction as one fused multiply-add.  avg == var gives avg back bit for bit.
__device__ __forceinline__ float ema_element(float avg, float var, float w) { return fmaf(-(avg - var), w, avg); }

// The moving average alone over a flat buffer, thread tid's share of nthr: 12 bytes per element.  VEC: both pointers are
// 16-byte aligned -- one 16-byte access per lane and array; the numel % 4 elements behind the last whole vector are taken one
// by one.  Otherwise (any 4-byte-aligned pointers) element by element.  The kernel hands tid and nthr in: read in here, the
// workgroup size costs a vector load and 4 VGPRs.
template <bool VEC>
__device__ __forceinline__ void ema_span(float* __restrict__ avg, const float* __restrict__ var, int64_t numel, float w,
                                         int64_t tid, int64_t nthr) {
  int64_t done = 0;
  if constexpr (VEC) {
    const int64_t nvec = numel >> 2;
    for (int64_t i = tid; i < nvec; i += nthr) {
      Vec16<float> a4 = ldv(avg + 4 * i);
      const Vec16<float> x4 = ldv(var + 4 * i);
#pragma unroll
      for (int e = 0; e < 4; ++e) a4.v[e] = ema_element(a4.v[e], x4.v[e], w);
      stv(avg + 4 * i, a4);
    }
    done = nvec << 2;
  }
  for (int64_t i = done + tid; i < numel; i += nthr) avg[i] = ema_element(avg[i], var[i], w);
}

// The group a run did not apply.  Its own kernel, not an instantiation of apply_kernel: 18 VGPRs against 51.
template <bool VEC>
__global__ __launch_bounds__(256) void ema_kernel(float* __restrict__ avg, const float* __restrict__ var, int64_t numel,
                                                  const float* __restrict__ w_dev) {
  ema_span<VEC>(avg, var, numel, w_dev[0], (int64_t)blockIdx.x * blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x);
}

// ---- the reference's other --optimizer rules (include/twingan_hip_optim.h; TF 1.8 core/kernels/training_ops.cc, the dense
// functors).  One element each, in adam_element's style: g arrives unscaled-by-the-loss (g * gscale), every multiply that
// feeds an add is an explicit fmaf, so the 16-byte loop and the tail loop of apply_kernel write the same bits, and so do the
// fused and the unfused form; contraction is off inside them, so that the caller's g * gscale is not pulled into one of
// their plain adds in one instantiation and left alone in another.  a, b: the rule's slots in slot0, slot1 order; a rule
// touches only those it has.
__device__ __forceinline__ float sgd_element(float th, float g, const TgOptimHyper& h) { return fmaf(-h.lr, g, th); }

// ApplyMomentum, use_nesterov = false: accum = accum * momentum + grad; var -= lr * accum
__device__ __forceinline__ float momentum_element(float th, float g, float& a, const TgOptimHyper& h) {
#pragma clang fp contract(off)
  a = fmaf(h.momentum, a, g);
  return fmaf(-h.lr, a, th);
}

// ApplyAdagrad (TF 1.8: no epsilon): accum += grad^2; var -= lr * grad / sqrt(accum)
__device__ __forceinline__ float adagrad_element(float th, float g, float& a, const TgOptimHyper& h) {
#pragma clang fp contract(off)
  a = fmaf(g, g, a);
  return th - h.lr * g / sqrtf(a);
}

// ApplyRMSProp (not centred; epsilon inside the root): ms += (grad^2 - ms) * (1 - rho); mom = mom * momentum + lr * grad /
// sqrt(ms + eps); var -= mom
__device__ __forceinline__ float rmsprop_element(float th, float g, float& ms, float& mom, const TgOptimHyper& h) {
#pragma clang fp contract(off)
  ms = fmaf(fmaf(g, g, -ms), 1.f - h.decay_or_rho, ms);
  mom = fmaf(h.momentum, mom, h.lr * g / sqrtf(ms + h.eps));
  return th - mom;
}

// ApplyAdadelta: accum = rho accum + (1 - rho) grad^2; update = sqrt(accum_update + eps) / sqrt(accum + eps) * grad;
// var -= lr * update; accum_update = rho accum_update + (1 - rho) update^2
__device__ __forceinline__ float adadelta_element(float th, float g, float& accum, float& upd, const TgOptimHyper& h) {
#pragma clang fp contract(off)
  const float rho = h.decay_or_rho, omr = 1.f - rho;
  accum = fmaf(rho, accum, omr * g * g);
  const float u = sqrtf(upd + h.eps) / sqrtf(accum + h.eps) * g;
  upd = fmaf(rho, upd, omr * u * u);
  return fmaf(-h.lr, u, th);
}

// ApplyFtrl (no l2 shrinkage).  x^(-lr_power): the square root at the default -0.5, powf otherwise (lr_power <= 0; 0 gives 1).
// |linear| <= l1 -- linear == 0 with l1 == 0 included -- writes 0: TF's rule.
template <bool SQRT>
__device__ __forceinline__ float ftrl_element(float th, float g, float& accum, float& linear, const TgOptimHyper& h) {
#pragma clang fp contract(off)
  const float n = fmaf(g, g, accum);
  const float pn = SQRT ? sqrtf(n) : powf(n, -h.lr_power), pa = SQRT ? sqrtf(accum) : powf(accum, -h.lr_power);
  const float sigma = (pn - pa) / h.lr;
  const float lin = fmaf(-sigma, th, linear + g);
  const float q = fmaf(2.f, h.l2, pn / h.lr);
  accum = n;
  linear = lin;
  return fabsf(lin) > h.l1 ? (copysignf(h.l1, lin) - lin) / q : 0.f;
}

constexpr int TG_OPT_FTRL_POW = TG_OPT_FTRL + 1;      // kernel-side only: ftrl with lr_power != -0.5
constexpr int TG_OPT_ADAM = TG_OPT_FTRL + 2;          // kernel-side only: Adam has its own entry points (tg_adam_*)
constexpr int optim_slots(int rule) {
  return rule == TG_OPT_SGD ? 0 : (rule == TG_OPT_MOMENTUM || rule == TG_OPT_ADAGRAD) ? 1 : 2;
}

// a, b: the rule's slots.  Adam: h.lr is the bias-corrected rate, its betas ride in h.momentum and h.decay_or_rho.
template <int RULE>
__device__ __forceinline__ float apply_element(float th, float g, float& a, float& b, const TgOptimHyper& h) {
  if constexpr (RULE == TG_OPT_SGD) return sgd_element(th, g, h);
  else if constexpr (RULE == TG_OPT_MOMENTUM) return momentum_element(th, g, a, h);
  else if constexpr (RULE == TG_OPT_ADAGRAD) return adagrad_element(th, g, a, h);
  else if constexpr (RULE == TG_OPT_RMSPROP) return rmsprop_element(th, g, a, b, h);
  else if constexpr (RULE == TG_OPT_ADADELTA) return adadelta_element(th, g, a, b, h);
  else if constexpr (RULE == TG_OPT_ADAM) return adam_element(th, g, a, b, h.lr, h.momentum, h.decay_or_rho, h.eps);
  else return ftrl_element<RULE == TG_OPT_FTRL>(th, g, a, b, h);
}

// What every optimiser entry point (tg_adam_step, tg_adam_ema_step, their _guarded forms, tg_optim_step) hands to
// apply_kernel: what all of them have, then what only some have.
struct ApplyArgs {
  float* th;
  const float* g;
  float *s0, *s1;                            // null where the rule has no such slot: never dereferenced then.  Adam: m, v
  int64_t numel;
  TgOptimHyper h;                            // Adam: {lr_t, beta1, beta2, eps}, see apply_element
  float gscale = 0.f;                        // multiplies g first, without ls
  const TgLossScaleState* ls = nullptr;      // the guard: the gradient scale is its inv_scale, its skip decides
  float* avg = nullptr;                      // the fused moving average (EMA instantiations)
  const float* w_dev = nullptr;
  const float* lr_t_dev = nullptr;           // Adam alone: the rate on the device; null: h.lr
  bf16* shadow = nullptr;                    // Adam alone: tg_adam_step's rounded copy of theta (the instantiation without EMA)
};

// The apply of one group's flat buffers under RULE: 12 (sgd), 20 (momentum, adagrad) or 28 bytes per element (read theta, g
// and the slots; write theta and the slots).  EMA: the moving average of the parameters it just wrote in the same pass, 8
// bytes per element more against 12 for the apply followed by ema_kernel.  VEC as for ema_span, over every pointer in use.
// ls (dynamic loss scaling, below): the gradient scale is the state's inv_scale, and a skipped apply stores nothing -- but
// for the average, which is then ema_span over the unchanged theta (12 bytes per element): every run updates every average.
template <int RULE, bool VEC, bool EMA>
__global__ __launch_bounds__(256) void apply_kernel(const ApplyArgs a) {
  static_assert(RULE != TG_OPT_ADAM || EMA || !VEC, "plain Adam stores its bf16 shadow in the element loop: it has no 16-byte one");
  constexpr int NS = optim_slots(RULE);
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nthr = (int64_t)gridDim.x * blockDim.x;
  if (a.ls && a.ls->skip) {
    if constexpr (EMA) ema_span<VEC>(a.avg, a.th, a.numel, a.w_dev[0], tid, nthr);
    return;
  }
  const float gscale = a.ls ? a.ls->inv_scale : a.gscale;
  TgOptimHyper h = a.h;
  if constexpr (RULE == TG_OPT_ADAM) {
    if (a.lr_t_dev) h.lr = a.lr_t_dev[0];
  }
  float w = 0.f;
  if constexpr (EMA) w = a.w_dev[0];
  int64_t done = 0;
  if constexpr (VEC) {
    const int64_t nvec = a.numel >> 2;
    for (int64_t i = tid; i < nvec; i += nthr) {
      Vec16<float> t4 = ldv(a.th + 4 * i), p4 = {}, q4 = {}, a4 = {};
      const Vec16<float> g4 = ldv(a.g + 4 * i);
      if constexpr (NS >= 1) p4 = ldv(a.s0 + 4 * i);
      if constexpr (NS >= 2) q4 = ldv(a.s1 + 4 * i);
      if constexpr (EMA) a4 = ldv(a.avg + 4 * i);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float pi = p4.v[e], qi = q4.v[e];
        const float t = apply_element<RULE>(t4.v[e], g4.v[e] * gscale, pi, qi, h);
        p4.v[e] = pi;
        q4.v[e] = qi;
        t4.v[e] = t;
        if constexpr (EMA) a4.v[e] = ema_element(a4.v[e], t, w);
      }
      if constexpr (NS >= 1) stv(a.s0 + 4 * i, p4);
      if constexpr (NS >= 2) stv(a.s1 + 4 * i, q4);
      stv(a.th + 4 * i, t4);
      if constexpr (EMA) stv(a.avg + 4 * i, a4);
    }
    done = nvec << 2;
  }
  for (int64_t i = done + tid; i < a.numel; i += nthr) {
    float pi = 0.f, qi = 0.f, ai = 0.f;
    if constexpr (NS >= 1) pi = a.s0[i];
    if constexpr (NS >= 2) qi = a.s1[i];
    if constexpr (EMA) ai = a.avg[i];      // with the other loads: behind a store it would wait for the whole update
    const float t = apply_element<RULE>(a.th[i], a.g[i] * gscale, pi, qi, h);
    if constexpr (NS >= 1) a.s0[i] = pi;
    if constexpr (NS >= 2) a.s1[i] = qi;
    a.th[i] = t;
    if constexpr (EMA) a.avg[i] = ema_element(ai, t, w);
    else if constexpr (RULE == TG_OPT_ADAM) {
      if (a.shadow) a.shadow[i] = (bf16)t;
    }
  }
}

// ---- the moving averages of MANY small tensors in one launch (the non-trainable state: a few hundred separately allocated
// tensors of 1 to a few hundred elements).  A host-built job table as for pack_weights_multi (conv_mfma.hip).
struct EmaJob {
  float* avg;
  const float* var;
  int64_t numel;
  int block_begin, block_end;      // this job's slice of the grid (EMA_EPB elements per block)
};
constexpr int EMA_EPB = 1024;

__global__ __launch_bounds__(256) void ema_multi_kernel(const EmaJob* __restrict__ jobs, int njobs,
                                                        const float* __restrict__ w_dev) {
  // binary search: the job whose [block_begin, block_end) holds this block (uniform -> scalar loads)
  int lo = 0, hi = njobs - 1;
  const int b = blockIdx.x;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (b >= jobs[mid].block_end) lo = mid + 1;
    else hi = mid;
  }
  const EmaJob j = jobs[lo];
  if (b < j.block_begin || b >= j.block_end) return;      // a grid larger than the table's total: nothing to do
  const float w = w_dev[0];
  const int64_t i0 = (int64_t)(b - j.block_begin) * EMA_EPB;
#pragma unroll
  for (int e = threadIdx.x; e < EMA_EPB; e += 256) {
    const int64_t i = i0 + e;
    if (i < j.numel) j.avg[i] = ema_element(j.avg[i], j.var[i], w);
  }
}

// t = ++step; lr_t = lr * sqrt(1 - b2^t) / (1 - b1^t)   (tf.train.AdamOptimizer._prepare/_apply_dense).  One thread calls it.
__device__ __forceinline__ void adam_tick(int64_t* step, float* lr_t, float lr, float b1, float b2) {
  const int64_t t = step[0] + 1;
  step[0] = t;
  lr_t[0] = (float)((double)lr * sqrt(1.0 - pow((double)b2, (double)t)) / (1.0 - pow((double)b1, (double)t)));
}

__global__ void adam_tick_kernel(int64_t* step, float* lr_t, float lr, float b1, float b2) {
  if (threadIdx.x == 0 && blockIdx.x == 0) adam_tick(step, lr_t, lr, b1, b2);
}

// ---- dynamic loss scaling (Config.dynamic_loss_scale; this project's own rule): the scale, the skip
// decision and their bookkeeping live in a TgLossScaleState on the device, so a captured apply graph replays the decision.
// (nonfinite_bits: above, with the loss gradients that share it)

// found |= any x[i] non-finite, i < numel: 4 bytes per element.  VEC (x 16-byte aligned): TG_NF_U 16-byte loads per lane in
// flight per trip, the numel % 4 elements behind the last whole vector one by one; otherwise element by element.  A wave that
// saw one stores 1 through its first lane -- every writer writes the same value, so the stores need no atomic and no order --
// and nobody ever stores 0: several ranges may be checked before one tick.
constexpr int TG_NF_U = 2, TG_NF_CAP = 2048;      // 16-byte loads in flight per lane and trip; the grid's workgroup cap
template <bool VEC>
__global__ __launch_bounds__(256) void nonfinite_kernel(const float* __restrict__ x, int64_t numel,
                                                        TgLossScaleState* __restrict__ ls) {
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nthr = (int64_t)gridDim.x * blockDim.x;
  int bad = 0;
  int64_t done = 0;
  if constexpr (VEC) {
    const int64_t nvec = numel >> 2;
    for (int64_t i = tid; i < nvec; i += TG_NF_U * nthr) {
      Vec16<float> a[TG_NF_U];
#pragma unroll
      for (int u = 0; u < TG_NF_U; ++u) {
        const int64_t j = i + u * nthr;
        a[u] = ldv(x + 4 * (j < nvec ? j : i));
      }
#pragma unroll
      for (int u = 0; u < TG_NF_U; ++u)
#pragma unroll
        for (int e = 0; e < 4; ++e) bad |= nonfinite_bits(a[u].v[e]);
    }
    done = nvec << 2;
  }
  for (int64_t i = done + tid; i < numel; i += nthr) bad |= nonfinite_bits(x[i]);
  if (__any(bad) && (threadIdx.x & 63) == 0) ls->found = 1;
}

// One thread, once per apply of a group.  S = the scale the backward just used; the apply in flight unscales with 1 / S
// (exact: S is a power of two), the group's next backward is seeded with the new S / world.  found: the apply is skipped,
// S <- max(S / 2, 1), the shared Adam step and rate stay; otherwise adam_tick_kernel's step and, after `interval` good applies
// in a row, S <- min(2 S, max_scale).
__global__ void loss_scale_tick_kernel(TgLossScaleState* ls, int64_t* step, float* lr_t, float lr, float b1, float b2,
                                       int interval, float max_scale, int world) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const float S = ls->scale;
  const int found = ls->found != 0;
  float next = S;
  if (found) {
    next = fmaxf(S * 0.5f, 1.f);
    ls->good_steps = 0;
    ls->skipped += 1;
  } else {
    adam_tick(step, lr_t, lr, b1, b2);
    const int good = ls->good_steps + 1;
    if (good >= interval) next = fminf(2.f * S, max_scale);
    ls->good_steps = good >= interval ? 0 : good;
  }
  ls->inv_scale = 1.f / S;
  ls->skip = found;
  ls->found = 0;
  ls->scale = next;
  ls->seed = (float)((double)next / (double)world);
}

// The one launch of apply_kernel, `name` the entry point's.  The 16-byte loop is taken when every pointer in use (theta, grad,
// the rule's slots, the average when there is one) is 16-byte aligned, else the apply goes element by element.  avg and
// shadow exclude each other: the EMA instantiations store no shadow, and no entry point has both.
template <int RULE>
int launch_apply(const ApplyArgs& a, void* stream, const char* name) {
  constexpr int NS = optim_slots(RULE);
  // plain Adam (no average) has no 16-byte instantiation: its bf16 shadow is stored in the element loop
  constexpr bool PLAIN_VEC = RULE != TG_OPT_ADAM;
  const bool ema = a.avg != nullptr;
  const bool vec = (ema || PLAIN_VEC) && tg_aligned16(a.th) && tg_aligned16(a.g) && (NS < 1 || tg_aligned16(a.s0)) &&
                   (NS < 2 || tg_aligned16(a.s1)) && (!ema || tg_aligned16(a.avg));
  auto kernel = ema ? (vec ? apply_kernel<RULE, true, true> : apply_kernel<RULE, false, true>)
                    : (vec ? apply_kernel<RULE, PLAIN_VEC, false> : apply_kernel<RULE, false, false>);
  hipLaunchKernelGGL(kernel, dim3(tg_grid_for(vec ? (a.numel + 3) / 4 : a.numel, 256)), dim3(256), 0, (hipStream_t)stream, a);
  TG_LAUNCH_CHECK(name);
  return TG_OK;
}

// ---- training summaries (include/twingan_hip_summary.h): statistics and TensorFlow histogram of a table of tensors -----------
// One workgroup summarises SUM_EPB consecutive logical elements of one job (the job found as in ema_multi_kernel): every
// thread keeps its counts, minimum, maximum and the two double sums in registers, the workgroup reduces them in a fixed
// order (xor tree in the wave, wave 0..3 in turn) and stores ONE partial; summary_finish_kernel adds a job's partials in
// block order.  The histogram is a per-workgroup LDS array of TG_SUMMARY_BUCKETS counters beside the 774 float limits;
// its non-zero bins go to the result with one integer atomic each (integer adds commute: the result has no order).
struct SummaryJob {
  const void* base;
  int64_t row_stride;
  uint32_t rows, row_valid, numel;      // numel = rows * row_valid < 2^32
  int dtype, out;
  int block_begin, block_end;
};
struct SummaryPartial {
  double sum, sumsq;
  float mn, mx;
  uint32_t num, zeros, nonfinite, pad;
};
static_assert(sizeof(SummaryPartial) == sizeof(TgSummaryStats), "a partial is a result over one workgroup's elements");
constexpr int SUM_EPB = 16384, SUM_THREADS = 256, SUM_U = 4;
constexpr int SUM_NL = TG_SUMMARY_POS_LIMITS;
constexpr float SUM_FLT_MAX = 3.402823466e+38f;

// Bucket of a finite v: c = #{k: L[k] <= |v|} counted on the rounded-up float limits (exact for L[k] <= a, and for L[k] < a
// too because no L[k] is a float itself: tg_summary_limits checks), then 776 + c for v >= 0 (both zeros: 776) and 775 - c for
// v < 0.  The logarithm only guesses; the two loops make c exact against the table whatever the guess was.
__device__ __forceinline__ int summary_bucket(float v, const float* lim) {
  const float a = fabsf(v);
  // k ~ log(a / 1e-12) / log(1.1) = (log2 a + 39.8631) * 7.27254
  const float g = (log2f(a) + 39.863137f) * 7.2725409f;
  int c = g > 0.f ? (g < (float)SUM_NL ? (int)g : SUM_NL) : 0;      // NaN-free: a is finite; a = 0 gives -inf -> 0
  while (c < SUM_NL && lim[c] <= a) ++c;
  while (c > 0 && lim[c - 1] > a) --c;
  return v < 0.f ? SUM_NL + 1 - c : SUM_NL + 2 + c;
}

struct SummaryAcc {
  double sum = 0.0, sumsq = 0.0;
  float mn = SUM_FLT_MAX, mx = -SUM_FLT_MAX;
  uint32_t num = 0, zeros = 0, nonfinite = 0;
};

template <typename T>
__device__ __forceinline__ void summary_elements(const SummaryJob& j, int64_t i0, float scale, const float* scale_dev, bool unit,
                                                 const float* lim, unsigned* hist, SummaryAcc& acc) {
  const T* p = (const T*)j.base;
  const bool dense = j.rows == 1 || j.row_stride == (int64_t)j.row_valid;
  const float dev = scale_dev ? scale_dev[0] : 1.f;
  for (int e0 = threadIdx.x; e0 < SUM_EPB; e0 += SUM_THREADS * SUM_U) {
    float x[SUM_U];
    bool in[SUM_U];
#pragma unroll
    for (int u = 0; u < SUM_U; ++u) {      // SUM_U independent loads in flight
      const int64_t i = i0 + e0 + u * SUM_THREADS;
      in[u] = i < (int64_t)j.numel;
      x[u] = 0.f;
      if (in[u]) {
        int64_t off = i;
        if (!dense) {
          const uint32_t r = (uint32_t)i / j.row_valid;
          off = (int64_t)r * j.row_stride + ((uint32_t)i - r * j.row_valid);
        }
        x[u] = ld<T>(p + off);
      }
    }
#pragma unroll
    for (int u = 0; u < SUM_U; ++u) {
      if (!in[u]) continue;
      float v = x[u];
      if (!unit) {
        v *= scale;
        if (scale_dev) v *= dev;
      }
      if (nonfinite_bits(v)) {
        ++acc.nonfinite;
        continue;
      }
      ++acc.num;
      acc.zeros += v == 0.f;
      acc.mn = fminf(acc.mn, v);
      acc.mx = fmaxf(acc.mx, v);
      const double d = (double)v;
      acc.sum += d;
      acc.sumsq += d * d;
      atomicAdd(&hist[summary_bucket(v, lim)], 1u);
    }
  }
}

__device__ __forceinline__ int summary_find_job(const SummaryJob* jobs, int njobs, int b) {
  int lo = 0, hi = njobs - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (b >= jobs[mid].block_end) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(SUM_THREADS) void summary_partial_kernel(const SummaryJob* __restrict__ jobs, int njobs, int nout, float scale,
                                                                      const float* __restrict__ scale_dev,
                                                                      const float* __restrict__ limits, uint32_t* __restrict__ buckets,
                                                                      SummaryPartial* __restrict__ partials) {
  __shared__ unsigned hist[TG_SUMMARY_BUCKETS];
  __shared__ float lim[SUM_NL];
  __shared__ SummaryPartial red[SUM_THREADS / TG_WAVE];
  const int b = blockIdx.x, tid = threadIdx.x;
  const SummaryJob j = jobs[summary_find_job(jobs, njobs, b)];
  // a grid larger than the table's total, a job whose result row the caller did not provide: nothing to do (uniform)
  if (b < j.block_begin || b >= j.block_end || j.out >= nout) return;
  for (int i = tid; i < TG_SUMMARY_BUCKETS; i += SUM_THREADS) hist[i] = 0u;
  for (int i = tid; i < SUM_NL; i += SUM_THREADS) lim[i] = limits[i];
  __syncthreads();
  SummaryAcc acc;
  const int64_t i0 = (int64_t)(b - j.block_begin) * SUM_EPB;
  const bool unit = scale == 1.f && !scale_dev;
  if (j.dtype == TG_F32) summary_elements<float>(j, i0, scale, scale_dev, unit, lim, hist, acc);
  else if (j.dtype == TG_BF16) summary_elements<bf16>(j, i0, scale, scale_dev, unit, lim, hist, acc);
  else summary_elements<f16>(j, i0, scale, scale_dev, unit, lim, hist, acc);
  // the workgroup's partial, in a fixed order
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    acc.sum += __shfl_xor(acc.sum, o, 64);
    acc.sumsq += __shfl_xor(acc.sumsq, o, 64);
    acc.mn = fminf(acc.mn, __shfl_xor(acc.mn, o, 64));
    acc.mx = fmaxf(acc.mx, __shfl_xor(acc.mx, o, 64));
    acc.num += __shfl_xor(acc.num, o, 64);
    acc.zeros += __shfl_xor(acc.zeros, o, 64);
    acc.nonfinite += __shfl_xor(acc.nonfinite, o, 64);
  }
  if ((tid & 63) == 0) red[tid >> 6] = SummaryPartial{acc.sum, acc.sumsq, acc.mn, acc.mx, acc.num, acc.zeros, acc.nonfinite, 0u};
  __syncthreads();      // also: every LDS histogram add of the workgroup is done
  if (tid == 0) {
    SummaryPartial r = red[0];
    for (int w = 1; w < SUM_THREADS / TG_WAVE; ++w) {
      r.sum += red[w].sum;
      r.sumsq += red[w].sumsq;
      r.mn = fminf(r.mn, red[w].mn);
      r.mx = fmaxf(r.mx, red[w].mx);
      r.num += red[w].num;
      r.zeros += red[w].zeros;
      r.nonfinite += red[w].nonfinite;
    }
    partials[b] = r;
  }
  uint32_t* dst = buckets + (size_t)j.out * TG_SUMMARY_BUCKETS;
  for (int i = tid; i < TG_SUMMARY_BUCKETS; i += SUM_THREADS) {
    const unsigned n = hist[i];
    if (n) atomicAdd(&dst[i], n);
  }
}

// one thread per job: its partials in block order
__global__ __launch_bounds__(64) void summary_finish_kernel(const SummaryJob* __restrict__ jobs, int njobs, int nout,
                                                            const SummaryPartial* __restrict__ partials,
                                                            TgSummaryStats* __restrict__ stats) {
  const int k = blockIdx.x * 64 + threadIdx.x;
  if (k >= njobs) return;
  const SummaryJob j = jobs[k];
  if (j.out >= nout) return;
  TgSummaryStats r{0.0, 0.0, SUM_FLT_MAX, -SUM_FLT_MAX, 0u, 0u, 0u, 0u};
  for (int b = j.block_begin; b < j.block_end; ++b) {
    const SummaryPartial p = partials[b];
    r.sum += p.sum;
    r.sum_squares += p.sumsq;
    r.min = fminf(r.min, p.mn);
    r.max = fmaxf(r.max, p.mx);
    r.num += p.num;
    r.zeros += p.zeros;
    r.nonfinite += p.nonfinite;
  }
  stats[j.out] = r;
}

}  // namespace

extern "C" {

int tg_mbstd_fwd(const void* x, void* out, float* stat, int n, int groups, int hw, int c, int cpad, float eps, int dtype,
                 void* stream) {
  TG_CHECK(x && out && n > 0 && hw > 0 && c > 0 && cpad > c, TG_EINVAL, "tg_mbstd_fwd: bad arguments (cpad must exceed c)");
  TG_CHECK(groups > 0 && n % groups == 0, TG_EINVAL, "tg_mbstd_fwd: n (%d) not divisible by groups (%d)", n, groups);
  TG_DISPATCH_DTYPE(dtype, "tg_mbstd_fwd", {
    hipLaunchKernelGGL(mbstd_fwd_kernel<T>, dim3(groups), dim3(1024), 0, (hipStream_t)stream, (const T*)x, (T*)out, stat,
                       n / groups, hw, c, cpad, eps);
  });
  TG_LAUNCH_CHECK("tg_mbstd_fwd");
  return TG_OK;
}

int tg_mbstd_bwd(const void* gout, const void* x, void* gx, int n, int groups, int hw, int c, int cpad, float eps,
                 int dtype, void* stream) {
  TG_CHECK(gout && x && gx && n > 0 && hw > 0 && c > 0 && cpad > c, TG_EINVAL, "tg_mbstd_bwd: bad arguments");
  TG_CHECK(groups > 0 && n % groups == 0, TG_EINVAL, "tg_mbstd_bwd: n (%d) not divisible by groups (%d)", n, groups);
  TG_DISPATCH_DTYPE(dtype, "tg_mbstd_bwd", {
    int nsplit = (hw * c / mb_v<T>() + 255) / 256;
    if (nsplit < 1) nsplit = 1;
    if (nsplit > 8) nsplit = 8;
    hipLaunchKernelGGL(mbstd_bwd_kernel<T>, dim3(groups, nsplit), dim3(256), 0, (hipStream_t)stream, (const T*)gout, (const T*)x,
                       (T*)gx, n / groups, hw, c, cpad, eps);
  });
  TG_LAUNCH_CHECK("tg_mbstd_bwd");
  return TG_OK;
}

int tg_mbstd_bwd_bwd(const void* v, const void* gout, const void* x, void* ggout, void* gx2, int n, int groups, int hw, int c,
                     int cpad, float eps, int dtype, void* stream) {
  TG_CHECK(v && gout && x && n > 0 && hw > 0 && c > 0 && cpad > c, TG_EINVAL, "tg_mbstd_bwd_bwd: bad arguments");
  TG_CHECK(groups > 0 && n % groups == 0, TG_EINVAL, "tg_mbstd_bwd_bwd: n (%d) not divisible by groups (%d)", n, groups);
  TG_DISPATCH_DTYPE(dtype, "tg_mbstd_bwd_bwd", {
    constexpr int NTHR = sizeof(T) == 4 ? 512 : 1024;
    hipLaunchKernelGGL((mbstd_bwd_bwd_kernel<T, NTHR>), dim3(groups), dim3(NTHR), 0, (hipStream_t)stream, (const T*)v,
                       (const T*)gout, (const T*)x, (T*)ggout, (T*)gx2, n / groups, hw, c, cpad, eps);
  });
  TG_LAUNCH_CHECK("tg_mbstd_bwd_bwd");
  return TG_OK;
}

static int zero_unless(float* p, size_t bytes, int accumulate, hipStream_t s, const char* who) {
  if (!accumulate) return tg_zero_async(p, bytes, nullptr, 0, s);
  return TG_OK;
}

int tg_sum(const void* x, float* out, int64_t numel, float scale, int accumulate, int dtype, void* stream) {
  TG_CHECK(x && out && numel > 0, TG_EINVAL, "tg_sum: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  TG_DISPATCH_DTYPE(dtype, "tg_sum", {
    const int blocks = exact_grid<T>() ? 1 : tg_grid_for(numel / Vec16<T>::N + 1, 256, 1024);
    const int direct = (blocks == 1 && !accumulate) ? 1 : 0;      // the [B, 1] predictions of the loss tails: one launch, not two
    if (!direct) {
      int rc = zero_unless(out, sizeof(float), accumulate, s, "tg_sum");
      if (rc) return rc;
    }
    hipLaunchKernelGGL((sum_kernel<T, 0>), dim3(blocks), dim3(256), 0, s, (const T*)x, (const T*)nullptr, out, numel, scale, direct,
                       tg_aligned16(x));
  });
  TG_LAUNCH_CHECK("tg_sum");
  return TG_OK;
}

int tg_abs_diff_sum(const void* a, const void* b, float* out, int64_t numel, float scale, int accumulate, int dtype,
                    void* stream) {
  TG_CHECK(a && b && out && numel > 0, TG_EINVAL, "tg_abs_diff_sum: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  TG_DISPATCH_DTYPE(dtype, "tg_abs_diff_sum", {
    const int blocks = exact_grid<T>() ? 1 : tg_grid_for(numel / Vec16<T>::N + 1, 256, 1024);
    const int direct = (blocks == 1 && !accumulate) ? 1 : 0;
    if (!direct) {
      int rc = zero_unless(out, sizeof(float), accumulate, s, "tg_abs_diff_sum");
      if (rc) return rc;
    }
    hipLaunchKernelGGL((sum_kernel<T, 1>), dim3(blocks), dim3(256), 0, s, (const T*)a, (const T*)b, out, numel, scale, direct,
                       tg_aligned16(a) && tg_aligned16(b));
  });
  TG_LAUNCH_CHECK("tg_abs_diff_sum");
  return TG_OK;
}

// The two sums above with per-workgroup partials in a caller workspace, added in workgroup order: the same value on
// every run whatever the storage type and whatever the mode (the plain entry points end in one fp32 atomic per workgroup)
int tg_sum_ordered(const void* x, const void* y_or_null, float* out, int64_t numel, float scale, int accumulate, float* ws,
                   size_t ws_floats, int dtype, void* stream) {
  TG_CHECK(x && out && ws && ws_floats >= 1 && numel > 0, TG_EINVAL, "tg_sum_ordered: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  int blocks = 0;
  TG_DISPATCH_DTYPE(dtype, "tg_sum_ordered", {
    blocks = tg_grid_for(numel / Vec16<T>::N + 1, 256, 512);
    if ((size_t)blocks > ws_floats) blocks = (int)ws_floats;
    if (y_or_null)
      hipLaunchKernelGGL((sum_kernel<T, 1, true>), dim3(blocks), dim3(256), 0, s, (const T*)x, (const T*)y_or_null, ws, numel, 1.f, 0,
                         tg_aligned16(x) && tg_aligned16(y_or_null));
    else
      hipLaunchKernelGGL((sum_kernel<T, 0, true>), dim3(blocks), dim3(256), 0, s, (const T*)x, (const T*)nullptr, ws, numel, 1.f, 0,
                         tg_aligned16(x));
  });
  hipLaunchKernelGGL(ordered_scalar_sum_kernel, dim3(1), dim3(64), 0, s, ws, blocks, out, scale, accumulate);
  TG_LAUNCH_CHECK("tg_sum_ordered");
  return TG_OK;
}

int tg_abs_diff_bwd(const void* a, const void* b, const float* gscale, void* ga, void* gb, int64_t numel, float scale,
                    int dtype, void* stream) {
  TG_CHECK(a && b && numel > 0 && (ga || gb), TG_EINVAL, "tg_abs_diff_bwd: bad arguments");
  TG_DISPATCH_DTYPE(dtype, "tg_abs_diff_bwd", {
    hipLaunchKernelGGL(abs_diff_bwd_kernel<T>, dim3(tg_grid_for(numel, 256)), dim3(256), 0, (hipStream_t)stream,
                       (const T*)a, (const T*)b, gscale, (T*)ga, (T*)gb, numel, scale);
  });
  TG_LAUNCH_CHECK("tg_abs_diff_bwd");
  return TG_OK;
}

int tg_sample_sumsq(const void* x, float* out, int batch, int64_t per, int dtype, void* stream) {
  TG_CHECK(x && out && batch > 0 && per > 0, TG_EINVAL, "tg_sample_sumsq: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  int rc = zero_unless(out, (size_t)batch * sizeof(float), 0, s, "tg_sample_sumsq");
  if (rc) return rc;
  TG_DISPATCH_DTYPE(dtype, "tg_sample_sumsq", {
    const int chunks = exact_grid<T>() ? 1 : tg_grid_for(per / Vec16<T>::N + 1, 256, 64);
    // sample b starts at x + b * per: on a 16-byte boundary for every b only when per is a multiple of the vector width
    const int vec = tg_aligned16(x) && (batch == 1 || per % Vec16<T>::N == 0);
    hipLaunchKernelGGL(sample_sumsq_kernel<T>, dim3(chunks, batch), dim3(256), 0, s, (const T*)x, out, per, vec);
  });
  TG_LAUNCH_CHECK("tg_sample_sumsq");
  return TG_OK;
}

int tg_gp_penalty(const float* sumsq, float* loss, float* coef, int batch, float lambda, void* stream) {
  TG_CHECK(sumsq && batch > 0, TG_EINVAL, "tg_gp_penalty: bad arguments");
  hipLaunchKernelGGL(gp_penalty_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, sumsq, loss, coef, batch, lambda);
  TG_LAUNCH_CHECK("tg_gp_penalty");
  return TG_OK;
}

int tg_pred_loss_fwd(const float* x, float* out, int n, int mode, float a, float b, float scale, int accumulate,
                     void* stream) {
  TG_CHECK(x && out && n > 0 && mode >= 0 && mode <= 3, TG_EINVAL, "tg_pred_loss_fwd: bad arguments");
  hipLaunchKernelGGL(pred_loss_fwd_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, x, out, n, mode, a, b, scale,
                     accumulate);
  TG_LAUNCH_CHECK("tg_pred_loss_fwd");
  return TG_OK;
}

int tg_pred_loss_bwd(const float* x, const float* gscale, float* gx, int n, int mode, float a, float b, float scale,
                     void* stream) {
  TG_CHECK(x && gx && n > 0 && mode >= 0 && mode <= 3, TG_EINVAL, "tg_pred_loss_bwd: bad arguments");
  hipLaunchKernelGGL(pred_loss_bwd_kernel, dim3(tg_grid_for(n, 256)), dim3(256), 0, (hipStream_t)stream, x, gscale, gx, n,
                     mode, a, b, scale);
  TG_LAUNCH_CHECK("tg_pred_loss_bwd");
  return TG_OK;
}

int tg_pred_losses_fwd(const float* pred, int group_size, int groups, const TgPredJob* jobs, int njobs, float* terms, int nterms,
                       void* stream) {
  TG_CHECK(pred && jobs && terms && group_size > 0 && groups > 0 && njobs > 0 && njobs <= PRED_MAX_JOBS && nterms > 0 &&
               nterms <= PRED_MAX_TERMS, TG_EINVAL, "tg_pred_losses_fwd: bad arguments (at most %d jobs, %d terms)", PRED_MAX_JOBS,
           PRED_MAX_TERMS);
  PredJobs pj;
  pj.n = njobs;
  for (int j = 0; j < njobs; ++j) {
    TG_CHECK(jobs[j].group >= 0 && jobs[j].group < groups && jobs[j].term >= 0 && jobs[j].term < nterms && jobs[j].mode >= 0 &&
                 jobs[j].mode <= 3, TG_EINVAL, "tg_pred_losses_fwd: job %d out of range", j);
    pj.j[j] = jobs[j];
  }
  hipLaunchKernelGGL(pred_losses_fwd_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, pred, group_size, pj, terms, nterms);
  TG_LAUNCH_CHECK("tg_pred_losses_fwd");
  return TG_OK;
}

int tg_pred_losses_bwd(const float* pred, int group_size, int groups, const TgPredJob* jobs, int njobs, const float* const* gterms,
                       int nterms, float* gpred, void* stream) {
  TG_CHECK(pred && jobs && gterms && gpred && group_size > 0 && groups > 0 && njobs > 0 && njobs <= PRED_MAX_JOBS && nterms > 0 &&
               nterms <= PRED_MAX_TERMS, TG_EINVAL, "tg_pred_losses_bwd: bad arguments");
  PredJobs pj;
  pj.n = njobs;
  for (int j = 0; j < njobs; ++j) {
    TG_CHECK(jobs[j].group >= 0 && jobs[j].group < groups && jobs[j].term >= 0 && jobs[j].term < nterms, TG_EINVAL,
             "tg_pred_losses_bwd: job %d out of range", j);
    pj.j[j] = jobs[j];
  }
  PredGrads pg;
  for (int t = 0; t < PRED_MAX_TERMS; ++t) pg.g[t] = t < nterms ? gterms[t] : nullptr;
  hipLaunchKernelGGL(pred_losses_bwd_kernel, dim3(tg_grid_for((int64_t)group_size * groups, 256, 64)), dim3(256), 0,
                     (hipStream_t)stream, pred, group_size, groups, pj, pg, gpred);
  TG_LAUNCH_CHECK("tg_pred_losses_bwd");
  return TG_OK;
}

int tg_sum_scalars(const float* const* scalars, int n, float* out, void* stream) {
  TG_CHECK(scalars && out && n > 0 && n <= 24, TG_EINVAL, "tg_sum_scalars: 1..24 scalars");
  ScalarPtrs a;
  a.n = n;
  for (int i = 0; i < n; ++i) {
    TG_CHECK(scalars[i], TG_EINVAL, "tg_sum_scalars: null scalar %d", i);
    a.p[i] = scalars[i];
  }
  hipLaunchKernelGGL(sum_scalars_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, a, out);
  TG_LAUNCH_CHECK("tg_sum_scalars");
  return TG_OK;
}

int tg_cosine_distance_fwd(const float* expected, const float* embedding, float* out, int batch, int dim, float weight,
                           void* stream) {
  TG_CHECK(expected && embedding && out && batch > 0 && dim > 0, TG_EINVAL, "tg_cosine_distance_fwd: bad arguments");
  hipLaunchKernelGGL(cosine_distance_fwd_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, expected, embedding, out, batch,
                     dim, weight / (float)batch);
  TG_LAUNCH_CHECK("tg_cosine_distance_fwd");
  return TG_OK;
}

int tg_cosine_distance_bwd(const float* expected, const float* embedding, const float* gscale, float* g_embedding, int batch,
                           int dim, float weight, void* stream) {
  TG_CHECK(expected && embedding && gscale && g_embedding && batch > 0 && dim > 0, TG_EINVAL,
           "tg_cosine_distance_bwd: bad arguments");
  hipLaunchKernelGGL(cosine_distance_bwd_kernel, dim3(batch), dim3(256), 0, (hipStream_t)stream, expected, embedding, gscale,
                     g_embedding, dim, weight / (float)batch);
  TG_LAUNCH_CHECK("tg_cosine_distance_bwd");
  return TG_OK;
}

int tg_var_from_sums(const float* sum, const float* sample_sumsq, float* out, int batch, int64_t numel, void* stream) {
  TG_CHECK(sum && sample_sumsq && out && batch > 0 && numel > 0, TG_EINVAL, "tg_var_from_sums: bad arguments");
  hipLaunchKernelGGL(var_from_sums_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, sum, sample_sumsq, out, batch,
                     1.0f / (float)numel);
  TG_LAUNCH_CHECK("tg_var_from_sums");
  return TG_OK;
}

int tg_small_gemm(const float* a, const float* b, const float* bias, float* c, int m, int n, int k, int ta, int tb,
                  int accumulate, void* stream) {
  TG_CHECK(a && b && c && m > 0 && n > 0 && k > 0, TG_EINVAL, "tg_small_gemm: bad arguments");
  if (k >= 32 && (int64_t)m * n <= 4096)
    hipLaunchKernelGGL(small_gemm_wave_kernel, dim3(tg_grid_for((int64_t)m * n * 64, 256)), dim3(256), 0,
                       (hipStream_t)stream, a, b, bias, c, m, n, k, ta, tb, accumulate);
  else
    hipLaunchKernelGGL(small_gemm_kernel, dim3(tg_grid_for((int64_t)m * n, 256)), dim3(256), 0, (hipStream_t)stream, a, b,
                       bias, c, m, n, k, ta, tb, accumulate);
  TG_LAUNCH_CHECK("tg_small_gemm");
  return TG_OK;
}

int tg_fc_fwd(const void* x, const float* w, const float* bias, float* y, int m, int n, int k, int dtype, void* stream) {
  TG_CHECK(x && w && y && m > 0 && n > 0 && k > 0, TG_EINVAL, "tg_fc_fwd: bad arguments");
  TG_DISPATCH_DTYPE(dtype, "tg_fc_fwd", {
    hipLaunchKernelGGL(fc_fwd_kernel<T>, dim3(tg_grid_for((int64_t)m * n * 64, 256)), dim3(256), 0, (hipStream_t)stream,
                       (const T*)x, w, bias, y, m, n, k);
  });
  TG_LAUNCH_CHECK("tg_fc_fwd");
  return TG_OK;
}

int tg_fc_bwd(const void* x, const float* w, const float* g, void* gx, float* gw, float* gb, int m, int n, int k, int acc_w,
              int acc_b, int dtype, void* stream) {
  TG_CHECK(x && w && g && (gx || gw || gb) && m > 0 && n > 0 && k > 0 && n <= k, TG_EINVAL, "tg_fc_bwd: bad arguments");
  TG_DISPATCH_DTYPE(dtype, "tg_fc_bwd", {
    hipLaunchKernelGGL(fc_bwd_kernel<T>, dim3(tg_grid_for(k, 64)), dim3(64), 0, (hipStream_t)stream, (const T*)x, w, g, (T*)gx,
                       gw, gb, m, n, k, acc_w, acc_b);
  });
  TG_LAUNCH_CHECK("tg_fc_bwd");
  return TG_OK;
}

int tg_adam_step(float* theta, const float* grad, float* m, float* v, void* theta_bf16, int64_t numel, float lr_t,
                 const float* lr_t_dev, float beta1, float beta2, float eps, float grad_scale, void* stream) {
  TG_CHECK(theta && grad && m && v && numel > 0, TG_EINVAL, "tg_adam_step: bad arguments");
  ApplyArgs a{theta, grad, m, v, numel, {lr_t, beta1, beta2, eps}, grad_scale};
  a.lr_t_dev = lr_t_dev;
  a.shadow = (bf16*)theta_bf16;
  return launch_apply<TG_OPT_ADAM>(a, stream, "tg_adam_step");
}

int tg_adam_ema_step(float* theta, const float* grad, float* m, float* v, float* avg, int64_t numel, const float* lr_t_dev,
                     float beta1, float beta2, float eps, float grad_scale, const float* w_dev, void* stream) {
  TG_CHECK(theta && grad && m && v && avg && lr_t_dev && w_dev, TG_EINVAL, "tg_adam_ema_step: null pointer");
  TG_CHECK(numel > 0, TG_EINVAL, "tg_adam_ema_step: numel must be positive (got %lld)", (long long)numel);
  return launch_apply<TG_OPT_ADAM>({theta, grad, m, v, numel, {0.f, beta1, beta2, eps}, grad_scale, nullptr, avg, w_dev, lr_t_dev},
                                   stream, "tg_adam_ema_step");
}

int tg_ema_update(float* avg, const float* var, int64_t numel, const float* w_dev, void* stream) {
  TG_CHECK(avg && var && w_dev, TG_EINVAL, "tg_ema_update: null pointer");
  TG_CHECK(numel > 0, TG_EINVAL, "tg_ema_update: numel must be positive (got %lld)", (long long)numel);
  if (tg_aligned16(avg) && tg_aligned16(var))
    hipLaunchKernelGGL(ema_kernel<true>, dim3(tg_grid_for((numel + 3) / 4, 256)), dim3(256), 0, (hipStream_t)stream, avg, var,
                       numel, w_dev);
  else
    hipLaunchKernelGGL(ema_kernel<false>, dim3(tg_grid_for(numel, 256)), dim3(256), 0, (hipStream_t)stream, avg, var, numel,
                       w_dev);
  TG_LAUNCH_CHECK("tg_ema_update");
  return TG_OK;
}

size_t tg_ema_table_bytes(int njobs) { return (size_t)(njobs > 0 ? njobs : 0) * sizeof(EmaJob); }

int tg_ema_table_fill(float* avg, const float* var, int64_t numel, int job, void* table_host, int32_t* total_blocks) {
  TG_CHECK(avg && var && table_host && total_blocks && job >= 0, TG_EINVAL, "tg_ema_table_fill: bad arguments");
  TG_CHECK(numel > 0, TG_EINVAL, "tg_ema_table_fill: numel must be positive (got %lld)", (long long)numel);
  const int64_t blocks = (numel + EMA_EPB - 1) / EMA_EPB;
  TG_CHECK(*total_blocks >= 0 && *total_blocks + blocks <= 0x7fffffff, TG_EINVAL, "tg_ema_table_fill: grid too large");
  EmaJob j;
  j.avg = avg;
  j.var = var;
  j.numel = numel;
  j.block_begin = *total_blocks;
  j.block_end = j.block_begin + (int)blocks;
  *total_blocks = j.block_end;
  ((EmaJob*)table_host)[job] = j;
  return TG_OK;
}

int tg_ema_update_multi(const void* table_device, int njobs, int total_blocks, const float* w_dev, void* stream) {
  TG_CHECK(table_device && w_dev, TG_EINVAL, "tg_ema_update_multi: null pointer");
  TG_CHECK(njobs > 0 && total_blocks > 0, TG_EINVAL, "tg_ema_update_multi: njobs and total_blocks must be positive (got %d, %d)",
           njobs, total_blocks);
  hipLaunchKernelGGL(ema_multi_kernel, dim3(total_blocks), dim3(256), 0, (hipStream_t)stream, (const EmaJob*)table_device, njobs,
                     w_dev);
  TG_LAUNCH_CHECK("tg_ema_update_multi");
  return TG_OK;
}

int tg_adam_tick(int64_t* step_dev, float* lr_t_dev, float lr, float beta1, float beta2, void* stream) {
  TG_CHECK(step_dev && lr_t_dev, TG_EINVAL, "tg_adam_tick: null pointer");
  hipLaunchKernelGGL(adam_tick_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, step_dev, lr_t_dev, lr, beta1, beta2);
  TG_LAUNCH_CHECK("tg_adam_tick");
  return TG_OK;
}

size_t tg_loss_scale_state_bytes(void) { return sizeof(TgLossScaleState); }

int tg_nonfinite_check(const float* x, int64_t numel, TgLossScaleState* state, void* stream) {
  TG_CHECK(x && state, TG_EINVAL, "tg_nonfinite_check: null pointer");
  TG_CHECK(numel > 0, TG_EINVAL, "tg_nonfinite_check: numel must be positive (got %lld)", (long long)numel);
  // at most 2048 workgroups (8 per CU, 32 KiB of loads in flight per CU with 16 bytes per lane); the rest is the grid stride
  if (tg_aligned16(x))
    hipLaunchKernelGGL(nonfinite_kernel<true>, dim3(tg_grid_for((numel + 4 * TG_NF_U - 1) / (4 * TG_NF_U), 256, TG_NF_CAP)), dim3(256), 0, (hipStream_t)stream,
                       x, numel, state);
  else
    hipLaunchKernelGGL(nonfinite_kernel<false>, dim3(tg_grid_for(numel, 256, 2048)), dim3(256), 0, (hipStream_t)stream, x,
                       numel, state);
  TG_LAUNCH_CHECK("tg_nonfinite_check");
  return TG_OK;
}

int tg_loss_scale_tick(TgLossScaleState* state, int64_t* step_dev, float* lr_t_dev, float lr, float beta1, float beta2,
                       int growth_interval, float max_scale, int world, void* stream) {
  TG_CHECK(state && step_dev && lr_t_dev, TG_EINVAL, "tg_loss_scale_tick: null pointer");
  TG_CHECK(growth_interval >= 1 && max_scale >= 1.f && world >= 1, TG_EINVAL,
           "tg_loss_scale_tick: growth_interval (%d), max_scale (%g) and world (%d) must be at least 1", growth_interval,
           (double)max_scale, world);
  hipLaunchKernelGGL(loss_scale_tick_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state, step_dev, lr_t_dev, lr, beta1,
                     beta2, growth_interval, max_scale, world);
  TG_LAUNCH_CHECK("tg_loss_scale_tick");
  return TG_OK;
}

int tg_adam_step_guarded(float* theta, const float* grad, float* m, float* v, int64_t numel, const float* lr_t_dev,
                         float beta1, float beta2, float eps, const TgLossScaleState* state, void* stream) {
  TG_CHECK(theta && grad && m && v && lr_t_dev && state, TG_EINVAL, "tg_adam_step_guarded: null pointer");
  TG_CHECK(numel > 0, TG_EINVAL, "tg_adam_step_guarded: numel must be positive (got %lld)", (long long)numel);
  return launch_apply<TG_OPT_ADAM>({theta, grad, m, v, numel, {0.f, beta1, beta2, eps}, 0.f, state, nullptr, nullptr, lr_t_dev}, stream,
                                   "tg_adam_step_guarded");
}

int tg_adam_ema_step_guarded(float* theta, const float* grad, float* m, float* v, float* avg, int64_t numel,
                             const float* lr_t_dev, float beta1, float beta2, float eps, const TgLossScaleState* state,
                             const float* w_dev, void* stream) {
  TG_CHECK(theta && grad && m && v && avg && lr_t_dev && state && w_dev, TG_EINVAL, "tg_adam_ema_step_guarded: null pointer");
  TG_CHECK(numel > 0, TG_EINVAL, "tg_adam_ema_step_guarded: numel must be positive (got %lld)", (long long)numel);
  return launch_apply<TG_OPT_ADAM>({theta, grad, m, v, numel, {0.f, beta1, beta2, eps}, 0.f, state, avg, w_dev, lr_t_dev}, stream,
                                   "tg_adam_ema_step_guarded");
}

int tg_optim_slot_count(int rule) { return rule >= TG_OPT_SGD && rule <= TG_OPT_FTRL ? optim_slots(rule) : -1; }

int tg_optim_step(int rule, float* theta, const float* grad, float* slot0, float* slot1, float* avg, int64_t numel,
                  const TgOptimHyper* hyper, float grad_scale, const TgLossScaleState* guard, const float* w_dev, void* stream) {
  const int ns = tg_optim_slot_count(rule);
  TG_CHECK(ns >= 0, TG_EINVAL, "tg_optim_step: unknown rule %d", rule);
  TG_CHECK(theta, TG_EINVAL, "tg_optim_step: theta is null");
  TG_CHECK(grad, TG_EINVAL, "tg_optim_step: grad is null");
  TG_CHECK(hyper, TG_EINVAL, "tg_optim_step: hyper is null");
  TG_CHECK(numel > 0, TG_EINVAL, "tg_optim_step: numel must be positive (got %lld)", (long long)numel);
  TG_CHECK(ns < 1 || slot0, TG_EINVAL, "tg_optim_step: slot0 is null and rule %d needs it", rule);
  TG_CHECK(ns < 2 || slot1, TG_EINVAL, "tg_optim_step: slot1 is null and rule %d needs it", rule);
  TG_CHECK(!avg || w_dev, TG_EINVAL, "tg_optim_step: avg without w_dev");
  TG_CHECK(avg || !w_dev, TG_EINVAL, "tg_optim_step: w_dev without avg");
  if (rule == TG_OPT_FTRL)
    TG_CHECK(hyper->lr_power <= 0.f, TG_EINVAL, "tg_optim_step: hyper->lr_power must not be positive (got %g)",
             (double)hyper->lr_power);
  const ApplyArgs a{theta, grad, ns >= 1 ? slot0 : nullptr, ns >= 2 ? slot1 : nullptr, numel, *hyper, grad_scale, guard, avg, w_dev};
  const char* name = "tg_optim_step";
  switch (rule) {
    case TG_OPT_SGD: return launch_apply<TG_OPT_SGD>(a, stream, name);
    case TG_OPT_MOMENTUM: return launch_apply<TG_OPT_MOMENTUM>(a, stream, name);
    case TG_OPT_ADAGRAD: return launch_apply<TG_OPT_ADAGRAD>(a, stream, name);
    case TG_OPT_RMSPROP: return launch_apply<TG_OPT_RMSPROP>(a, stream, name);
    case TG_OPT_ADADELTA: return launch_apply<TG_OPT_ADADELTA>(a, stream, name);
    default: return hyper->lr_power == -0.5f ? launch_apply<TG_OPT_FTRL>(a, stream, name) : launch_apply<TG_OPT_FTRL_POW>(a, stream, name);
  }
}

int tg_summary_limits(double* limits, float* pos_limits_f32) {
  double pos[TG_SUMMARY_POS_LIMITS + 1];
  int n = 0;
  for (double v = 1e-12; v < 1e20; v *= 1.1) {
    TG_CHECK(n < TG_SUMMARY_POS_LIMITS, TG_ENOSUP, "tg_summary_limits: more than %d positive limits on this host", TG_SUMMARY_POS_LIMITS);
    pos[n++] = v;
  }
  TG_CHECK(n == TG_SUMMARY_POS_LIMITS, TG_ENOSUP, "tg_summary_limits: %d positive limits on this host, not %d", n, TG_SUMMARY_POS_LIMITS);
  float prev = 0.f;
  for (int k = 0; k < n; ++k) {
    float f = (float)pos[k];
    if ((double)f < pos[k]) f = nextafterf(f, INFINITY);
    TG_CHECK((double)f > pos[k] && f > prev, TG_ENOSUP, "tg_summary_limits: limit %d is a float itself or rounds onto its predecessor", k);
    prev = f;
    if (pos_limits_f32) pos_limits_f32[k] = f;
  }
  if (limits) {
    limits[0] = -1.7976931348623157e308;
    for (int k = 0; k < n; ++k) {
      limits[1 + k] = -pos[n - 1 - k];
      limits[n + 2 + k] = pos[k];
    }
    limits[n + 1] = 0.0;
    limits[2 * n + 2] = 1.7976931348623157e308;
  }
  return TG_OK;
}

size_t tg_summary_table_bytes(int njobs) { return (size_t)(njobs > 0 ? njobs : 0) * sizeof(SummaryJob); }

int tg_summary_table_fill(const void* base, int dtype, int64_t rows, int64_t row_valid, int64_t row_stride, int out, int job,
                          void* table_host, int32_t* total_blocks) {
  TG_CHECK(base, TG_EINVAL, "tg_summary_table_fill: base is null");
  TG_CHECK(table_host, TG_EINVAL, "tg_summary_table_fill: table_host is null");
  TG_CHECK(total_blocks, TG_EINVAL, "tg_summary_table_fill: total_blocks is null");
  TG_CHECK(dtype == TG_F32 || dtype == TG_BF16 || dtype == TG_F16, TG_EINVAL, "tg_summary_table_fill: unsupported dtype %d", dtype);
  TG_CHECK(rows >= 1, TG_EINVAL, "tg_summary_table_fill: rows must be positive (got %lld)", (long long)rows);
  TG_CHECK(row_valid >= 1, TG_EINVAL, "tg_summary_table_fill: row_valid must be positive (got %lld)", (long long)row_valid);
  TG_CHECK(row_stride >= row_valid, TG_EINVAL, "tg_summary_table_fill: row_stride (%lld) is below row_valid (%lld)",
           (long long)row_stride, (long long)row_valid);
  TG_CHECK(out >= 0, TG_EINVAL, "tg_summary_table_fill: out must not be negative (got %d)", out);
  TG_CHECK(job >= 0, TG_EINVAL, "tg_summary_table_fill: job must not be negative (got %d)", job);
  TG_CHECK(rows < (1ll << 32) && row_valid < (1ll << 32) && rows * row_valid < (1ll << 32), TG_EINVAL,
           "tg_summary_table_fill: rows * row_valid (%lld x %lld) must stay below 2^32 elements", (long long)rows, (long long)row_valid);
  const int64_t numel = rows * row_valid, blocks = (numel + SUM_EPB - 1) / SUM_EPB;
  TG_CHECK(*total_blocks >= 0 && *total_blocks + blocks <= 0x7fffffff, TG_EINVAL, "tg_summary_table_fill: total_blocks: grid too large");
  SummaryJob j;
  j.base = base;
  j.row_stride = row_stride;
  j.rows = (uint32_t)rows;
  j.row_valid = (uint32_t)row_valid;
  j.numel = (uint32_t)numel;
  j.dtype = dtype;
  j.out = out;
  j.block_begin = *total_blocks;
  j.block_end = j.block_begin + (int)blocks;
  *total_blocks = j.block_end;
  ((SummaryJob*)table_host)[job] = j;
  return TG_OK;
}

size_t tg_summary_workspace_bytes(int total_blocks) { return (size_t)(total_blocks > 0 ? total_blocks : 0) * sizeof(SummaryPartial); }

int tg_summary_multi(const void* table_device, int njobs, int total_blocks, int nout, float scale, const float* scale_dev,
                     const float* limits_dev, TgSummaryStats* stats, uint32_t* buckets, void* workspace, size_t workspace_bytes,
                     void* stream) {
  TG_CHECK(table_device, TG_EINVAL, "tg_summary_multi: table_device is null");
  TG_CHECK(limits_dev, TG_EINVAL, "tg_summary_multi: limits_dev is null");
  TG_CHECK(stats, TG_EINVAL, "tg_summary_multi: stats is null");
  TG_CHECK(buckets, TG_EINVAL, "tg_summary_multi: buckets is null");
  TG_CHECK(workspace, TG_EINVAL, "tg_summary_multi: workspace is null");
  TG_CHECK(njobs > 0 && total_blocks > 0 && nout > 0, TG_EINVAL,
           "tg_summary_multi: njobs, total_blocks and nout must be positive (got %d, %d, %d)", njobs, total_blocks, nout);
  TG_CHECK(workspace_bytes >= tg_summary_workspace_bytes(total_blocks), TG_EINVAL,
           "tg_summary_multi: workspace_bytes %zu is below the %zu that %d blocks need", workspace_bytes,
           tg_summary_workspace_bytes(total_blocks), total_blocks);
  hipStream_t s = (hipStream_t)stream;
  const int rc = tg_zero_async(buckets, (size_t)nout * TG_SUMMARY_BUCKETS * sizeof(uint32_t), nullptr, 0, s);
  if (rc != TG_OK) return rc;
  hipLaunchKernelGGL(summary_partial_kernel, dim3(total_blocks), dim3(SUM_THREADS), 0, s, (const SummaryJob*)table_device, njobs, nout, scale,
                     scale_dev, limits_dev, buckets, (SummaryPartial*)workspace);
  TG_LAUNCH_CHECK("tg_summary_multi");
  hipLaunchKernelGGL(summary_finish_kernel, dim3((njobs + 63) / 64), dim3(64), 0, s, (const SummaryJob*)table_device, njobs, nout,
                     (const SummaryPartial*)workspace, stats);
  TG_LAUNCH_CHECK("tg_summary_multi");
  return TG_OK;
}

}  // extern "C"
