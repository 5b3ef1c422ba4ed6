// Training-image preprocessing on the GPU: decoded uint8 images of arbitrary size -> the [n, hw, hw, 3] batch in [0, 1]
// the networks train on.  One launch per batch, one thread per output pixel.
//
// Reference call site replaced: preprocessing/danbooru_preprocessing.py:115-230 (preprocess_image, the factory entry
// for the TwinGAN trainer: model/model_inheritor.py:403-457) with the trainer's defaults -- dtype conversion to [0, 1]
// (tf.image.convert_image_dtype), resize_mode PAD / CROP / RESHAPE to a square (preprocessing_util.py:97-146:
// pad_to_bounding_box / crop_to_bounding_box about the centre, then tf.image.resize_images BILINEAR,
// align_corners=False = the TF-1.x kernel without half-pixel centres), random_flip_left_right
// (preprocessing_util.py:171-205), distort_color in fast mode (danbooru_preprocessing.py:62-113: random_brightness
// max_delta 32/255 and random_saturation [0.5, 1.5) in one of two orders), tf.clip_by_value(0, 1).  The random draws are
// inputs (aug[n][4] = flip?, saturation first?, brightness delta, saturation factor): the host draws them.
//
// --do_random_cropping (model_inheritor.py:225,449-454; the reference's training recipe sets it, docs/training.md:22-23;
// danbooru_preprocessing.py:187-201, preprocessing_util.random_crop_image :312-331): the first bilinear resize goes to
// mid = int(hw / 0.8), tf.random_crop cuts a [ch, cw] rectangle out of that at (cy, cx) (crop[n][4] = cy, cx, ch, cw, drawn
// by the host), a second bilinear resize brings the rectangle to [hw, hw].  The kernel never materialises the mid x mid
// image: an output pixel's four taps in the rectangle are each evaluated from their four source taps (16 fetches).
// --color_space (model_inheritor.py:240,414; danbooru_preprocessing.py:208-225): 'gray' skips the colour distortion,
// 'yiq' / 'bgr' transform the finished image (preprocessing_util.rgb_to_yiq :154-160, tf.reverse on the channel axis).
//
// MS-SSIM evaluation (libs/ms_ssim.py:115-171 msssim, :39-110 _SSIMForMultiScale, :112 _HoxDownsample, :27-37 _FSpecialGauss;
// the metric docs/infer_and_eval.md names under "Evaluation"): the second half of this file.  One launch per level reads the
// two images of that level once, forms the five Gaussian-windowed moments separably in LDS, sums the ssim and cs maps per
// workgroup and writes the 2x2-mean pair the next level reads; an ordered pass per (level, image) and one small kernel finish.
#include "tg_common.h"
#include "../../include/twingan_hip_summary.h"

namespace {

struct PreGeom {
  int n, hw, mid, color_space;      // mid: side of the intermediate image (with a crop table); TG_CS_*
};

enum { TG_CS_RGB = 0, TG_CS_YIQ = 1, TG_CS_BGR = 2, TG_CS_GRAY = 3 };

__device__ __forceinline__ float3 fetch(const uint8_t* img, int h, int w, int y0, int x0, int vy, int vx) {
  // virtual source pixel (vy, vx) -> image pixel (vy + y0, vx + x0); outside the image: the zero padding
  const int y = vy + y0, x = vx + x0;
  if (y < 0 || y >= h || x < 0 || x >= w) return make_float3(0.f, 0.f, 0.f);
  const uint8_t* p = img + ((int64_t)y * w + x) * 3;
  const float k = 1.0f / 255.0f;      // tf.image.convert_image_dtype(uint8 -> float32): cast * (1 / max)
  return make_float3((float)p[0] * k, (float)p[1] * k, (float)p[2] * k);
}

__device__ __forceinline__ float3 lerp3(float3 a, float3 b, float t) {
  return make_float3(a.x + (b.x - a.x) * t, a.y + (b.y - a.y) * t, a.z + (b.z - a.z) * t);
}

// tf.image.adjust_saturation: RGB -> HSV, s = clip(s * factor, 0, 1), HSV -> RGB.  Hue and value do not change, and
// v - channel = s * v * (1 - d_channel(h)) is linear in s, so the round trip is  v - (v - channel) * (s' / s).
__device__ __forceinline__ float3 saturate(float3 c, float factor) {
  const float v = fmaxf(c.x, fmaxf(c.y, c.z));
  const float range = v - fminf(c.x, fminf(c.y, c.z));
  if (!(v > 0.f) || !(range > 0.f)) return c;          // s = 0: grey stays grey
  const float s = range / v;
  const float ratio = fminf(s * factor, 1.f) / s;
  return make_float3(v - (v - c.x) * ratio, v - (v - c.y) * ratio, v - (v - c.z) * ratio);
}

struct Src {      // one decoded image and the rectangle of it (in image coordinates) that the first resize reads
  const uint8_t* img;
  int h, w, y0, x0, sh, sw;
};

// pixel (oy, ox) of ResizeBilinear(source rectangle -> [size, size]), align_corners = False: in = out * (in_size / out_size)
__device__ __forceinline__ float3 resized(const Src& s, int oy, int ox, float sy, float sx) {
  const float fy = (float)oy * sy, fx = (float)ox * sx;
  const int top = (int)floorf(fy), left = (int)floorf(fx);
  const int bot = min(top + 1, s.sh - 1), right = min(left + 1, s.sw - 1);
  const float ly = fy - (float)top, lx = fx - (float)left;
  const float3 t = lerp3(fetch(s.img, s.h, s.w, s.y0, s.x0, top, left), fetch(s.img, s.h, s.w, s.y0, s.x0, top, right), lx);
  const float3 b = lerp3(fetch(s.img, s.h, s.w, s.y0, s.x0, bot, left), fetch(s.img, s.h, s.w, s.y0, s.x0, bot, right), lx);
  return lerp3(t, b, ly);
}

template <typename T, bool CROP>
__global__ void preprocess_kernel(const uint8_t* __restrict__ packed, const int64_t* __restrict__ offsets,
                                  const int* __restrict__ rect, const int* __restrict__ crop,
                                  const float* __restrict__ aug, T* __restrict__ out, PreGeom g) {
  const int n = blockIdx.y;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= g.hw * g.hw) return;
  int oy = idx / g.hw, ox = idx - oy * g.hw;
  const int* r = rect + n * 6;                         // image h, w; source rectangle y0, x0, sh, sw
  Src s;
  s.img = packed + offsets[n];
  s.h = r[0], s.w = r[1], s.y0 = r[2], s.x0 = r[3], s.sh = r[4], s.sw = r[5];
  const float* a = aug + n * 4;
  if (a[0] != 0.f) ox = g.hw - 1 - ox;                 // tf.reverse(image, [1]) of the RESIZED image
  float3 c;
  if (CROP) {
    const int* cr = crop + n * 4;                      // the rectangle tf.random_crop cut out of the mid x mid image
    const int cy = cr[0], cx = cr[1], ch = cr[2], cw = cr[3];
    const float sy = (float)s.sh / (float)g.mid, sx = (float)s.sw / (float)g.mid;
    const float fy = (float)oy * ((float)ch / (float)g.hw), fx = (float)ox * ((float)cw / (float)g.hw);
    const int top = (int)floorf(fy), left = (int)floorf(fx);
    const int bot = min(top + 1, ch - 1), right = min(left + 1, cw - 1);
    const float ly = fy - (float)top, lx = fx - (float)left;
    const float3 t = lerp3(resized(s, cy + top, cx + left, sy, sx), resized(s, cy + top, cx + right, sy, sx), lx);
    const float3 b = lerp3(resized(s, cy + bot, cx + left, sy, sx), resized(s, cy + bot, cx + right, sy, sx), lx);
    c = lerp3(t, b, ly);
  } else {
    c = resized(s, oy, ox, (float)s.sh / (float)g.hw, (float)s.sw / (float)g.hw);
  }
  if (g.color_space != TG_CS_GRAY) {                   // danbooru_preprocessing.py:208-212: no distort_color for 'gray'
    const float delta = a[2], factor = a[3];
    if (a[1] == 0.f) {                                 // ordering 0: brightness, then saturation
      c = make_float3(c.x + delta, c.y + delta, c.z + delta);
      c = saturate(c, factor);
    } else {                                           // orderings 1-3 (fast mode): saturation, then brightness
      c = saturate(c, factor);
      c = make_float3(c.x + delta, c.y + delta, c.z + delta);
    }
    c = make_float3(fminf(fmaxf(c.x, 0.f), 1.f), fminf(fmaxf(c.y, 0.f), 1.f), fminf(fmaxf(c.z, 0.f), 1.f));
  }
  if (g.color_space == TG_CS_YIQ) {                    // preprocessing_util.rgb_to_yiq: tensordot with the fp32 matrix
    c = make_float3(0.299f * c.x + 0.587f * c.y + 0.114f * c.z, 0.596f * c.x - 0.274f * c.y - 0.322f * c.z,
                    0.211f * c.x - 0.523f * c.y + 0.312f * c.z);
  } else if (g.color_space == TG_CS_BGR) {
    c = make_float3(c.z, c.y, c.x);
  }
  T* o = out + (((int64_t)n * g.hw + oy) * g.hw + (a[0] != 0.f ? g.hw - 1 - ox : ox)) * 3;
  st(o + 0, c.x);
  st(o + 1, c.y);
  st(o + 2, c.z);
}

}  // namespace

extern "C" int tg_preprocess_images_crop(const void* packed, const int64_t* offsets, const int* rect, const int* crop,
                                         const float* aug, void* out, int n, int hw, int mid, int color_space, int dtype,
                                         void* stream) {
  TG_CHECK(packed && offsets && rect && aug && out && n > 0 && hw > 0, TG_EINVAL, "tg_preprocess_images: bad arguments");
  TG_CHECK(color_space >= TG_CS_RGB && color_space <= TG_CS_GRAY, TG_EINVAL, "tg_preprocess_images: color_space 0..3");
  TG_CHECK(!crop || mid >= hw, TG_EINVAL, "tg_preprocess_images: a crop table needs the intermediate size mid >= hw");
  PreGeom g;
  g.n = n;
  g.hw = hw;
  g.mid = mid;
  g.color_space = color_space;
  const dim3 grid((hw * hw + 255) / 256, n);
  TG_DISPATCH_DTYPE(dtype, "tg_preprocess_images", {
    if (crop)
      hipLaunchKernelGGL((preprocess_kernel<T, true>), grid, dim3(256), 0, (hipStream_t)stream, (const uint8_t*)packed,
                         offsets, rect, crop, aug, (T*)out, g);
    else
      hipLaunchKernelGGL((preprocess_kernel<T, false>), grid, dim3(256), 0, (hipStream_t)stream, (const uint8_t*)packed,
                         offsets, rect, crop, aug, (T*)out, g);
  });
  TG_LAUNCH_CHECK("tg_preprocess_images");
  return TG_OK;
}

extern "C" int tg_preprocess_images(const void* packed, const int64_t* offsets, const int* rect, const float* aug, void* out,
                                    int n, int hw, int dtype, void* stream) {
  return tg_preprocess_images_crop(packed, offsets, rect, nullptr, aug, out, n, hw, 0, TG_CS_RGB, dtype, stream);
}

// ---- MS-SSIM -------------------------------------------------------------------------------------------------------------
namespace {

enum { MS_TH = 16, MS_TW = 32, MS_K = 11, MS_RH = MS_TH + MS_K - 1, MS_RW = MS_TW + MS_K - 1, MS_HP = MS_TW + 1,
       MS_MAXC = 4, MS_RP_MAX = MS_RW * MS_MAXC + 1, MS_MAXL = 8 };

struct MsLevel {
  int h, w, c;            // this level's image size
  int oh, ow;             // size of the 'valid' ssim / cs maps: h - size + 1, w - size + 1
  float scale, off;       // a pixel enters as x * scale - off (off = max_val / 2 at the first level; later levels are stored so)
  float mu_off;           // what the windowed means get back: max_val / 2
  float c1, c2;
  float taps[MS_K];       // the 1-D window, normalised in double by the host; taps beyond `size` are 0
};

// One map position's ssim and cs terms from its five windowed moments (of the centred pixels).  No contraction here: every
// product is rounded before it is added, so that two identical images give numerator == denominator bit for bit and score
// exactly 1, as they do in the reference.
__device__ __forceinline__ void ms_terms(float m1, float m2, float e11, float e22, float e12, float mu_off, float c1, float c2,
                                         float* ssim, float* cs) {
#pragma clang fp contract(off)
  const float s11 = e11 - m1 * m1, s22 = e22 - m2 * m2, s12 = e12 - m1 * m2;
  const float mu1 = m1 + mu_off, mu2 = m2 + mu_off;
  const float v1 = 2.0f * s12 + c2, v2 = (s11 + s22) + c2;
  *ssim = ((2.0f * (mu1 * mu2) + c1) * v1) / (((mu1 * mu1 + mu2 * mu2) + c1) * v2);
  *cs = v1 / v2;
}

// One workgroup = one MS_TH x MS_TW tile of one image pair (grid: tiles x, tiles y, pair).  The tile of map positions and
// the tile of pixels that is pooled for the next level share the origin, which is even.  Pixels are centred on load: the
// variances are differences of numbers up to max_val^2 and lose bits that c2 does not hide on near-flat images; the
// (co)variances do not see the shift and the means get it back (the taps sum to 1).
template <typename T>
__global__ __launch_bounds__(256) void msssim_level_kernel(const T* __restrict__ img1, const T* __restrict__ img2,
                                                           float* __restrict__ out1, float* __restrict__ out2,
                                                           float* __restrict__ partial, MsLevel g) {
  // every fused multiply-add below is written out: left to the compiler, the moments of image 1, of image 2 and of their
  // product were contracted differently, and two identical images did not score exactly 1
#pragma clang fp contract(off)
  __shared__ float raw[2][MS_RH * MS_RP_MAX];      // both images' tile with halo, channels interleaved as in memory
  __shared__ float hb[5][MS_RH * MS_HP];           // one channel's row-filtered x1, x2, x1^2, x2^2, x1 x2
  __shared__ float red[8];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int C = g.c, rp = MS_RW * C + 1, wc = g.w * C;
  const int y0 = blockIdx.y * MS_TH, x0 = blockIdx.x * MS_TW, b = blockIdx.z;
  const int64_t base = (int64_t)b * g.h * wc;

  // the tile with its halo: every load of a thread is issued before the first LDS write waits for one (a loop that loads and
  // stores element by element runs at one memory latency per iteration with 12 waves on a CU)
  {
    constexpr int NR = (MS_RH + 3) / 4, NE = (MS_RW * MS_MAXC + 63) / 64;
    float v1[NR][NE], v2[NR][NE];
#pragma unroll
    for (int i = 0; i < NR; ++i) {
#pragma unroll
      for (int q = 0; q < NE; ++q) {
        const int row = wv + 4 * i, e = lane + 64 * q, gy = y0 + row, ge = x0 * C + e;
        v1[i][q] = 0.f, v2[i][q] = 0.f;
        if (row < MS_RH && e < MS_RW * C && gy < g.h && ge < wc) {
          const int64_t o = base + (int64_t)gy * wc + ge;
          v1[i][q] = fmaf(ld(img1 + o), g.scale, -g.off);
          v2[i][q] = fmaf(ld(img2 + o), g.scale, -g.off);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < NR; ++i) {
#pragma unroll
      for (int q = 0; q < NE; ++q) {
        const int row = wv + 4 * i, e = lane + 64 * q;
        if (row < MS_RH && e < MS_RW * C) {
          raw[0][row * rp + e] = v1[i][q];
          raw[1][row * rp + e] = v2[i][q];
        }
      }
    }
  }
  __syncthreads();

  if (out1) {      // _HoxDownsample of the tile's own pixels, in the reference's order of additions
    const int h2 = g.h >> 1, w2 = g.w >> 1, ne = (MS_TW / 2) * C;
    for (int i = tid; i < 2 * (MS_TH / 2) * ne; i += 256) {
      const int im = i / ((MS_TH / 2) * ne), r = i - im * (MS_TH / 2) * ne;
      const int oy = r / ne, e = r - oy * ne, ox = e / C, ch = e - ox * C;
      const int gy = (y0 >> 1) + oy, gx = (x0 >> 1) + ox;
      if (gy < h2 && gx < w2) {
        const float* p = raw[im] + (2 * oy) * rp + (2 * ox) * C + ch;
        const float v = (((p[0] + p[rp]) + p[C]) + p[rp + C]) * 0.25f;
        (im ? out2 : out1)[((int64_t)b * h2 + gy) * (w2 * C) + gx * C + ch] = v;
      }
    }
  }

  float ssum = 0.f, csum = 0.f;
  for (int ch = 0; ch < C; ++ch) {
    if (tid < MS_RH * (MS_TW / 4)) {      // rows: four adjacent map columns per thread from one sliding window of 14 pixels
      const int row = tid >> 3, xs = (tid & 7) * 4;
      const float* r1 = raw[0] + row * rp + xs * C + ch;
      const float* r2 = raw[1] + row * rp + xs * C + ch;
      float a1[4] = {0.f, 0.f, 0.f, 0.f}, a2[4] = {0.f, 0.f, 0.f, 0.f}, a11[4] = {0.f, 0.f, 0.f, 0.f},
            a22[4] = {0.f, 0.f, 0.f, 0.f}, a12[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int k = 0; k < MS_K + 3; ++k) {
        const float v1 = r1[k * C], v2 = r2[k * C];
        const float p11 = v1 * v1, p22 = v2 * v2, p12 = v1 * v2;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (k - j >= 0 && k - j < MS_K) {
            const float t = g.taps[k - j];
            a1[j] = fmaf(t, v1, a1[j]);
            a2[j] = fmaf(t, v2, a2[j]);
            a11[j] = fmaf(t, p11, a11[j]);
            a22[j] = fmaf(t, p22, a22[j]);
            a12[j] = fmaf(t, p12, a12[j]);
          }
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int o = row * MS_HP + xs + j;
        hb[0][o] = a1[j];
        hb[1][o] = a2[j];
        hb[2][o] = a11[j];
        hb[3][o] = a22[j];
        hb[4][o] = a12[j];
      }
    }
    __syncthreads();
    {      // columns: two map rows per thread from a window of 12 filtered rows, then the ssim / cs terms
      const int x = tid & 31, ys = (tid >> 5) * 2;
      float m[5][2] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};
#pragma unroll
      for (int k = 0; k < MS_K + 1; ++k) {
#pragma unroll
        for (int p = 0; p < 5; ++p) {
          const float v = hb[p][(ys + k) * MS_HP + x];
#pragma unroll
          for (int j = 0; j < 2; ++j)
            if (k - j >= 0 && k - j < MS_K) m[p][j] = fmaf(g.taps[k - j], v, m[p][j]);
        }
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        if (y0 + ys + j < g.oh && x0 + x < g.ow) {
          float s, c;
          ms_terms(m[0][j], m[1][j], m[2][j], m[3][j], m[4][j], g.mu_off, g.c1, g.c2, &s, &c);
          ssum += s;
          csum += c;
        }
      }
    }
    __syncthreads();
  }
  ssum = block_sum(ssum, red);
  csum = block_sum(csum, red + 4);
  if (tid == 0) {
    float* p = partial + (((int64_t)b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * 2;
    p[0] = ssum;
    p[1] = csum;
  }
}

struct MsReduce {
  int n, levels;
  int tiles[MS_MAXL];            // workgroups per image at each level
  int64_t offset[MS_MAXL];       // where the level's partials start, in floats
  float count[MS_MAXL];          // oh * ow * c: the size of the level's maps
};

// the ordered pass: one wave per (image, level) adds that image's tile sums in an order that depends on the tile count only
__global__ __launch_bounds__(64) void msssim_reduce_kernel(const float* __restrict__ partial, float* __restrict__ ssim,
                                                           float* __restrict__ cs, MsReduce g) {
  const int b = blockIdx.x, l = blockIdx.y, nt = g.tiles[l];
  const float* p = partial + g.offset[l] + (int64_t)b * nt * 2;
  float s = 0.f, c = 0.f;
  for (int t = threadIdx.x; t < nt; t += 64) {
    s += p[2 * t];
    c += p[2 * t + 1];
  }
  s = wave_sum(s);
  c = wave_sum(c);
  if (threadIdx.x == 0) {
    ssim[(int64_t)l * g.n + b] = s / g.count[l];
    cs[(int64_t)l * g.n + b] = c / g.count[l];
  }
}

struct MsFinal {
  int n, levels;
  float weights[MS_MAXL];
};

// msssim :165-171: clip at 0, prod_l cs_l^w_l (l < L - 1) * ssim_{L-1}^w_{L-1} per pair, then the mean over pairs
__global__ __launch_bounds__(256) void msssim_final_kernel(const float* __restrict__ ssim, const float* __restrict__ cs,
                                                           float* __restrict__ score, float* __restrict__ mean, MsFinal g) {
  __shared__ float red[4];
  float acc = 0.f;
  for (int b = threadIdx.x; b < g.n; b += 256) {
    float prod = 1.f;
    for (int l = 0; l < g.levels; ++l) {
      const float v = l == g.levels - 1 ? ssim[(int64_t)l * g.n + b] : cs[(int64_t)l * g.n + b];
      prod *= powf(fmaxf(v, 0.f), g.weights[l]);
    }
    score[b] = prod;
    acc += prod;
  }
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) *mean = acc / (float)g.n;
}

inline size_t ms_align(size_t v) { return (v + 15) & ~(size_t)15; }
inline int ms_tiles(int h, int w) { return ((h + MS_TH - 1) / MS_TH) * ((w + MS_TW - 1) / MS_TW); }

bool ms_shape_ok(int n, int h, int w, int c, int levels) {
  return n > 0 && n <= 65535 && h > 0 && w > 0 && c >= 1 && c <= MS_MAXC && levels >= 1 && levels <= MS_MAXL &&
         h % (1 << (levels - 1)) == 0 && w % (1 << (levels - 1)) == 0 && (int64_t)n * h * w * c < ((int64_t)1 << 40);
}

}  // namespace

extern "C" size_t tg_msssim_workspace_bytes(int n, int h, int w, int c, int levels) {
  if (!ms_shape_ok(n, h, w, c, levels)) return 0;
  size_t bytes = 0;
  for (int l = 0; l < levels; ++l) {
    const int hl = h >> l, wl = w >> l;
    if (l > 0) bytes += 2 * ms_align((size_t)n * hl * wl * c * sizeof(float));
    bytes += ms_align((size_t)n * ms_tiles(hl, wl) * 2 * sizeof(float));
  }
  return bytes;
}

extern "C" int tg_msssim(const void* img1, const void* img2, int n, int h, int w, int c, int dtype, float scale, float max_val,
                         float k1, float k2, const float* weights, int levels, float* score, float* ssim, float* cs, float* mean,
                         void* ws, size_t ws_bytes, void* stream) {
  static const float kDefault[5] = {0.0448f, 0.2856f, 0.3001f, 0.2363f, 0.1333f};
  TG_CHECK(img1 && img2 && score && ssim && cs && mean && ws, TG_EINVAL, "tg_msssim: null argument");
  TG_CHECK(n > 0 && h > 0 && w > 0 && c >= 1 && c <= MS_MAXC, TG_EINVAL, "tg_msssim: need n, h, w > 0 and 1 <= c <= %d (got %d, %d, %d, %d)",
           MS_MAXC, n, h, w, c);
  TG_CHECK(levels >= 1 && levels <= MS_MAXL, TG_EINVAL, "tg_msssim: levels 1..%d (got %d)", MS_MAXL, levels);
  TG_CHECK(weights || levels == 5, TG_EINVAL, "tg_msssim: the default weights are for 5 levels (got %d)", levels);
  TG_CHECK(h % (1 << (levels - 1)) == 0 && w % (1 << (levels - 1)) == 0, TG_EINVAL,
           "tg_msssim: h and w must be divisible by 2^(levels-1) = %d (got %d x %d)", 1 << (levels - 1), h, w);
  TG_CHECK(ms_shape_ok(n, h, w, c, levels), TG_EINVAL, "tg_msssim: at most 65535 pairs per call (got %d)", n);
  TG_CHECK(dtype == TG_F32 || dtype == TG_BF16 || dtype == TG_F16, TG_EINVAL, "tg_msssim: unsupported dtype %d", dtype);
  TG_CHECK(max_val > 0.f && scale > 0.f, TG_EINVAL, "tg_msssim: max_val and scale must be positive");
  TG_CHECK(ws_bytes >= tg_msssim_workspace_bytes(n, h, w, c, levels), TG_EINVAL, "tg_msssim: workspace too small");
  TG_CHECK(tg_aligned16(ws), TG_EALIGN, "tg_msssim: workspace must be 16-byte aligned");

  MsReduce rd;
  rd.n = n;
  rd.levels = levels;
  char* wp = (char*)ws;
  const void *in1 = img1, *in2 = img2;
  for (int l = 0; l < levels; ++l) {
    const int hl = h >> l, wl = w >> l;
    float *o1 = nullptr, *o2 = nullptr;
    if (l + 1 < levels) {
      const size_t plane = ms_align((size_t)n * (hl >> 1) * (wl >> 1) * c * sizeof(float));
      o1 = (float*)wp;
      o2 = (float*)(wp + plane);
      wp += 2 * plane;
    }
    float* partial = (float*)wp;
    rd.tiles[l] = ms_tiles(hl, wl);
    rd.offset[l] = (int64_t)(partial - (float*)ws);
    wp += ms_align((size_t)n * rd.tiles[l] * 2 * sizeof(float));

    MsLevel g;
    g.h = hl, g.w = wl, g.c = c;
    const int size = hl < wl ? (hl < MS_K ? hl : MS_K) : (wl < MS_K ? wl : MS_K);      // min(11, h, w)
    g.oh = hl - size + 1, g.ow = wl - size + 1;
    rd.count[l] = (float)g.oh * (float)g.ow * (float)c;
    g.scale = l == 0 ? scale : 1.f;
    g.off = l == 0 ? 0.5f * max_val : 0.f;
    g.mu_off = 0.5f * max_val;
    g.c1 = (k1 * max_val) * (k1 * max_val), g.c2 = (k2 * max_val) * (k2 * max_val);
    // _FSpecialGauss: the 2-D window is the outer product of this 1-D one with itself; even sizes sit on the half pixel
    const double sigma = size * 1.5 / 11.0, first = -(size / 2) + (size % 2 == 0 ? 0.5 : 0.0);
    double t[MS_K], sum = 0.0;
    for (int i = 0; i < size; ++i) {
      const double x = first + i;
      t[i] = exp(-(x * x) / (2.0 * sigma * sigma));
      sum += t[i];
    }
    for (int i = 0; i < MS_K; ++i) g.taps[i] = i < size ? (float)(t[i] / sum) : 0.f;

    const dim3 grid((wl + MS_TW - 1) / MS_TW, (hl + MS_TH - 1) / MS_TH, n);
    if (l == 0) {
      TG_DISPATCH_DTYPE(dtype, "tg_msssim", {
        hipLaunchKernelGGL((msssim_level_kernel<T>), grid, dim3(256), 0, (hipStream_t)stream, (const T*)in1, (const T*)in2, o1, o2,
                           partial, g);
      });
    } else {
      hipLaunchKernelGGL((msssim_level_kernel<float>), grid, dim3(256), 0, (hipStream_t)stream, (const float*)in1,
                         (const float*)in2, o1, o2, partial, g);
    }
    TG_LAUNCH_CHECK("tg_msssim");
    in1 = o1, in2 = o2;
  }
  hipLaunchKernelGGL(msssim_reduce_kernel, dim3(n, levels), dim3(64), 0, (hipStream_t)stream, (const float*)ws, ssim, cs, rd);
  TG_LAUNCH_CHECK("tg_msssim");
  MsFinal fg;
  fg.n = n;
  fg.levels = levels;
  for (int l = 0; l < MS_MAXL; ++l) fg.weights[l] = l < levels ? (weights ? weights[l] : kDefault[l]) : 0.f;
  hipLaunchKernelGGL(msssim_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)ssim, (const float*)cs, score,
                     mean, fg);
  TG_LAUNCH_CHECK("tg_msssim");
  return TG_OK;
}

// ---- sliced Wasserstein distance --------------------------------------------------------------------------------------------
// The evaluation the reference names but cannot run (image_generation.py:868-941 _calc_swd: one route raises :926-927, the other
// asserts :931 that TF 1.8 "is wrongly normalizing by patch"): section 5 of the PGGAN paper with the reference's parameters
// (:938: 128 patches per image, 4 x 128 directions; :912-916 resolutions hw, hw/2, ... >= 16; :910 the 1e3 scale).  Stages:
// Laplacian pyramid (two launches per level transition), descriptor gather, per-channel statistics (fp64, fixed partition)
// folded into the directions, projection to column-major sort keys, bitonic column sort, mean |difference|.
namespace {

enum { SW_C = 3, SW_P = 7, SW_K = SW_C * SW_P * SW_P, SW_T = 16, SW_IN = 2 * SW_T + 3, SW_ROWS = 64, SW_COLS = 32,
       SW_STAT_ROWS = 256, SW_MAD_ROWS = 4096, SW_SORT = 4096, SW_MAXHW = 512 };

// a pixel of the stored image as the metric sees it: float32(pixel) * scale, rounded to the uint8 grid with `quantize`
template <typename T, bool RAW>
__device__ __forceinline__ float sw_pixel(const T* p, float scale, int quantize) {
#pragma clang fp contract(off)
  float v = ld(p);
  if (RAW) {
    v = v * scale;
    if (quantize) v = fminf(fmaxf(rintf(v), 0.f), 255.f);
  }
  return v;
}

__device__ __forceinline__ int sw_mirror(int i, int s) { return i < 0 ? -i : (i >= s ? 2 * (s - 1) - i : i); }

// down(x): the 5 x 5 binomial filter with mirror boundary at the even positions.  One workgroup = a 16 x 16 tile of the coarse
// level of one image, from the 35 x 35 fine pixels under it staged in LDS (the coarse side is a power of two >= 16: no ragged tile).
template <typename T, bool RAW>
__global__ __launch_bounds__(256) void swd_down_kernel(const T* __restrict__ fine, float* __restrict__ coarse, int s, float scale,
                                                       int quantize) {
  __shared__ float tile[SW_IN * SW_IN * SW_C];
  const int tid = threadIdx.x, sc = s >> 1;
  const int oy0 = blockIdx.y * SW_T, ox0 = blockIdx.x * SW_T;
  const T* img = fine + (int64_t)blockIdx.z * s * s * SW_C;
#pragma unroll 5
  for (int i = tid; i < SW_IN * SW_IN * SW_C; i += 256) {
    const int r = i / (SW_IN * SW_C), e = i - r * (SW_IN * SW_C), cx = e / SW_C, ch = e - cx * SW_C;
    const int gy = sw_mirror(2 * oy0 - 2 + r, s), gx = sw_mirror(2 * ox0 - 2 + cx, s);
    tile[i] = sw_pixel<T, RAW>(img + ((int64_t)gy * s + gx) * SW_C + ch, scale, quantize);
  }
  __syncthreads();
  const int ty = tid >> 4, tx = tid & 15;
  const float g[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
  float acc[SW_C] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int dy = 0; dy < 5; ++dy) {
    float row[SW_C] = {0.f, 0.f, 0.f};
    const float* p = tile + ((2 * ty + dy) * SW_IN + 2 * tx) * SW_C;
#pragma unroll
    for (int dx = 0; dx < 5; ++dx)
#pragma unroll
      for (int ch = 0; ch < SW_C; ++ch) row[ch] = fmaf(g[dx], p[dx * SW_C + ch], row[ch]);
#pragma unroll
    for (int ch = 0; ch < SW_C; ++ch) acc[ch] = fmaf(g[dy], row[ch], acc[ch]);
  }
  float* o = coarse + (((int64_t)blockIdx.z * sc + oy0 + ty) * sc + ox0 + tx) * SW_C;
#pragma unroll
  for (int ch = 0; ch < SW_C; ++ch) o[ch] = acc[ch];
}

// up(x) along one axis in polyphase form: output o of 2h reads at most three coarse samples.  The mirror acts on the
// zero-inserted grid, so the low border reflects (sample -1 is sample 1) and the high border repeats sample h - 1.
__device__ __forceinline__ void sw_up_taps(int o, int h, int* idx, float* w) {
  const int i = o >> 1, hi = min(i + 1, h - 1);
  if (o & 1) {
    idx[0] = i, idx[1] = hi, idx[2] = i;
    w[0] = 0.5f, w[1] = 0.5f, w[2] = 0.f;
  } else {
    idx[0] = i == 0 ? 1 : i - 1, idx[1] = i, idx[2] = hi;
    w[0] = 0.125f, w[1] = 0.75f, w[2] = 0.125f;
  }
}

// lap = fine - up(coarse), one thread per fine pixel; coarse == nullptr: the level itself (a one-level pyramid).  `out` may be
// `fine` (levels >= 1 are rewritten in place: a thread reads only its own fine pixel).
template <typename T, bool RAW>
__global__ __launch_bounds__(256) void swd_lap_kernel(const T* fine, const float* __restrict__ coarse, float* out, int s,
                                                      int64_t pixels, float scale, int quantize) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= pixels) return;
  const int x = (int)(idx & (s - 1)), y = (int)((idx / s) & (s - 1)), h = s >> 1;
  const int64_t b = idx / ((int64_t)s * s);
  float v[SW_C], u[SW_C] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int ch = 0; ch < SW_C; ++ch) v[ch] = sw_pixel<T, RAW>(fine + idx * SW_C + ch, scale, quantize);
  if (coarse) {
    int iy[3], ix[3];
    float wy[3], wx[3];
    sw_up_taps(y, h, iy, wy);
    sw_up_taps(x, h, ix, wx);
    const float* cimg = coarse + b * h * h * SW_C;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      float row[SW_C] = {0.f, 0.f, 0.f};
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        const float* p = cimg + ((int64_t)iy[a] * h + ix[q]) * SW_C;
#pragma unroll
        for (int ch = 0; ch < SW_C; ++ch) row[ch] = fmaf(wx[q], p[ch], row[ch]);
      }
#pragma unroll
      for (int ch = 0; ch < SW_C; ++ch) u[ch] = fmaf(wy[a], row[ch], u[ch]);
    }
  }
#pragma unroll
  for (int ch = 0; ch < SW_C; ++ch) out[idx * SW_C + ch] = v[ch] - u[ch];
}

// rows [N, 147] of 7 x 7 x 3 neighbourhoods, k = c * 49 + dy * 7 + dx; one thread per output value, so a row is one contiguous
// 588-byte write.  The host checked the centres; the clamp only keeps a corrupted table inside the image.
__global__ __launch_bounds__(256) void swd_desc_kernel(const float* __restrict__ level, const int* __restrict__ centres,
                                                       float* __restrict__ out, int s, int per, int64_t total) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int64_t row = idx / SW_K;
  const int k = (int)(idx - row * SW_K), ch = k / (SW_P * SW_P), r = k - ch * (SW_P * SW_P), dy = r / SW_P, dx = r - dy * SW_P;
  const int cy = min(max(centres[2 * row], 3), s - 4), cx = min(max(centres[2 * row + 1], 3), s - 4);
  out[idx] = level[(((row / per) * s + cy - 3 + dy) * s + cx - 3 + dx) * SW_C + ch];
}

// block-wide sum in double; the result is valid in every thread.  red: __shared__ double[>= blockDim / 64]
__device__ __forceinline__ double sw_block_sum(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
  __syncthreads();
  if (lane == 0) red[wid] = v;
  __syncthreads();
  double r = 0.0;
  for (int i = 0; i < nw; ++i) r += red[i];
  return r;
}

// statistics, stage 1: per channel sum and sum of squares of (x - x0[c]) over a FIXED chunk of 256 rows, in double (x0 = the
// set's first value of the channel: a flat channel sums exact zeros, and the squares stay small next to a large DC offset).
// The partition depends on N alone, never on the launch.
__global__ __launch_bounds__(256) void swd_stats_kernel(const float* __restrict__ desc, double* __restrict__ partial, int64_t N) {
  __shared__ double red[4];
  const int64_t r0 = (int64_t)blockIdx.x * SW_STAT_ROWS;
  const int n = (int)(N - r0 < SW_STAT_ROWS ? N - r0 : SW_STAT_ROWS) * SW_K;
  const float x0[SW_C] = {desc[0], desc[SW_P * SW_P], desc[2 * SW_P * SW_P]};
  double s1[SW_C] = {0.0, 0.0, 0.0}, s2[SW_C] = {0.0, 0.0, 0.0};
  const float* p = desc + r0 * SW_K;
  for (int e = threadIdx.x; e < n; e += 256) {
    const int ch = (e % SW_K) / (SW_P * SW_P);
    const double d = (double)p[e] - (double)x0[ch];
    s1[ch] += d;
    s2[ch] += d * d;
  }
  for (int ch = 0; ch < SW_C; ++ch) {
    const double a = sw_block_sum(s1[ch], red), q = sw_block_sum(s2[ch], red);
    if (threadIdx.x == 0) {
      partial[blockIdx.x * 6 + ch] = a;
      partial[blockIdx.x * 6 + 3 + ch] = q;
    }
  }
}

// statistics, stage 2, and the fold: every workgroup adds the chunk sums in the same fixed order, then a thread per column
// writes dirs'[k][col] = dirs[r][k][d] * rstd[c(k)] and the column's offset.  The projection subtracts the fp32 mean while it
// stages a row (so no large products cancel); the offset carries what that rounding of the mean left: (mean - fp32(mean)) . dirs'.
__global__ __launch_bounds__(256) void swd_fold_kernel(const float* __restrict__ desc, const double* __restrict__ partial,
                                                       const float* __restrict__ dirs, float* __restrict__ dirs2,
                                                       float* __restrict__ off, float* __restrict__ statf, float* __restrict__ stats_out,
                                                       int64_t N, int nparts, int R, int D) {
  __shared__ double red[4];
  double mean[SW_C], rstd[SW_C];
  for (int ch = 0; ch < SW_C; ++ch) {
    double a = 0.0, q = 0.0;
    for (int i = threadIdx.x; i < nparts; i += 256) {
      a += partial[i * 6 + ch];
      q += partial[i * 6 + 3 + ch];
    }
    a = sw_block_sum(a, red);
    q = sw_block_sum(q, red);
    const double m = (double)N * (SW_P * SW_P), d = a / m, var = q / m - d * d;
    mean[ch] = (double)desc[ch * SW_P * SW_P] + d;
    rstd[ch] = var > 0.0 ? 1.0 / sqrt(var) : 0.0;      // sigma = 0: the channel's normalised values are 0
  }
  if (blockIdx.x == 0 && threadIdx.x < SW_C) {
    const int ch = threadIdx.x;
    statf[ch] = (float)mean[ch];
    statf[3 + ch] = (float)rstd[ch];
    if (stats_out) {
      stats_out[ch] = (float)mean[ch];
      stats_out[3 + ch] = (float)rstd[ch];
    }
  }
  const int RD = R * D, col = blockIdx.x * 256 + threadIdx.x;
  if (col >= RD) return;
  const int r = col / D, d = col - r * D;
  double o = 0.0;
  for (int k = 0; k < SW_K; ++k) {
    const int ch = k / (SW_P * SW_P);
    const float w = (float)((double)dirs[((int64_t)r * SW_K + k) * D + d] * rstd[ch]);
    dirs2[(int64_t)k * RD + col] = w;
    o += (mean[ch] - (double)(float)mean[ch]) * (double)w;
  }
  off[col] = (float)o;
}

// proj[col][row] = sum_k (desc[row][k] - mean[c(k)]) * dirs'[k][col] - off[col], column-major [R D][Npad] so that a sort key
// stream is contiguous; rows N .. Npad - 1 are +inf.  One workgroup stages 64 centred rows in LDS once and walks all R D
// columns in chunks of 32 (lane = row: stride 147 floats is odd, no bank conflict; a wave shares its 8 directions: broadcast reads).
__global__ __launch_bounds__(256) void swd_project_kernel(const float* __restrict__ desc, const float* __restrict__ dirs2,
                                                          const float* __restrict__ off, const float* __restrict__ statf,
                                                          float* __restrict__ proj, int64_t N, int64_t Npad, int RD) {
  __shared__ float rows[SW_ROWS * SW_K];
  __shared__ __attribute__((aligned(16))) float dch[SW_K * SW_COLS];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t r0 = (int64_t)blockIdx.x * SW_ROWS;
  const float m[SW_C] = {statf[0], statf[1], statf[2]};
#pragma unroll 4
  for (int i = tid; i < SW_ROWS * SW_K; i += 256) {
    const int row = i / SW_K, k = i - row * SW_K;
    rows[i] = r0 + row < N ? desc[(r0 + row) * SW_K + k] - m[k / (SW_P * SW_P)] : 0.f;
  }
  const int64_t gr = r0 + lane;
  for (int c0 = 0; c0 < RD; c0 += SW_COLS) {
    __syncthreads();
    for (int i = tid; i < SW_K * SW_COLS; i += 256) {
      const int k = i / SW_COLS, j = i - k * SW_COLS;
      dch[i] = c0 + j < RD ? dirs2[(int64_t)k * RD + c0 + j] : 0.f;
    }
    __syncthreads();
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const float* a = rows + lane * SW_K;
    const float* d = dch + wv * 8;
#pragma unroll 7
    for (int k = 0; k < SW_K; ++k) {
      const float av = a[k];
      const f32x4 d0 = *reinterpret_cast<const f32x4*>(d + k * SW_COLS), d1 = *reinterpret_cast<const f32x4*>(d + k * SW_COLS + 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        acc[j] = fmaf(av, d0[j], acc[j]);
        acc[4 + j] = fmaf(av, d1[j], acc[4 + j]);
      }
    }
    if (gr < Npad) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int col = c0 + wv * 8 + j;
        if (col < RD) proj[(int64_t)col * Npad + gr] = gr < N ? acc[j] - off[col] : INFINITY;
      }
    }
  }
}

__device__ __forceinline__ void sw_cmpx(float& a, float& b, bool up) {
  if (up ? a > b : a < b) {
    const float t = a;
    a = b;
    b = t;
  }
}

// Bitonic network over a column of Npad = 2^m keys.  One workgroup holds `nloc` = min(SW_SORT, Npad) keys in LDS.  FULL: every
// merge up to nloc (the start of the sort).  Otherwise the steps j = nloc / 2 .. 1 of the merge of size k, whose steps
// j >= nloc ran as global passes.  The direction of a compare-exchange comes from the key's index in the whole column.
template <bool FULL>
__global__ __launch_bounds__(256) void swd_sort_local_kernel(float* __restrict__ keys, int64_t Npad, int nloc, int64_t kmerge) {
  __shared__ float sk[SW_SORT];
  const int tid = threadIdx.x;
  const int64_t g0 = (int64_t)blockIdx.x * nloc;
  float* base = keys + (int64_t)blockIdx.y * Npad + g0;
  for (int i = tid; i < nloc; i += 256) sk[i] = base[i];
  __syncthreads();
  for (int64_t k = FULL ? 2 : kmerge; k <= (FULL ? (int64_t)nloc : kmerge); k <<= 1) {
    for (int j = k >> 1 < nloc >> 1 ? (int)(k >> 1) : nloc >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < (nloc >> 1); t += 256) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        sw_cmpx(sk[i], sk[i + j], ((g0 + i) & k) == 0);
      }
      __syncthreads();
    }
  }
  for (int i = tid; i < nloc; i += 256) base[i] = sk[i];
}

// one step j >= SW_SORT of the merge of size k, in global memory: a thread owns four adjacent pairs (i, i + j)
__global__ __launch_bounds__(256) void swd_sort_global_kernel(float* __restrict__ keys, int64_t Npad, int64_t k, int64_t j) {
  const int64_t t = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (t >= (Npad >> 1)) return;
  const int64_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
  float* base = keys + (int64_t)blockIdx.y * Npad;
  f32x4 a = *reinterpret_cast<const f32x4*>(base + i), b = *reinterpret_cast<const f32x4*>(base + i + j);
  const bool up = (i & k) == 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    float x = a[q], y = b[q];
    sw_cmpx(x, y, up);
    a[q] = x, b[q] = y;
  }
  *reinterpret_cast<f32x4*>(base + i) = a;
  *reinterpret_cast<f32x4*>(base + i + j) = b;
}

// mean |a - b|, stage 1: one workgroup per (fixed chunk of 4096 rows, column), in double
__global__ __launch_bounds__(256) void swd_mad_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                      double* __restrict__ partial, int64_t N, int64_t Npad) {
  __shared__ double red[4];
  const int64_t r0 = (int64_t)blockIdx.x * SW_MAD_ROWS, o = (int64_t)blockIdx.y * Npad;
  const int n = (int)(N - r0 < SW_MAD_ROWS ? N - r0 : SW_MAD_ROWS);
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) s += (double)fabsf(a[o + r0 + i] - b[o + r0 + i]);
  s = sw_block_sum(s, red);
  if (threadIdx.x == 0) partial[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = s;
}

// stage 2: the chunk sums of a repeat's D columns in a fixed order -> out[r]; out[R] = the mean over the repeats
__global__ __launch_bounds__(256) void swd_mad_final_kernel(const double* __restrict__ partial, float* __restrict__ out, int64_t N,
                                                            int nchunks, int R, int D) {
  __shared__ double red[4];
  double total = 0.0;
  for (int r = 0; r < R; ++r) {
    const double* p = partial + (int64_t)r * D * nchunks;
    double s = 0.0;
    for (int i = threadIdx.x; i < D * nchunks; i += 256) s += p[i];
    s = sw_block_sum(s, red) / ((double)N * (double)D);
    total += s;
    if (threadIdx.x == 0) out[r] = (float)s;
  }
  if (threadIdx.x == 0) out[R] = (float)(total / (double)R);
}

inline bool sw_pow2(int64_t v) { return v > 0 && (v & (v - 1)) == 0; }
inline bool sw_hw_ok(int hw) { return hw >= 16 && hw <= SW_MAXHW && sw_pow2(hw); }
inline int64_t sw_npad(int64_t n) {
  int64_t p = 1;
  while (p < n) p <<= 1;
  return p;
}
inline bool sw_count_ok(int64_t n, int r, int d) {
  return n > 0 && n <= ((int64_t)1 << 24) && r > 0 && d > 0 && (int64_t)r * d <= 65535;
}
inline size_t sw_project_parts(int64_t n) { return (size_t)((n + SW_STAT_ROWS - 1) / SW_STAT_ROWS); }
inline size_t sw_mad_chunks(int64_t n) { return (size_t)((n + SW_MAD_ROWS - 1) / SW_MAD_ROWS); }

}  // namespace

extern "C" int tg_swd_sort_block(void) { return SW_SORT; }

extern "C" size_t tg_swd_pyramid_workspace_bytes(int n, int hw) {
  if (n <= 0 || n > 65535 || !sw_hw_ok(hw)) return 0;
  size_t bytes = 0;
  for (int s = hw; s >= 16; s >>= 1) bytes += (size_t)n * s * s * SW_C * sizeof(float);
  return bytes;
}

extern "C" int tg_swd_pyramid(const void* x, int n, int hw, int c, int dtype, float scale, int quantize, void* ws, size_t ws_bytes,
                              void* stream) {
  TG_CHECK(x && ws, TG_EINVAL, "tg_swd_pyramid: null argument");
  TG_CHECK(sw_hw_ok(hw), TG_EINVAL, "tg_swd_pyramid: hw must be a power of two in 16..%d (got %d; the reference refuses < 16)",
           SW_MAXHW, hw);
  TG_CHECK(c == SW_C, TG_EINVAL, "tg_swd_pyramid: descriptors are 7 x 7 x 3: need c = 3 (got %d)", c);
  TG_CHECK(n > 0 && n <= 65535, TG_EINVAL, "tg_swd_pyramid: 1..65535 images per call (got %d)", n);
  TG_CHECK(dtype == TG_F32 || dtype == TG_BF16 || dtype == TG_F16, TG_EINVAL, "tg_swd_pyramid: unsupported dtype %d", dtype);
  TG_CHECK(ws_bytes >= tg_swd_pyramid_workspace_bytes(n, hw), TG_EINVAL, "tg_swd_pyramid: pyramid storage too small");
  TG_CHECK(tg_aligned16(ws), TG_EALIGN, "tg_swd_pyramid: pyramid storage must be 16-byte aligned");
  hipStream_t st_ = (hipStream_t)stream;
  float* lvl = (float*)ws;
  const int64_t px0 = (int64_t)n * hw * hw;
  float* next = lvl + px0 * SW_C;
  if (hw >= 32) {      // level 1 from the stored image, then level 0 = image - up(level 1)
    const dim3 grid(hw / 2 / SW_T, hw / 2 / SW_T, n);
    TG_DISPATCH_DTYPE(dtype, "tg_swd_pyramid", {
      hipLaunchKernelGGL((swd_down_kernel<T, true>), grid, dim3(256), 0, st_, (const T*)x, next, hw, scale, quantize);
    });
    TG_LAUNCH_CHECK("tg_swd_pyramid");
  }
  TG_DISPATCH_DTYPE(dtype, "tg_swd_pyramid", {
    hipLaunchKernelGGL((swd_lap_kernel<T, true>), dim3((unsigned)((px0 + 255) / 256)), dim3(256), 0, st_, (const T*)x,
                       hw >= 32 ? (const float*)next : (const float*)nullptr, lvl, hw, px0, scale, quantize);
  });
  TG_LAUNCH_CHECK("tg_swd_pyramid");
  for (int s = hw / 2; s >= 32; s >>= 1) {
    lvl = next;
    const int64_t px = (int64_t)n * s * s;
    next = lvl + px * SW_C;
    hipLaunchKernelGGL((swd_down_kernel<float, false>), dim3(s / 2 / SW_T, s / 2 / SW_T, n), dim3(256), 0, st_, (const float*)lvl,
                       next, s, 1.f, 0);
    TG_LAUNCH_CHECK("tg_swd_pyramid");
    hipLaunchKernelGGL((swd_lap_kernel<float, false>), dim3((unsigned)((px + 255) / 256)), dim3(256), 0, st_, (const float*)lvl,
                       (const float*)next, lvl, s, px, 1.f, 0);
    TG_LAUNCH_CHECK("tg_swd_pyramid");
  }
  return TG_OK;
}

extern "C" int tg_swd_descriptors(const float* level, const int* centres, int n, int s, int per, float* out, int64_t row_offset,
                                  int64_t out_rows, void* stream) {
  TG_CHECK(level && centres && out, TG_EINVAL, "tg_swd_descriptors: null argument");
  TG_CHECK(sw_hw_ok(s), TG_EINVAL, "tg_swd_descriptors: level side must be a power of two in 16..%d (got %d)", SW_MAXHW, s);
  TG_CHECK(n > 0 && per > 0 && (int64_t)n * per <= ((int64_t)1 << 24), TG_EINVAL,
           "tg_swd_descriptors: need n, per > 0 and n * per <= 2^24 (got %d, %d)", n, per);
  TG_CHECK(row_offset >= 0 && row_offset + (int64_t)n * per <= out_rows, TG_EINVAL,
           "tg_swd_descriptors: rows %lld..%lld do not fit a buffer of %lld rows", (long long)row_offset,
           (long long)(row_offset + (int64_t)n * per), (long long)out_rows);
  const int64_t total = (int64_t)n * per * SW_K;
  hipLaunchKernelGGL(swd_desc_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, level, centres,
                     out + row_offset * SW_K, s, per, total);
  TG_LAUNCH_CHECK("tg_swd_descriptors");
  return TG_OK;
}

extern "C" size_t tg_swd_project_workspace_bytes(int64_t n, int repeats, int dirs) {
  if (!sw_count_ok(n, repeats, dirs)) return 0;
  const size_t rd = (size_t)repeats * dirs;
  return ms_align(sw_project_parts(n) * 6 * sizeof(double)) + ms_align(SW_K * rd * sizeof(float)) + ms_align(rd * sizeof(float)) +
         ms_align(8 * sizeof(float));
}

extern "C" int tg_swd_project(const float* desc, const float* dirs, int64_t n, int repeats, int dirs_per, float* proj, float* stats,
                              void* ws, size_t ws_bytes, void* stream) {
  TG_CHECK(desc && dirs && proj && ws, TG_EINVAL, "tg_swd_project: null argument");
  TG_CHECK(sw_count_ok(n, repeats, dirs_per), TG_EINVAL,
           "tg_swd_project: need 1 <= N <= 2^24 rows and 1 <= repeats * dirs <= 65535 (got %lld, %d x %d)", (long long)n, repeats,
           dirs_per);
  TG_CHECK(ws_bytes >= tg_swd_project_workspace_bytes(n, repeats, dirs_per), TG_EINVAL, "tg_swd_project: workspace too small");
  TG_CHECK(tg_aligned16(ws), TG_EALIGN, "tg_swd_project: workspace must be 16-byte aligned");
  hipStream_t st_ = (hipStream_t)stream;
  const int rd = repeats * dirs_per, parts = (int)sw_project_parts(n);
  const int64_t npad = sw_npad(n);
  char* wp = (char*)ws;
  double* partial = (double*)wp;
  wp += ms_align((size_t)parts * 6 * sizeof(double));
  float* dirs2 = (float*)wp;
  wp += ms_align((size_t)SW_K * rd * sizeof(float));
  float* off = (float*)wp;
  wp += ms_align((size_t)rd * sizeof(float));
  float* statf = (float*)wp;
  hipLaunchKernelGGL(swd_stats_kernel, dim3(parts), dim3(256), 0, st_, desc, partial, n);
  TG_LAUNCH_CHECK("tg_swd_project");
  hipLaunchKernelGGL(swd_fold_kernel, dim3((rd + 255) / 256), dim3(256), 0, st_, desc, (const double*)partial, dirs, dirs2, off, statf,
                     stats, n, parts, repeats, dirs_per);
  TG_LAUNCH_CHECK("tg_swd_project");
  hipLaunchKernelGGL(swd_project_kernel, dim3((unsigned)((npad + SW_ROWS - 1) / SW_ROWS)), dim3(256), 0, st_, desc,
                     (const float*)dirs2, (const float*)off, (const float*)statf, proj, n, npad, rd);
  TG_LAUNCH_CHECK("tg_swd_project");
  return TG_OK;
}

extern "C" int tg_swd_sort_columns(float* keys, int cols, int64_t npad, void* stream) {
  TG_CHECK(keys, TG_EINVAL, "tg_swd_sort_columns: null argument");
  TG_CHECK(cols > 0 && cols <= 65535 && sw_pow2(npad) && npad <= ((int64_t)1 << 24), TG_EINVAL,
           "tg_swd_sort_columns: need 1..65535 columns of a power-of-two length <= 2^24 (got %d x %lld)", cols, (long long)npad);
  TG_CHECK(npad < 4 || tg_aligned16(keys), TG_EALIGN, "tg_swd_sort_columns: keys must be 16-byte aligned");
  hipStream_t st_ = (hipStream_t)stream;
  const int nloc = (int)(npad < SW_SORT ? npad : SW_SORT);
  const dim3 lgrid((unsigned)(npad / nloc), cols);
  hipLaunchKernelGGL((swd_sort_local_kernel<true>), lgrid, dim3(256), 0, st_, keys, npad, nloc, (int64_t)0);
  TG_LAUNCH_CHECK("tg_swd_sort_columns");
  for (int64_t k = 2 * (int64_t)SW_SORT; k <= npad; k <<= 1) {
    for (int64_t j = k >> 1; j >= SW_SORT; j >>= 1) {
      hipLaunchKernelGGL(swd_sort_global_kernel, dim3((unsigned)(npad / 2 / 4 / 256), cols), dim3(256), 0, st_, keys, npad, k, j);
      TG_LAUNCH_CHECK("tg_swd_sort_columns");
    }
    hipLaunchKernelGGL((swd_sort_local_kernel<false>), lgrid, dim3(256), 0, st_, keys, npad, nloc, k);
    TG_LAUNCH_CHECK("tg_swd_sort_columns");
  }
  return TG_OK;
}

extern "C" size_t tg_swd_mean_abs_diff_workspace_bytes(int64_t n, int repeats, int dirs) {
  if (!sw_count_ok(n, repeats, dirs)) return 0;
  return ms_align(sw_mad_chunks(n) * (size_t)repeats * dirs * sizeof(double));
}

extern "C" int tg_swd_mean_abs_diff(const float* a, const float* b, int64_t n, int64_t npad, int repeats, int dirs, float* out,
                                    void* ws, size_t ws_bytes, void* stream) {
  TG_CHECK(a && b && out && ws, TG_EINVAL, "tg_swd_mean_abs_diff: null argument");
  TG_CHECK(sw_count_ok(n, repeats, dirs) && npad >= n, TG_EINVAL,
           "tg_swd_mean_abs_diff: need 1 <= N <= Npad, N <= 2^24 and 1 <= repeats * dirs <= 65535 (got %lld, %lld, %d x %d)",
           (long long)n, (long long)npad, repeats, dirs);
  TG_CHECK(ws_bytes >= tg_swd_mean_abs_diff_workspace_bytes(n, repeats, dirs), TG_EINVAL, "tg_swd_mean_abs_diff: workspace too small");
  TG_CHECK(tg_aligned16(ws), TG_EALIGN, "tg_swd_mean_abs_diff: workspace must be 16-byte aligned");
  const int chunks = (int)sw_mad_chunks(n);
  hipLaunchKernelGGL(swd_mad_kernel, dim3(chunks, repeats * dirs), dim3(256), 0, (hipStream_t)stream, a, b, (double*)ws, n, npad);
  TG_LAUNCH_CHECK("tg_swd_mean_abs_diff");
  hipLaunchKernelGGL(swd_mad_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)ws, out, n, chunks, repeats,
                     dirs);
  TG_LAUNCH_CHECK("tg_swd_mean_abs_diff");
  return TG_OK;
}

extern "C" size_t tg_swd_distance_workspace_bytes(int64_t n, int repeats, int dirs) {
  if (!sw_count_ok(n, repeats, dirs)) return 0;
  const size_t keys = ms_align((size_t)repeats * dirs * (size_t)sw_npad(n) * sizeof(float));
  const size_t pw = tg_swd_project_workspace_bytes(n, repeats, dirs), mw = tg_swd_mean_abs_diff_workspace_bytes(n, repeats, dirs);
  return 2 * keys + (pw > mw ? pw : mw);
}

extern "C" int tg_swd_distance(const float* desc_a, int64_t n_a, const float* desc_b, int64_t n_b, const float* dirs, int repeats,
                               int dirs_per, float* out, float* stats, void* ws, size_t ws_bytes, void* stream) {
  TG_CHECK(desc_a && desc_b && dirs && out && ws, TG_EINVAL, "tg_swd_distance: null argument");
  TG_CHECK(n_a == n_b, TG_EINVAL, "tg_swd_distance: both sets must hold the same number of descriptors (got %lld and %lld)",
           (long long)n_a, (long long)n_b);
  TG_CHECK(sw_count_ok(n_a, repeats, dirs_per), TG_EINVAL,
           "tg_swd_distance: need 1 <= N <= 2^24 rows and 1 <= repeats * dirs <= 65535 (got %lld, %d x %d)", (long long)n_a, repeats,
           dirs_per);
  TG_CHECK(ws_bytes >= tg_swd_distance_workspace_bytes(n_a, repeats, dirs_per), TG_EINVAL, "tg_swd_distance: workspace too small");
  TG_CHECK(tg_aligned16(ws), TG_EALIGN, "tg_swd_distance: workspace must be 16-byte aligned");
  const int rd = repeats * dirs_per;
  const int64_t npad = sw_npad(n_a);
  const size_t keys = ms_align((size_t)rd * (size_t)npad * sizeof(float));
  float *pa = (float*)ws, *pb = (float*)((char*)ws + keys);
  void* rest = (char*)ws + 2 * keys;
  const size_t rest_bytes = ws_bytes - 2 * keys;
  int rc = tg_swd_project(desc_a, dirs, n_a, repeats, dirs_per, pa, stats, rest, rest_bytes, stream);
  if (rc != TG_OK) return rc;
  rc = tg_swd_project(desc_b, dirs, n_b, repeats, dirs_per, pb, stats ? stats + 6 : nullptr, rest, rest_bytes, stream);
  if (rc != TG_OK) return rc;
  rc = tg_swd_sort_columns(pa, rd, npad, stream);
  if (rc != TG_OK) return rc;
  rc = tg_swd_sort_columns(pb, rd, npad, stream);
  if (rc != TG_OK) return rc;
  return tg_swd_mean_abs_diff(pa, pb, n_a, npad, repeats, dirs_per, out, rest, rest_bytes, stream);
}

// ---- sample grids (include/twingan_hip_summary.h tg_image_grid_u8) ---------------------------------------------------------
// One thread per grid pixel: it finds the job of its column slot, reads the pixel's c values and stores three bytes; a pixel
// of a cell no job fills stores zeros, so the launch writes every byte of the grid once and needs no clear.
namespace {
struct GridJob {
  const void* src;
  int dtype, n, c, col;
};

// clip(trunc(x * 255), 0, 255): !(f > 0) takes NaN, -inf and every product that truncates to <= 0
__device__ __forceinline__ unsigned char grid_byte(float x) {
  const float f = x * 255.0f;
  if (!(f > 0.f)) return 0;
  return f >= 255.f ? (unsigned char)255 : (unsigned char)(int)f;
}

template <typename T>
__device__ __forceinline__ void grid_pixel(const GridJob& j, int64_t pix, unsigned char* dst) {
  const T* p = (const T*)j.src + pix * j.c;
  const unsigned char r = grid_byte(ld<T>(p));
  dst[0] = r;
  dst[1] = j.c == 3 ? grid_byte(ld<T>(p + 1)) : r;
  dst[2] = j.c == 3 ? grid_byte(ld<T>(p + 2)) : r;
}

__global__ __launch_bounds__(256) void image_grid_kernel(const GridJob* __restrict__ jobs, int njobs, int rows, int cols, int h, int w,
                                                         unsigned char* __restrict__ grid) {
  const int total = rows * h * cols * w;      // < 2^31: checked by the entry point
  // the stride is added in 64 bits: the last trip of a grid near 2^31 pixels must not wrap
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < total; p += (int64_t)gridDim.x * 256) {
    const int pix = (int)p;
    const int y = pix / (cols * w), x = pix - y * (cols * w);
    const int r = y / h, iy = y - r * h, cs = x / w, ix = x - cs * w;
    unsigned char* dst = grid + (int64_t)pix * 3;
    int k = 0;
    while (k < njobs && !(jobs[k].col == cs && r < jobs[k].n)) ++k;
    if (k == njobs) {
      dst[0] = dst[1] = dst[2] = 0;
      continue;
    }
    const GridJob j = jobs[k];
    const int64_t src_pix = ((int64_t)r * h + iy) * w + ix;
    if (j.dtype == TG_F32) grid_pixel<float>(j, src_pix, dst);
    else if (j.dtype == TG_BF16) grid_pixel<bf16>(j, src_pix, dst);
    else grid_pixel<f16>(j, src_pix, dst);
  }
}
}  // namespace

extern "C" size_t tg_image_grid_table_bytes(int njobs) { return (size_t)(njobs > 0 ? njobs : 0) * sizeof(GridJob); }

extern "C" int tg_image_grid_table_fill(const void* src, int dtype, int n, int c, int col, int job, void* table_host) {
  TG_CHECK(src, TG_EINVAL, "tg_image_grid_table_fill: src is null");
  TG_CHECK(table_host, TG_EINVAL, "tg_image_grid_table_fill: table_host is null");
  TG_CHECK(dtype == TG_F32 || dtype == TG_BF16 || dtype == TG_F16, TG_EINVAL, "tg_image_grid_table_fill: unsupported dtype %d", dtype);
  TG_CHECK(n >= 1, TG_EINVAL, "tg_image_grid_table_fill: n must be positive (got %d)", n);
  TG_CHECK(c == 1 || c == 3, TG_EINVAL, "tg_image_grid_table_fill: c must be 1 or 3 (got %d)", c);
  TG_CHECK(col >= 0, TG_EINVAL, "tg_image_grid_table_fill: col must not be negative (got %d)", col);
  TG_CHECK(job >= 0, TG_EINVAL, "tg_image_grid_table_fill: job must not be negative (got %d)", job);
  ((GridJob*)table_host)[job] = GridJob{src, dtype, n, c, col};
  return TG_OK;
}

extern "C" int tg_image_grid_u8(const void* table_device, int njobs, int rows, int cols, int h, int w, uint8_t* grid, void* stream) {
  TG_CHECK(table_device, TG_EINVAL, "tg_image_grid_u8: table_device is null");
  TG_CHECK(grid, TG_EINVAL, "tg_image_grid_u8: grid is null");
  TG_CHECK(njobs >= 1, TG_EINVAL, "tg_image_grid_u8: njobs must be positive (got %d)", njobs);
  TG_CHECK(rows >= 1 && cols >= 1, TG_EINVAL, "tg_image_grid_u8: rows and cols must be positive (got %d, %d)", rows, cols);
  TG_CHECK(h >= 1 && w >= 1, TG_EINVAL, "tg_image_grid_u8: h and w must be positive (got %d, %d)", h, w);
  const int64_t total = (int64_t)rows * h * cols * w;
  TG_CHECK(total < (1ll << 31), TG_EINVAL, "tg_image_grid_u8: rows * h * cols * w = %lld pixels, the limit is 2^31 - 1", (long long)total);
  hipLaunchKernelGGL(image_grid_kernel, dim3(tg_grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream, (const GridJob*)table_device,
                     njobs, rows, cols, h, w, grid);
  TG_LAUNCH_CHECK("tg_image_grid_u8");
  return TG_OK;
}
