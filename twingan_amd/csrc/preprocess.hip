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
