"""TEST INFRASTRUCTURE for the MS-SSIM kernel (never imported by the product): a NumPy restatement of the formulas of the
reference's libs/ms_ssim.py (msssim :115-171, _SSIMForMultiScale :39-110, _HoxDownsample :112, _FSpecialGauss :27-37) that
runs in float64 or, as its twin, in float32 throughout; the seeded input families of the parity tests; and the case table
shared by tools/make_msssim_golden.py (which records the reference's own results into tests/golden/msssim_cases.npz),
tests/test_msssim_cpu.py and tests/test_gpu_metrics.py."""
import os
import zlib

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'msssim_cases.npz')
WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


# ---- the formulas ------------------------------------------------------------------------------------------------------------
def window_1d(size, sigma):
  """The 1-D Gaussian whose outer product with itself is the reference's 2-D window (normalised to sum 1): positions
  -size//2 .. size//2, shifted onto the half pixel for even sizes."""
  x = np.arange(size, dtype=np.float64) - (size // 2) + (0.5 if size % 2 == 0 else 0.0)
  g = np.exp(-(x * x) / (2.0 * sigma * sigma))
  return g / g.sum()


def _valid_filter(x, taps):
  """'valid' windowed sum along H then W of [B, H, W, C] in x's dtype (the window is symmetric: correlation = convolution)."""
  k = len(taps)
  oh, ow = x.shape[1] - k + 1, x.shape[2] - k + 1
  rows = np.zeros((x.shape[0], oh, x.shape[2], x.shape[3]), x.dtype)
  for i in range(k):
    rows += taps[i] * x[:, i:i + oh]
  out = np.zeros((x.shape[0], oh, ow, x.shape[3]), x.dtype)
  for i in range(k):
    out += taps[i] * rows[:, :, i:i + ow]
  return out


def ssim_level(x1, x2, max_val=255., k1=0.01, k2=0.03, filter_size=11, filter_sigma=1.5):
  """-> (ssim[B], cs[B]): the per-image means of the ssim and cs maps of one level, in the dtype of x1."""
  dt = x1.dtype.type
  size = min(filter_size, x1.shape[1], x1.shape[2])
  taps = window_1d(size, size * filter_sigma / filter_size).astype(dt)
  mu1, mu2 = _valid_filter(x1, taps), _valid_filter(x2, taps)
  s11 = _valid_filter(x1 * x1, taps) - mu1 * mu1
  s22 = _valid_filter(x2 * x2, taps) - mu2 * mu2
  s12 = _valid_filter(x1 * x2, taps) - mu1 * mu2
  c1, c2 = dt((k1 * max_val) ** 2), dt((k2 * max_val) ** 2)
  v1 = dt(2.0) * s12 + c2
  v2 = s11 + s22 + c2
  ssim = ((dt(2.0) * mu1 * mu2 + c1) * v1) / ((mu1 * mu1 + mu2 * mu2 + c1) * v2)
  return ssim.mean(axis=(1, 2, 3), dtype=dt), (v1 / v2).mean(axis=(1, 2, 3), dtype=dt)


def downsample(x):
  return (x[:, 0::2, 0::2] + x[:, 1::2, 0::2] + x[:, 0::2, 1::2] + x[:, 1::2, 1::2]) * x.dtype.type(0.25)


def score_from_tables(ssim, cs, weights):
  """msssim :165-171 per pair: clip both tables at 0, prod_l cs_l^w_l (l < L-1) * ssim_{L-1}^w_{L-1}."""
  w = np.asarray(weights, np.float64)
  ssim, cs = np.clip(np.asarray(ssim, np.float64), 0.0, np.inf), np.clip(np.asarray(cs, np.float64), 0.0, np.inf)
  return np.prod(cs[:-1] ** w[:-1, None], axis=0) * ssim[-1] ** w[-1]


def msssim_tables(img1, img2, max_val=255., weights=None, k1=0.01, k2=0.03, dtype=np.float64):
  """-> (score[B], ssim[L, B], cs[L, B]) as float64 arrays, every step before the final product computed in ``dtype``."""
  weights = WEIGHTS if weights is None else weights
  x1, x2 = np.asarray(img1).astype(dtype), np.asarray(img2).astype(dtype)
  ssim, cs = [], []
  for l in range(len(weights)):
    s, c = ssim_level(x1, x2, max_val, k1, k2)
    ssim.append(s)
    cs.append(c)
    if l + 1 < len(weights):
      x1, x2 = downsample(x1), downsample(x2)
  ssim, cs = np.asarray(ssim, np.float64), np.asarray(cs, np.float64)
  return score_from_tables(ssim, cs, weights), ssim, cs


# ---- the inputs ----------------------------------------------------------------------------------------------------------------
def texture(r, h, w, c):
  """A multi-octave random texture in [0, 1]: uniform grids of 1/1, 1/2, 1/4, ... resolution, nearest-upsampled and summed
  with equal amplitudes (every MS-SSIM level sees structure, none dominates)."""
  out = np.zeros((h, w, c), np.float64)
  octaves, step = 0, 1
  while True:
    gh, gw = -(-h // step), -(-w // step)
    out += np.repeat(np.repeat(r.rand(gh, gw, c), step, axis=0), step, axis=1)[:h, :w]
    octaves += 1
    if gh <= 2 or gw <= 2:
      break
    step *= 2
  return out / octaves


FAMILIES = ('blend10', 'blend50', 'noise', 'roll', 'affine', 'same', 'flat', 'unrelated')
SCORE_COMPARED = tuple(f for f in FAMILIES if f != 'unrelated')      # the clip bites on unrelated textures: tables only


def make_pair(seed, h, w, c, family):
  """-> (a, b) float64 [h, w, c] in [0, 1]."""
  r = np.random.RandomState(seed)
  a, o = texture(r, h, w, c), texture(r, h, w, c)
  if family == 'blend10':
    b = 0.9 * a + 0.1 * o
  elif family == 'blend50':
    b = 0.5 * a + 0.5 * o
  elif family == 'noise':
    b = np.clip(a + 0.1 * r.standard_normal(a.shape), 0.0, 1.0)
  elif family == 'roll':
    b = np.roll(a, 1, axis=1)
  elif family == 'affine':
    b = 0.8 * a + 0.1
  elif family == 'same':
    b = a.copy()
  elif family == 'flat':
    a = np.full(a.shape, 0.7)
    b = a + 1e-3 * r.standard_normal(a.shape)
  elif family == 'unrelated':
    b = o
  else:
    raise KeyError(family)
  return a, b


def round_to(x, dtype):
  """float64 -> the nearest value of the storage format ('fp32', 'bf16', 'fp16'; ties to even), returned as float32."""
  x = np.asarray(x, np.float64).astype(np.float32)
  if dtype == 'fp16':
    return x.astype(np.float16).astype(np.float32)
  if dtype == 'bf16':
    u = x.view(np.uint32).astype(np.uint64)
    u = (u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000
    return u.astype(np.uint32).view(np.float32)
  assert dtype == 'fp32', dtype
  return x


def case_inputs(case):
  """-> (d1, d2): the stored values [B, h, w, c] (float32 holding values exact in the case's dtype) that the kernel is
  given; what enters the metric is float32(d) * float32(scale), which is also what the reference was fed."""
  d1, d2 = [], []
  for i in range(case['b']):
    a, b = make_pair(case['seed'] + i, case['h'], case['w'], case['c'], case['family'])
    k = 255.0 / case['scale']      # scale 1: data in 0..255; scale 255: data in [0, 1]
    d1.append(round_to(a * k, case['dtype']))
    d2.append(round_to(b * k, case['dtype']))
  return np.stack(d1), np.stack(d2)


def metric_inputs(case, d1, d2):
  s = np.float32(case['scale'])
  return d1 * s, d2 * s


def checksum(x):
  return zlib.crc32(np.ascontiguousarray(x, np.float32).tobytes())


SHAPES = ((16, 16), (32, 32), (32, 48), (64, 64), (128, 128), (256, 256))
DTYPES = ('fp32', 'bf16', 'fp16')
SCALES = (1.0, 255.0)


def _cases():
  out, seed = [], 1000
  for h, w in SHAPES:
    for fam in FAMILIES:
      for dt in DTYPES:
        for sc in SCALES:
          out.append(dict(name='%dx%d-%s-%s-s%d' % (h, w, fam, dt, sc), h=h, w=w, c=3, b=3, dtype=dt, scale=sc, family=fam,
                          weights=None, seed=seed))
      seed += 10
  out.append(dict(name='64x64-c1-blend10-fp32-s1', h=64, w=64, c=1, b=3, dtype='fp32', scale=1.0, family='blend10',
                  weights=None, seed=9000))
  out.append(dict(name='24x40-levels3-noise-bf16-s255', h=24, w=40, c=3, b=3, dtype='bf16', scale=255.0, family='noise',
                  weights=(0.2, 0.3, 0.5), seed=9010))
  return out


CASES = _cases()
CASE_BY_NAME = {c['name']: c for c in CASES}


def load_golden():
  """-> {case name: dict(score[B], ssim[L, B], cs[L, B], mean, crc1, crc2)} as recorded from the reference's own code."""
  z = np.load(GOLDEN)
  names = [str(n) for n in z['names']]
  out = {}
  for i, n in enumerate(names):
    L = int(z['levels'][i])
    out[n] = dict(score=z['score'][i], ssim=z['ssim'][i, :L], cs=z['cs'][i, :L], mean=float(z['mean'][i]),
                  crc1=int(z['crc1'][i]), crc2=int(z['crc2'][i]))
  return out
