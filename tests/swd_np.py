"""Float64 NumPy restatement of the sliced Wasserstein distance the GPU kernels compute (twingan_amd/csrc/preprocess.hip,
ops.swd_*, evaluate.SlicedWasserstein) -- section 5 of the PGGAN paper with the parameters the reference fixes
(image_generation.py:938, :912-916, :910) -- written literally: zero insertion and np.pad(mode='reflect') for the pyramid, a
plain gather, np.sort.  There is no reference code to run (image_generation.py:926-931), so this file is the statement of
the algorithm the tests hold the kernels to; tests/test_swd_cpu.py pins it by its own properties.  ``dtype=np.float32``
evaluates the same formulas in float32 (the E32 of tests/elementwise.py).  Two things are float32 / float64 in BOTH
evaluations, because the algorithm says so: a pixel enters as float32(pixel) * scale (rounded to the uint8 grid with
``quantize``), and the per-channel statistics are accumulated in float64.  Seeded input makers at the end."""
import numpy as np

G = np.array([1., 4., 6., 4., 1.]) / 16.
K = 147


def resolutions(hw):
  out = []
  while hw >= 16:
    out.append(hw)
    hw //= 2
  return out


def pixels(x, scale=255., quantize=True):
  """What the metric sees of stored pixels (any float array): float32(pixel) * scale in float32, then the uint8 grid."""
  v = np.asarray(x, np.float32) * np.float32(scale)
  return np.clip(np.rint(v), 0., 255.).astype(np.float32) if quantize else v


def _filter(x, gain):
  """5 x 5 filter gain * g (x) g over axes 1, 2 of [n, h, w, c] with mirror boundary (numpy 'reflect': d c b | a b c d | c b a)."""
  g = (G * gain).astype(x.dtype)
  p = np.pad(x, ((0, 0), (2, 2), (2, 2), (0, 0)), mode='reflect')
  h, w = x.shape[1], x.shape[2]
  rows = sum(g[i] * p[:, :, i:i + w] for i in range(5))
  return sum(g[i] * rows[:, i:i + h] for i in range(5))


def down(x):
  return _filter(x, 1.)[:, ::2, ::2]


def up(x):
  z = np.zeros((x.shape[0], 2 * x.shape[1], 2 * x.shape[2], x.shape[3]), x.dtype)
  z[:, ::2, ::2] = x
  return _filter(z, 2.)      # 2 per axis: the 5 x 5 filter times 4


def up_axis_polyphase(x):
  """up along axis 0 of x [h, ...] by the border formulas of the algorithm's text (what the kernel evaluates)."""
  h = x.shape[0]
  out = np.empty((2 * h,) + x.shape[1:], x.dtype)
  for i in range(h):
    if i == 0:
      out[0] = (6 * x[0] + 2 * x[1]) / 8
    elif i == h - 1:
      out[2 * i] = (x[h - 2] + 7 * x[h - 1]) / 8
    else:
      out[2 * i] = (x[i - 1] + 6 * x[i] + x[i + 1]) / 8
    out[2 * i + 1] = x[h - 1] if i == h - 1 else (x[i] + x[i + 1]) / 2
  return out


def pyramid(v, dtype=np.float64):
  """v: metric pixels [n, hw, hw, 3] (pixels(...)) -> list of levels, finest first; the coarsest stays Gaussian."""
  pyr = [np.asarray(v, dtype)]
  for _ in resolutions(v.shape[1])[1:]:
    pyr.append(down(pyr[-1]))
    pyr[-2] = pyr[-2] - up(pyr[-1])
  return pyr


def reconstruct(pyr):
  x = pyr[-1]
  for lap in pyr[-2::-1]:
    x = lap + up(x)
  return x


def descriptors(level, centres, per):
  """level [n, s, s, 3], centres int [n * per, 2] = (y, x) -> [n * per, 147], k = c * 49 + dy * 7 + dx."""
  centres = np.asarray(centres)
  out = np.empty((centres.shape[0], K), level.dtype)
  for i, (y, x) in enumerate(centres):
    out[i] = level[i // per, y - 3:y + 4, x - 3:x + 4, :].transpose(2, 0, 1).reshape(-1)
  return out


def statistics(desc):
  """Per channel mean and 1 / population standard deviation over all N * 49 values, in float64; sigma = 0 -> rstd 0."""
  d = np.asarray(desc, np.float64).reshape(-1, 3, 49)
  mean, std = d.mean(axis=(0, 2)), d.std(axis=(0, 2))
  return mean, np.where(std > 0, 1.0 / np.where(std > 0, std, 1.0), 0.0)


def normalise(desc, dtype=np.float64):
  mean, rstd = statistics(desc)
  d = np.asarray(desc, dtype).reshape(-1, 3, 49)
  return ((d - mean.astype(dtype)[None, :, None]) * rstd.astype(dtype)[None, :, None]).reshape(-1, K)


def sorted_projections(desc, dirs, dtype=np.float64):
  """-> [R, N, D]: the set normalised by its own statistics, projected on dirs [R, 147, D], every column sorted ascending."""
  a = normalise(desc, dtype)
  return np.stack([np.sort(a @ np.asarray(dirs[r], dtype), axis=0) for r in range(len(dirs))])


def distance(desc_a, desc_b, dirs, dtype=np.float64):
  """mean_r mean_{i,d} |sort(A dirs_r) - sort(B dirs_r)| -> (mean, per_repeat [R])."""
  assert desc_a.shape == desc_b.shape, 'both sets must hold the same N'
  sa, sb = sorted_projections(desc_a, dirs, dtype), sorted_projections(desc_b, dirs, dtype)
  per = np.abs(sa - sb).mean(axis=(1, 2))
  return per.mean(), per


def swd(reals, fakes, centres, dirs, per, scale=255., quantize=True, dtype=np.float64):
  """The report: reals / fakes = lists of stored minibatches [n, hw, hw, 3] (values as the kernel reads them), centres = per
  minibatch, per level, (table of the reals, of the fakes), dirs = per level [R, 147, D].  -> (real [L], fake [L]) times 1e3:
  fake = distance(reals, fakes), real = distance(first half of the reals in feed order, second half)."""
  levels = len(resolutions(reals[0].shape[1]))
  dr, df = [[] for _ in range(levels)], [[] for _ in range(levels)]
  for mb, (r, f) in enumerate(zip(reals, fakes)):
    for which, (x, acc) in enumerate(((r, dr), (f, df))):
      for l, level in enumerate(pyramid(pixels(x, scale, quantize), dtype)):
        acc[l].append(descriptors(level, centres[mb][l][which], per))
  real, fake = [], []
  for l in range(levels):
    a, b = np.concatenate(dr[l]), np.concatenate(df[l])
    assert a.shape[0] % (2 * per) == 0, 'the real column needs an even number of images'
    fake.append(distance(a, b, dirs[l], dtype)[0] * 1e3)
    real.append(distance(a[:a.shape[0] // 2], a[a.shape[0] // 2:], dirs[l], dtype)[0] * 1e3)
  return np.array(real, np.float64), np.array(fake, np.float64)


# ---- seeded inputs -----------------------------------------------------------------------------------------------------------
def images(seed, n, hw, noise=0.08):
  """Smooth sinusoids plus noise in [0, 1], float32 [n, hw, hw, 3]."""
  rs = np.random.RandomState(seed)
  y, x = np.meshgrid(np.arange(hw) / hw, np.arange(hw) / hw, indexing='ij')
  out = np.empty((n, hw, hw, 3), np.float32)
  for i in range(n):
    for c in range(3):
      fy, fx, ph = rs.uniform(0.5, 4.0), rs.uniform(0.5, 4.0), rs.uniform(0, 2 * np.pi)
      out[i, :, :, c] = 0.5 + 0.35 * np.sin(2 * np.pi * (fy * y + fx * x) + ph) + noise * rs.randn(hw, hw)
  return np.clip(out, 0., 1.)


def centre_table(seed, rows, s):
  return np.random.RandomState(seed).randint(3, s - 3, size=(rows, 2)).astype(np.int32)


def directions(seed, repeats, dirs):
  d = np.random.RandomState(seed).randn(repeats, K, dirs)
  return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def dc_offset_set(seed, n, mean=128., sigma=30.):
  """A descriptor matrix [n, 147] whose values sit on a large offset (the cancellation a folded mean must survive)."""
  rs = np.random.RandomState(seed)
  return (mean + sigma * rs.randn(n, K) + np.repeat(np.array([-20., 0., 35.]), 49)[None]).astype(np.float32)


def flat_channel_set(seed, n, channel=1, value=37.25):
  d = dc_offset_set(seed, n)
  d[:, channel * 49:(channel + 1) * 49] = np.float32(value)
  return d
