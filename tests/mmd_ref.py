"""The float64 restatement the kernel two-sample tests hold include/twingan_hip_mmd.h, ops.mmd_block_sums and
evaluate.KernelDistance to (TEST INFRASTRUCTURE).  No reference code exists for this metric; the definitions are those of
Binkowski et al., "Demystifying MMD GANs": the polynomial kernel k(x, y) = (gamma x.y + coef0) ** degree and the unbiased
estimator  MMD^2 = sum_{i != j} k(x_i, x_j) / (m (m - 1)) + sum_{i != j} k(y_i, y_j) / (n (n - 1)) - 2 sum_{i, j} k(x_i, y_j) / (m n).

pair_values / block_sums / estimate are plain float64.  ``fp32_steps=True`` takes t and the powers in float32, step by step as
the header states them, for the EXACT cases: there the dot product is an integer and gamma a power of two, so s and t are
exact, every float32 product is the correctly rounded one, and the float64 sum of float32 values of one magnitude is exact in
any order -- the kernel's block sums must then be bitwise these.

Bounds (block_sum_bound), per pair, with u = 2^-24, first order as the issue sets them:
  e_s = d u sum_i |a_i b_i|                              the fp32 chain's error on s
  e_t = |gamma| e_s + u (|t| + |gamma| e_s)              carried through gamma, plus the rounding of the fmaf
  e_p = degree T^(degree - 1) e_t + (degree - 1) u T^degree,  T = |t| + e_t      carried through the power, plus its products
summed over the block's pairs, plus 2^-50 sum |p| for the fp64 additions (at most 2^20 x 2^20 pairs)."""
import numpy as np

U = 2.0 ** -24


def default_gamma(d):
  return float(np.float32(1.0) / np.float32(d))


def pair_values(a, b, degree=3, gamma=None, coef0=1.0, fp32_steps=False):
  """[m, n] float64: the kernel's value for every pair of rows of ``a`` [m, d] and ``b`` [n, d]."""
  a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
  gamma = default_gamma(a.shape[1]) if gamma is None else float(np.float32(gamma))
  coef0 = float(np.float32(coef0))
  with np.errstate(all='ignore'):
    s = a @ b.T
    if not fp32_steps:
      return (gamma * s + coef0) ** degree if degree > 1 else gamma * s + coef0
    s32 = s.astype(np.float32)
    assert np.array_equal(s32.astype(np.float64), s), 'fp32_steps is for the exact cases: s must be a float32'
    t64 = gamma * s + coef0
    t = t64.astype(np.float32)
    assert np.array_equal(t.astype(np.float64), t64), 'fp32_steps is for the exact cases: t must be a float32'
    p = t.copy()
    for _ in range(degree - 1):
      p = p * t      # float32 * float32 -> float32, correctly rounded
    return p.astype(np.float64)


def mask(m, n, a_index0=0, b_index0=0, skip_same_index=False):
  """[m, n] bool: the pairs that count."""
  keep = np.ones((m, n), dtype=bool)
  if skip_same_index:
    i, j = np.arange(m, dtype=np.int64)[:, None] + int(a_index0), np.arange(n, dtype=np.int64)[None, :] + int(b_index0)
    keep &= i != j
  return keep


def sum_blocks(values, block):
  """[ceil(m / block), ceil(n / block)]: float64 sums of ``values`` [m, n] over blocks of ``block`` rows and columns."""
  m, n = values.shape
  with np.errstate(all='ignore'):
    rows = np.add.reduceat(values, np.arange(0, m, block), axis=0)
    return np.add.reduceat(rows, np.arange(0, n, block), axis=1)


def block_sums(a, b, block=32, degree=3, gamma=None, coef0=1.0, a_index0=0, b_index0=0, skip_same_index=False, fp32_steps=False):
  p = pair_values(a, b, degree, gamma, coef0, fp32_steps)
  keep = mask(p.shape[0], p.shape[1], a_index0, b_index0, skip_same_index)
  return sum_blocks(np.where(keep, p, 0.0), block)


def block_sum_bound(a, b, block=32, degree=3, gamma=None, coef0=1.0, a_index0=0, b_index0=0, skip_same_index=False):
  """The bound of the module docstring for every block sum, from the inputs alone."""
  a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
  d = a.shape[1]
  gamma = default_gamma(d) if gamma is None else float(np.float32(gamma))
  t = np.abs(gamma * (a @ b.T) + float(np.float32(coef0)))
  e_s = d * U * (np.abs(a) @ np.abs(b).T)
  e_t = abs(gamma) * e_s + U * (t + abs(gamma) * e_s)
  T = t + e_t
  e_p = degree * T ** (degree - 1) * e_t + (degree - 1) * U * T ** degree
  e_p = e_p + 2.0 ** -50 * T ** degree
  keep = mask(t.shape[0], t.shape[1], a_index0, b_index0, skip_same_index)
  return sum_blocks(np.where(keep, e_p, 0.0), block)


def estimate(kxx, kyy, kxy):
  """The unbiased estimator by its definition: double loops over the pair values [m, m], [n, n], [m, n]."""
  m, n = kxy.shape
  sxx = sum(float(kxx[i, j]) for i in range(m) for j in range(m) if i != j)
  syy = sum(float(kyy[i, j]) for i in range(n) for j in range(n) if i != j)
  sxy = sum(float(kxy[i, j]) for i in range(m) for j in range(n))
  return sxx / (m * (m - 1)) + syy / (n * (n - 1)) - 2.0 * sxy / (m * n)


def estimate_fast(x, y, **kernel):
  """estimate() of the pair values of x and y, vectorised (the off-diagonal sums by masking)."""
  kxx, kyy, kxy = pair_values(x, x, **kernel), pair_values(y, y, **kernel), pair_values(x, y, **kernel)
  m, n = kxy.shape
  return (kxx.sum() - np.trace(kxx)) / (m * (m - 1)) + (kyy.sum() - np.trace(kyy)) / (n * (n - 1)) - 2.0 * kxy.sum() / (m * n)


def from_sums(xx, yy, xy, m, n, block, subset_size):
  """The result dict of KernelDistance.end() from block sums (xx, yy without their diagonal pairs)."""
  def est(sxx, syy, sxy, rx, ry):
    return float(np.sum(sxx)) / (rx * (rx - 1)) + float(np.sum(syy)) / (ry * (ry - 1)) - 2.0 * float(np.sum(sxy)) / (rx * ry)
  per, subsets = subset_size // block, min(m, n) // subset_size
  vals = []
  for k in range(subsets):
    sl = slice(k * per, (k + 1) * per)
    vals.append(est(xx[sl, sl], yy[sl, sl], xy[sl, sl], subset_size, subset_size))
  return {'mmd2': est(xx, yy, xy, m, n), 'm': m, 'n': n, 'subset_size': subset_size, 'num_subsets': subsets,
          'kid_mean': float(np.mean(vals)) if vals else None, 'kid_std': float(np.std(vals)) if vals else None}


def kernel_distance(x, y, subset_size=1024, block=32, **kernel):
  """What KernelDistance.end() returns for the rows x [m, d] and y [n, d], in float64 throughout."""
  xx = block_sums(x, x, block, skip_same_index=True, **kernel)
  yy = block_sums(y, y, block, skip_same_index=True, **kernel)
  xy = block_sums(x, y, block, **kernel)
  return from_sums(xx, yy, xy, x.shape[0], y.shape[0], block, subset_size)


def kernel_distance_bound(x, y, subset_size=1024, block=32, with_max=False, **kernel):
  """-> (bound on |mmd2 error|, bound on |kid_mean error| or None) that the block-sum bounds imply: the estimator is linear in
  the block sums, so their bounds go through its coefficients, and the mean of the subsets' bounds bounds the mean.
  ``with_max`` adds the largest subset bound: numpy.std is sqrt(mean((v - mean) ** 2)), a 1-Lipschitz function of v / sqrt(K)
  in the 2-norm, so kid_std moves by at most sqrt(mean(e ** 2)) <= max |e|."""
  bxx = block_sum_bound(x, x, block, skip_same_index=True, **kernel)
  byy = block_sum_bound(y, y, block, skip_same_index=True, **kernel)
  bxy = block_sum_bound(x, y, block, **kernel)
  m, n = x.shape[0], y.shape[0]

  def est(sxx, syy, sxy, rx, ry):
    return float(np.sum(sxx)) / (rx * (rx - 1)) + float(np.sum(syy)) / (ry * (ry - 1)) + 2.0 * float(np.sum(sxy)) / (rx * ry)
  per, subsets = subset_size // block, min(m, n) // subset_size
  vals = []
  for k in range(subsets):
    sl = slice(k * per, (k + 1) * per)
    vals.append(est(bxx[sl, sl], byy[sl, sl], bxy[sl, sl], subset_size, subset_size))
  out = (est(bxx, byy, bxy, m, n), float(np.mean(vals)) if vals else None)
  return out + ((max(vals) if vals else None),) if with_max else out
