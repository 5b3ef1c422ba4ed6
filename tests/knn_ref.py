"""float64 / int64 NumPy restatement of the nearest-neighbour search (include/twingan_hip_knn.h), shared by tests/test_knn_cpu.py
and tests/test_gpu_knn.py (a test helper, not a conftest).

The definitions restated here are this project's own:
  * results ascend by (distance, index); equal distances resolve to the lower index;
  * a pair whose distance is NaN is never selected, and a pair at +inf never displaces the filler;
  * unfilled slots are +inf / -1;
  * cosine distance of a pair with a zero-norm row is 1;
  * the gallery row whose index equals query_ids[i] does not exist for query i.

Error bounds of the fp32 kernels against float64, from the inputs alone (u = 2^-23: one bit is left to an MFMA accumulation
that need not round to nearest; gamma_m = m u / (1 - m u)):
  squared L2   the two norms are sums of d products, each within gamma_d of itself; their sum adds one rounding; the dot
               product is within gamma_(d+1) sum|q_i g_i|, doubled exactly; the subtraction adds one rounding:
               b = gamma_(d+3) (|q|^2 + |g|^2 + 2 sum|q_i||g_i|)
  cosine       c = q.g / (|q| |g|).  The dot product's error over the denominator is gamma_(d+1) S with S = sum|q_i g_i| /
               (|q| |g|); each norm is within gamma_d, its square root within gamma_d / 2 + u, the product of the roots and
               the quotient one rounding each: |c| (gamma_d + 4 u); the final 1 - c one rounding of a number <= 2: 2 u:
               b = gamma_(d+8) (S + |c| + 1), which covers the three to first order and leaves the second order 4 u of room.
"""
import numpy as np

U = 2.0 ** -23


def gamma(m):
  return m * U / (1.0 - m * U)


def sq_l2_int(q, g):
  """int64 [Q, N]: exact squared distances of integer-valued inputs."""
  q, g = np.asarray(q).astype(np.int64), np.asarray(g).astype(np.int64)
  return (q * q).sum(1)[:, None] + (g * g).sum(1)[None, :] - 2 * (q @ g.T)


def sq_l2(q, g):
  q, g = np.asarray(q, dtype=np.float64), np.asarray(g, dtype=np.float64)
  with np.errstate(all='ignore'):
    t = (q * q).sum(1)[:, None] + (g * g).sum(1)[None, :] - 2.0 * (q @ g.T)
    return np.where(t < 0, 0.0, t)      # NaN stays NaN


def cosine(q, g):
  q, g = np.asarray(q, dtype=np.float64), np.asarray(g, dtype=np.float64)
  with np.errstate(all='ignore'):
    den = np.sqrt((q * q).sum(1))[:, None] * np.sqrt((g * g).sum(1))[None, :]
    return np.where(den == 0, 1.0, 1.0 - (q @ g.T) / np.where(den == 0, 1.0, den))


def sq_l2_bound(q, g):
  q, g = np.asarray(q, dtype=np.float64), np.asarray(g, dtype=np.float64)
  d = q.shape[1]
  return gamma(d + 3) * ((q * q).sum(1)[:, None] + (g * g).sum(1)[None, :] + 2.0 * (np.abs(q) @ np.abs(g).T))


def cosine_bound(q, g):
  q, g = np.asarray(q, dtype=np.float64), np.asarray(g, dtype=np.float64)
  d = q.shape[1]
  den = np.sqrt((q * q).sum(1))[:, None] * np.sqrt((g * g).sum(1))[None, :]
  den = np.where(den == 0, 1.0, den)
  return gamma(d + 8) * ((np.abs(q) @ np.abs(g).T) / den + np.abs(q @ g.T) / den + 1.0)


def fresh(q, k):
  return np.full((q, k), np.inf), np.full((q, k), -1, dtype=np.int64)


def topk(dist, k, index_offset=0, query_ids=None, prior=None):
  """The k best of every row of the distance matrix ``dist`` [Q, N] (any real dtype; column j is gallery index index_offset
  + j) and of ``prior`` = (dist [Q, k], idx [Q, k]) -> (float64 [Q, k], int64 [Q, k])."""
  dist = np.asarray(dist)
  nq, n = dist.shape
  out_d, out_i = fresh(nq, k)
  for i in range(nq):
    d = dist[i].astype(np.float64)
    idx = index_offset + np.arange(n, dtype=np.int64)
    if prior is not None:
      d = np.concatenate([np.asarray(prior[0][i], dtype=np.float64), d])
      idx = np.concatenate([np.asarray(prior[1][i], dtype=np.int64), idx])
    keep = ~np.isnan(d) & ~np.isposinf(d)
    if query_ids is not None:
      keep &= idx != int(query_ids[i])
    d, idx = d[keep], idx[keep]
    order = np.lexsort((idx, d))[:k]      # by distance, then index
    out_d[i, :order.size] = d[order]
    out_i[i, :order.size] = idx[order]
  return out_d, out_i


def check_real(got_d, got_i, ref, bound, k, index_offset=0, query_ids=None):
  """The two conditions of a real-valued search against the float64 distances ``ref`` [Q, N] and their bounds ``bound``:
  (1) every returned distance lies within the pair's bound of the pair's float64 distance; (2) every row that was not returned
  has a float64 distance >= that of the returned k-th row minus the two pairs' bounds (at most 2 b).  No query is excused.
  -> the worst ratios (error / bound, shortfall / allowed), for printing."""
  nq, n = ref.shape
  kk = min(k, n - (0 if query_ids is None else 1))
  worst1 = worst2 = 0.0
  for i in range(nq):
    cols = got_i[i, :kk] - index_offset
    assert np.all(got_i[i, kk:] == -1) and np.all(np.isposinf(got_d[i, kk:])), (i, got_i[i], got_d[i])
    assert np.all((cols >= 0) & (cols < n)) and np.unique(cols).size == kk, (i, got_i[i])
    if query_ids is not None:
      assert int(query_ids[i]) not in got_i[i].tolist(), i
    assert np.all(np.diff(got_d[i, :kk]) >= 0), (i, got_d[i])
    err = np.abs(got_d[i, :kk].astype(np.float64) - ref[i, cols])
    assert np.all(err <= bound[i, cols]), (i, err, bound[i, cols])
    worst1 = max(worst1, float((err / bound[i, cols]).max()))
    rest = np.ones(n, dtype=bool)
    rest[cols] = False
    if query_ids is not None and 0 <= int(query_ids[i]) - index_offset < n:
      rest[int(query_ids[i]) - index_offset] = False
    if rest.any():
      last = cols[-1]
      allowed = bound[i, rest] + bound[i, last]
      short = ref[i, last] - ref[i, rest]
      assert np.all(short <= allowed), (i, float(short.max()), float(allowed.max()))
      worst2 = max(worst2, float((short / allowed).max()))
  return worst1, worst2
