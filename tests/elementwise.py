"""Element-wise parity: every element of a kernel's output against its own bound.

A norm over a whole tensor (rel-L2) measures rounding noise; what GPU kernels get wrong is local -- a tile edge, a halo row,
the tail chunk of a reduction, the last channel group, one image of the batch -- and a local fault's share of the tensor's
energy sits under any rel-L2 threshold that rounding noise passes (tests/test_elementwise_cpu.py shows it on planted faults).
The checks here bound |got - ref| per element.  Every bound is built from the float64 reference and the inputs alone, never
from the output under test, and is derived, not tuned:

  u(dtype)          unit roundoff of the storage type, round to nearest: 2^-8 bf16, 2^-11 fp16, 2^-24 fp32.
  tiny(dtype)       what a storage rounding can add near zero whatever |ref| is: half the subnormal spacing of fp16, 2^-25
                    (its normal range ends at 6.1e-5; gradients of unit-scale data do get there), and the smallest normal
                    number 2^-126 of bf16 / fp32 (a conversion may flush below it).  Every bound ends in + tiny; the
                    formulas below write it as 2^-126.

  conv_bound        an output stored in `dtype`, accumulated in fp32 from exact products of 16-bit operands (K summands, any
                    order -- the classical |fl(sum) - sum| <= (K-1) u32 sum|terms| to first order, K u32 taken to cover the
                    second-order terms):
                        u_out |ref| + (1 + u_out) K 2^-24 mag + 2^-126,      mag = the same sum over |operands|
                    Forward: K = k k cin, mag = conv(|x|, |w|).  Backward-data: K = k k cout, mag = conv_bwd_data(|gy|, |w|).
                    Each further fp32 operation of an epilogue (bias add, slope multiply) is one more summand: K + 1, K + 2.
  wgrad_bound       fp32 outputs summed over P pixels: 2^-24 |ref| + P 2^-24 mag, mag = bwd_weight(|x|, |gy|).
  pair_bound        two kernels of one operation, the same operands: `roundings` u_out max(|a|, |b|) + 2 K 2^-24 mag
                    (each within its accumulation error of the exact value, one storage rounding each).
  e32_bound         operations without a product structure (normalisers, pixel norm, minibatch stddev):
                        u_out |ref| + m E32,   E32 = max |f32 restatement - f64 reference|
                    of the same literal formula evaluated by torch on the CPU in float32, m = 16: torch's float32 sums are
                    pairwise (error ~ log N), the kernels sum chunks linearly and meet in atomics (up to ~ sqrt N of that).
  exact ops         (upsample, concat, cast, sign bytes) stay array_equal in the tests.

Attention, softmax, the batched GEMM, the scalar reductions and Adam (their derivations sit in the docstrings of the
functions below; every count names the kernel operation it stands for):
  attention_fwd_bound / attention_lse_bound   flash forward: P rounded to 16 bit (u), the exponent's fp32 error eps, the fp32
                    accumulation over len keys, the fp16 subnormal pack (2^-25 per key)
  attention_bwd_bounds   dQ, dK, dV of the flash backward: u_out |ref| + R u mag + A 2^-24 mag + 2^-25 S, with the forward's own
                    bounds of lse and O carried in (they are this kernel's inputs)
  gemm_bound        conv_bound with K = k + 2 (the alpha multiply, the accumulate add) and the rounding of a stored 16-bit C
  softmax kernels   e32_bound, each kernel on the operands it reads (the stored p is an operand of the two backwards)
  reduction_bound   L 2^-24 sum|terms|, L the longest chain of additions the launch geometry allows
  adam_step_bounds  one step in float64 from the fp32 state, every fp32 operation of the kernel counted once

LeakyReLU masks taken from a COMPUTED sign: an element may match `alt_ref` (the reference evaluated with the other slope)
only where `alt_where` holds (the float64 pre-activation is smaller than its own bound), and at most `alt_cap` of the
tensor's elements may take that route.
"""
import numpy as np

TINY = 2.0 ** -126
U32 = 2.0 ** -24
M_E32 = 16.0


def _name(dtype):
  return str(dtype).replace('torch.', '')


def tiny(dtype):
  """The absolute term of one storage rounding: 2^-25 for fp16 (half its subnormal spacing), 2^-126 for bf16 / fp32."""
  return 2.0 ** -25 if _name(dtype) in ('float16', 'f16', 'fp16') else TINY


def unit_roundoff(dtype):
  """Round-to-nearest unit roundoff of a storage type (a torch dtype, a numpy dtype or one of 'bf16' / 'f16' / 'f32')."""
  name = _name(dtype)
  table = {'bfloat16': 2.0 ** -8, 'bf16': 2.0 ** -8, 'float16': 2.0 ** -11, 'f16': 2.0 ** -11, 'fp16': 2.0 ** -11,
           'float32': U32, 'f32': U32, 'fp32': U32}
  if name not in table:
    raise ValueError('no unit roundoff for %r' % (dtype,))
  return table[name]


# ------------------------------------------------------------------------------------------------ bounds
def conv_bound(ref, mag, K, dtype, extra=None):
  """u_out |ref| + (1 + u_out) K 2^-24 mag + 2^-126 (+ extra: further u |intermediate| terms, named by the caller)."""
  u = unit_roundoff(dtype)
  b = u * np.abs(ref) + (1.0 + u) * K * U32 * np.abs(mag) + tiny(dtype)
  return b if extra is None else b + extra


def wgrad_bound(ref, mag, P):
  """fp32 filter / bias gradients summed over P pixels: 2^-24 |ref| + P 2^-24 mag + 2^-126."""
  return U32 * np.abs(ref) + P * U32 * np.abs(mag) + TINY


def pair_bound(a, b, mag, K, dtype, roundings=2):
  """Two kernels of the same operation on the same operands: `roundings` storage roundings and twice the accumulation term."""
  u = unit_roundoff(dtype)
  return roundings * (u * np.maximum(np.abs(a), np.abs(b)) + tiny(dtype)) + 2.0 * K * U32 * np.abs(mag)


def e32_bound(ref, e32, dtype, m=M_E32):
  """u_out |ref| + m E32 + 2^-126; e32 = max |float32 restatement - float64 reference| (a scalar, or an array per element)."""
  return unit_roundoff(dtype) * np.abs(ref) + m * np.asarray(e32, np.float64) + tiny(dtype)


def rounded_bound(ref, dtype):
  """One rounding of an exactly representable fp32 value (pool of 4, upsample adjoint of 4): u |ref| + 2^-126."""
  return unit_roundoff(dtype) * np.abs(ref) + tiny(dtype)


def e32(ref32, ref64):
  return float(np.max(np.abs(np.asarray(ref32, np.float64) - np.asarray(ref64, np.float64)))) if np.size(ref64) else 0.0


# ------------------------------------------------------------------------------------------------ minibatch stddev
def mbstd_reference(x, go, v, groups, eps, dt):
  """out = [x, mean_{h,w,c} sqrt(var_batch(x) + eps)] per group of n / groups consecutive images; first and second order by
  autograd (the gradient-penalty pattern: gx with create_graph, then the gradients of <gx, v>) -> out, gx, ggo, gx2."""
  import torch
  n, h, w, c = x.shape
  xt = x.to(dt).clone().requires_grad_(True)
  got = go.to(dt).clone().requires_grad_(True)
  xg = xt.view(groups, n // groups, h, w, c)
  mean = xg.mean(dim=1, keepdim=True)
  std = torch.sqrt(((xg - mean) ** 2).mean(dim=1) + eps)                      # [G, h, w, c]
  stat = std.mean(dim=(1, 2, 3)).view(groups, 1, 1, 1, 1).expand(groups, n // groups, h, w, 1).reshape(n, h, w, 1)
  out = torch.cat([xt, stat], dim=3)
  gx, = torch.autograd.grad(out, xt, grad_outputs=got, create_graph=True)
  ggo, gx2 = torch.autograd.grad(gx, [got, xt], grad_outputs=v.to(dt))
  return [t.detach().numpy() for t in (out, gx, ggo, gx2)]


def mbstd_conditioning(x, go, v, groups, eps):
  """What the fp32 rounding of d = x - mean_batch(x) does to the three gradients, to first order, from the float64 values.
  E32 cannot stand for it: where the samples of a position nearly coincide (|d| << |x|, certain for some position once the
  batch is 2), d carries dd = (m + 1) 2^-24 max_i |x_i| (a mean of m terms, a subtraction), sigma = sqrt(mean d^2 + eps)
  carries at most dd as well, and the gradients divide by sigma, sigma^2 and sigma^3.  With G = sum of the statistic channel's
  incoming gradient, P = hw c, S = sum_i |v_i d_i|, per position:
      gx   = go + G d / (m P sigma)                                -> G / (m P) (1 + sqrt m) dd / sigma
      T    = sum v d / (m P sigma)        (ggo's statistic channel)  -> sum |v| (1 + sqrt m) dd / (m P sigma)
      gx2  = G / (m P) [(v - mean v) / sigma - (sum v d) d / (m sigma^3)]
                                                                   -> G / (m P) [|v - mean v| dd / sigma^2
                                                                      + (sum |v| |d| + S) dd / (m sigma^3) + 3 S |d| dd / (m sigma^4)]
  -> (extra gx, extra T [one value per group], extra gx2), to be added to the E32 bounds of the fp32 path."""
  n, h, w, c = x.shape
  m, P = n // groups, h * w * c
  xg, vg = x.numpy().reshape(groups, m, h, w, c), v.numpy().reshape(groups, m, h, w, c)
  G = np.abs(go.numpy()[..., c].reshape(groups, -1).sum(axis=1)).reshape(groups, 1, 1, 1, 1)
  d = xg - xg.mean(axis=1, keepdims=True)
  sig = np.sqrt((d * d).mean(axis=1, keepdims=True) + eps)      # what the formula divides by: eps sits under the root
  dd = (m + 1) * 2.0 ** -24 * np.abs(xg).max(axis=1, keepdims=True)
  rm = 1.0 + np.sqrt(m)
  ex_gx = G / (m * P) * rm * dd / sig * np.ones_like(d)
  ex_T = (np.abs(vg) * rm * dd / sig).sum(axis=(1, 2, 3, 4)) / (m * P)
  S = np.abs(vg * d).sum(axis=1, keepdims=True)
  ex_gx2 = G / (m * P) * (np.abs(vg - vg.mean(axis=1, keepdims=True)) * dd / sig ** 2
                          + (np.abs(vg).sum(axis=1, keepdims=True) * np.abs(d) + S) * dd / (m * sig ** 3)
                          + 3 * S * np.abs(d) * dd / (m * sig ** 4))
  return ex_gx.reshape(n, h, w, c), ex_T, ex_gx2.reshape(n, h, w, c)



# ------------------------------------------------------------------------------------------------ the check


def _describe(idx_of_bad, shape, worst, got_w, ref_w, bound_w, count, total, what, via_alt, ratio):
  if len(shape) == 4:
    axes = ['n', 'h', 'w', 'c']
  else:
    axes = ['d%d' % i for i in range(len(shape))]
  box = ', '.join('%s %d..%d' % (a, lo, hi) for a, (lo, hi) in zip(axes, idx_of_bad))
  return ('%s: %d of %d elements outside their bound (worst ratio %.3g at (%s) = %s: got %.9g ref %.9g bound %.3g); '
          'violations span %s; shape %s%s'
          % (what, count, total, ratio, ', '.join(axes), tuple(int(v) for v in worst), got_w, ref_w, bound_w, box,
             tuple(shape), '; %d elements matched the other LeakyReLU slope' % via_alt if via_alt else ''))


def check_elementwise(got, ref, bound, what='', alt_ref=None, alt_where=None, alt_cap=1e-5):
  """-> (worst ratio |got - ref| / bound over the accepted elements, failure message or None)."""
  got = np.asarray(got, np.float64)
  ref = np.asarray(ref, np.float64)
  bound = np.broadcast_to(np.asarray(bound, np.float64), ref.shape)
  assert got.shape == ref.shape, (what, got.shape, ref.shape)
  assert np.all(np.isfinite(ref)) and np.all(bound > 0), (what, 'the reference or its bound is not finite / positive')
  with np.errstate(invalid='ignore', over='ignore'):
    ratio = np.abs(got - ref) / bound
  bad = ~(ratio <= 1.0)                    # NaN / inf in got: always a violation
  via_alt = 0
  if alt_ref is not None and bad.any():
    assert alt_where is not None, 'alt_ref needs alt_where'
    alt_ref = np.asarray(alt_ref, np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
      r2 = np.abs(got - alt_ref) / bound
    ok2 = bad & np.asarray(alt_where, bool) & (r2 <= 1.0)
    via_alt = int(ok2.sum())
    if via_alt > alt_cap * ref.size:
      return float(np.nanmax(ratio)), ('%s: %d of %d elements match only the other LeakyReLU slope, more than the cap of %g '
                                       'of the tensor' % (what, via_alt, ref.size, alt_cap))
    ratio = np.where(ok2, r2, ratio)
    bad = bad & ~ok2
  if not bad.any():
    return (float(ratio.max()) if ratio.size else 0.0), None
  where = np.nonzero(bad)
  rr = np.where(np.isfinite(ratio), ratio, np.inf)
  worst = np.unravel_index(int(np.argmax(np.where(bad, rr, -1.0))), ref.shape)
  box = [(int(ix.min()), int(ix.max())) for ix in where]
  msg = _describe(box, ref.shape, worst, float(got[worst]), float(ref[worst]), float(bound[worst]), int(bad.sum()), ref.size,
                  what, via_alt, float(rr[worst]))
  return float(rr[worst]), msg


def assert_elementwise(got, ref, bound, what, alt_ref=None, alt_where=None, alt_cap=1e-5):
  """Fails if any |got - ref| > bound (non-finite `got` included).  The message names the worst element as (n, h, w, c), its
  got / ref / bound, the number of violations and their bounding box per axis.  Returns the worst ratio."""
  worst, msg = check_elementwise(got, ref, bound, what, alt_ref, alt_where, alt_cap)
  assert msg is None, msg
  return worst


# ------------------------------------------------------------------------------------------------ whole batch, on the device
def conv_taps(x, w, padding, transpose=False):
  """Stride-1 NHWC conv as one torch matmul per tap, in the operands' own dtype and on their device (transpose: the
  backward-data of that conv).  x [n, h, w, c], w [k, k, cin, cout] -> [n, ho, wo, cout] (transpose: cin)."""
  import torch
  import torch.nn.functional as F
  k = w.shape[0]
  assert padding in ('SAME', 'VALID') and (padding != 'SAME' or k % 2 == 1)
  if transpose:
    w = w.flip(0, 1).transpose(2, 3)
    pad = (k - 1) // 2 if padding == 'SAME' else k - 1
  else:
    pad = (k - 1) // 2 if padding == 'SAME' else 0
  if pad:
    x = F.pad(x, (0, 0, pad, pad, pad, pad))
  n, hp, wp, _ = x.shape
  ho, wo = hp - k + 1, wp - k + 1
  out = torch.zeros((n, ho, wo, w.shape[3]), dtype=x.dtype, device=x.device)
  for i in range(k):
    for j in range(k):
      out += x[:, i:i + ho, j:j + wo, :] @ w[i, j]
  return out


def conv_mag_device(x, w, padding, transpose=False):
  """sum over taps and channels of |x| |w| (the magnitude term of conv_bound / pair_bound) in float32 on x's device,
  raised by its own worst-case summation error so that it never falls below the exact sum."""
  k = w.shape[0]
  return conv_taps(x.float().abs(), w.float().abs(), padding, transpose) * (1.0 + k * k * max(w.shape[2], w.shape[3]) * U32)


def norm_act_reference(y, gamma, beta, gz, gamma2=None, beta2=None, split=None, lrelu=True, pixel_norm=True, pool=False,
                       gzp=None, eps=1e-6, pn_eps=1e-6, alpha=0.2, flip=None, layer=False, detach_stats=False):
  """The literal formulas of the fused normaliser in y's dtype (float64: the reference; float32: its restatement for E32),
  torch on the CPU, gradients by autograd:
      u = (y - mean) rsqrt(var + eps) gamma + beta      mean / var over (H, W) of each image (layer: over (H, W, C))
      a = u (u > 0 ? 1 : alpha)                         flip: boolean mask of elements that take the OTHER slope
      z = a rsqrt(mean_C(a^2) + pn_eps),  zp = 2x2 mean of z
  gamma / beta: [c] (images [split, n) use gamma2 / beta2) or one row per image [n, c].
  detach_stats: mean / var are constants of the backward (the part of gy that does not pass through the statistics).
  -> dict(z, zp, gy, grads (in the order gamma, beta[, gamma2, beta2]), u)."""
  import torch
  dt = y.dtype
  n, h, w, c = y.shape
  y = y.detach().clone().requires_grad_(True)
  pars = [t.detach().to(dt).clone().requires_grad_(True) for t in (gamma, beta, gamma2, beta2) if t is not None]
  if pars[0].dim() == 2:
    G, B = pars[0].view(n, 1, 1, c), pars[1].view(n, 1, 1, c)
  elif len(pars) == 4:
    sel = (torch.arange(n) >= int(split)).view(n, 1, 1, 1)
    G, B = torch.where(sel, pars[2], pars[0]), torch.where(sel, pars[3], pars[1])
  else:
    G, B = pars[0], pars[1]
  dims = (1, 2, 3) if layer else (1, 2)
  mean = y.mean(dim=dims, keepdim=True)
  var = ((y - mean) ** 2).mean(dim=dims, keepdim=True)
  if detach_stats:
    mean, var = mean.detach(), var.detach()
  u = (y - mean) * torch.rsqrt(var + eps) * G + B
  a = u
  if lrelu:
    pos = u.detach() > 0
    if flip is not None:
      pos = pos ^ flip
    a = u * torch.where(pos, torch.ones((), dtype=dt), torch.full((), alpha, dtype=dt))
  z = a * torch.rsqrt((a * a).mean(dim=3, keepdim=True) + pn_eps) if pixel_norm else a
  outs, gouts = [z], [gz.to(dt)]
  zp = None
  if pool:
    zp = z.reshape(n, h // 2, 2, w // 2, 2, c).mean(dim=(2, 4))
    outs.append(zp)
    gouts.append(gzp.to(dt))
  torch.autograd.backward(outs, gouts)
  return dict(z=z.detach(), zp=None if zp is None else zp.detach(), gy=y.grad, grads=[p.grad for p in pars], u=u.detach())


def assert_pair_device(a, b, mag, K, what, roundings=2, chunk=8, extra=None):
  """Two kernels' outputs over the WHOLE batch, compared on the device in float32 against pair_bound; only the violation
  report comes back to the host.  `mag`: callable(i0, i1) -> float32 magnitude term of images [i0, i1); `extra`: callable
  of the same form -> a further term of the bound (a storage rounding one of the two routes defines), named by the caller."""
  import torch
  u = unit_roundoff(a.dtype)
  assert a.shape == b.shape, (what, a.shape, b.shape)
  worst, nbad, rep = 0.0, 0, None
  for i0 in range(0, a.shape[0], chunk):
    i1 = min(a.shape[0], i0 + chunk)
    af, bf = a[i0:i1].float(), b[i0:i1].float()
    bound = roundings * (u * torch.maximum(af.abs(), bf.abs()) + tiny(a.dtype)) + (2.0 * K * U32) * mag(i0, i1)
    if extra is not None:
      bound = bound + extra(i0, i1)
    ratio = (af - bf).abs() / bound
    bad = ~(ratio <= 1.0)
    cnt = int(bad.sum())
    good = torch.where(bad, torch.zeros_like(ratio), ratio)
    worst = max(worst, float(good.max()))
    if cnt:
      nbad += cnt
      if rep is None:
        idx = bad.nonzero()
        rr = torch.where(torch.isfinite(ratio), ratio, torch.full_like(ratio, float('inf')))
        flat = int(torch.where(bad, rr, torch.full_like(rr, -1.0)).argmax())
        wi = np.unravel_index(flat, tuple(af.shape))
        box = [(int(idx[:, d].min()) + (i0 if d == 0 else 0), int(idx[:, d].max()) + (i0 if d == 0 else 0))
               for d in range(idx.shape[1])]
        rep = (box, (wi[0] + i0,) + tuple(wi[1:]), float(af[wi]), float(bf[wi]), float(bound[wi]), float(rr[wi]))
  if rep is not None:
    box, wi, ga, gb, bd, rw = rep
    raise AssertionError(_describe(box, tuple(a.shape), wi, ga, gb, bd, nbad, a.numel(), what + ' (first failing chunk)', 0, rw))
  return worst


# ------------------------------------------------------------------------------------------------ batched GEMM
def gemm_bound(ref, mag, k, dtype, c0=None, c_f32=False):
  """tg_batched_gemm: C = alpha op(A) op(B) (+ C0).  conv_bound with K = k products accumulated in fp32 (MFMA, or fmaf in
  the fp32 kernel), + 1 for `g.alpha * acc`, + 1 for the `*c + v` of accumulate; mag = |alpha| |a| |b| (+ |C0|).
  `ref` includes C0.  A 16-bit C0 is read back exactly; the sum is rounded once to C's type (fp32 when c_f32)."""
  out = 'f32' if c_f32 else dtype
  K = k + 1 + (0 if c0 is None else 1)
  m = np.abs(mag) + (0.0 if c0 is None else np.abs(c0))
  return conv_bound(ref, m, K, out)


# ------------------------------------------------------------------------------------------------ row softmax
def softmax_kernels_reference(s, p, dp, v, dt):
  """The three softmax kernels' literal formulas in numpy dtype `dt` (float64: the reference; float32: the restatement for
  E32), each on the operands the kernel itself READS -- the backward kernels take the STORED p, so p is an operand here,
  already rounded to the storage type, and nothing a 16-bit store did to it is left for the bound to cover:
      fwd      softmax(s)                                tg_softmax_rows_fwd
      bwd      p (dp - t),            t = sum dp p      tg_softmax_rows_bwd
      bwd_bwd  v (dp - t) - dp u,     u = sum v p       tg_softmax_rows_bwd_bwd
  -> (fwd, bwd, bwd_bwd)."""
  s, p, dp, v = (np.asarray(x, dt) for x in (s, p, dp, v))
  e = np.exp(s - s.max(-1, keepdims=True))
  fwd = e / e.sum(-1, keepdims=True, dtype=dt)
  t = (dp * p).sum(-1, keepdims=True, dtype=dt)
  u = (v * p).sum(-1, keepdims=True, dtype=dt)
  return fwd, p * (dp - t), v * (dp - t) - dp * u


# ------------------------------------------------------------------------------------------------ scalar reductions
def reduction_chain(numel, dtype, cap, vec=True, block=256, one_block=None):
  """The longest chain of fp32 additions a term of sum_kernel / sample_sumsq_kernel can pass through, from the launch
  geometry the entry points define (csrc/reduce.hip): blocks = min(cap, ceil((numel / V + 1) / 256)) workgroups of 256
  threads (ONE for fp32 and in deterministic mode: the exact-parity path -- one_block; tg_sum_ordered keeps its grid for every
  type: one_block=False), V = 16 bytes of the type; per thread ceil(nvec / threads) trips of V
  additions plus ceil(tail / threads) scalar ones (vec False: every element is tail); 6 butterfly levels of the wave sum and
  the 4 wave partials of block_sum added in order; one atomic (or ordered) addition per workgroup; one multiply by the
  scale.  -> (L, blocks)."""
  V = 16 // {'float32': 4}.get(_name(dtype), 2)
  if one_block is None:
    one_block = _name(dtype) == 'float32'
  blocks = 1 if one_block else max(1, min(cap, (numel // V + 1 + block - 1) // block))
  threads = blocks * block
  nvec = numel // V if vec else 0
  trips = -(-nvec // threads)
  tail = -(-(numel - nvec * V) // threads)
  return trips * V + tail + 6 + block // 64 + blocks + 1, blocks


def reduction_bound(terms_abs_sum, L, scale=1.0, term_ops=0):
  """|err| <= (L + term_ops) 2^-24 |scale| sum|terms| + 2^-126; term_ops: the fp32 operations that FORM a term (1 for |a - b| and
  for the fmaf of x^2, 0 for a plain sum)."""
  return (L + term_ops) * U32 * abs(scale) * float(terms_abs_sum) + TINY


def gp_penalty_bounds(ss, L, lam):
  """tg_sample_sumsq + tg_gp_penalty from the float64 per-sample sums of squares ss[b] (L: reduction_chain of one sample):
      ss^      (L + 1) 2^-24 ss                      the fmaf chain
      slope    sqrtf: d ss / (2 slope) + 2 2^-24 slope (one unit in the last place); a zero sample has slope = 0 exactly
      d        slope - 1: one rounding
      d^2      2 |d| dd + 2^-24 d^2;  summed over the batch by one workgroup: (ceil(batch / 256) + 12) 2^-24 sum d^2;
               lambda * tot / batch: two operations
      coef     lambda 2 d / (slope batch): three multiplies and a division (2): 5 2^-24 |coef| + the errors of d and slope;
               slope = 0: coef = 0, this project's choice (the literal formula divides 0 by 0)
  -> (loss, coef) references and (b_loss, b_coef)."""
  ss = np.asarray(ss, np.float64)
  b = ss.size
  slope = np.sqrt(ss)
  dss = (L + 1) * U32 * ss
  pos = slope > 0
  sl = np.where(pos, slope, 1.0)
  dslope = np.where(pos, dss / (2 * sl) + 2 * U32 * slope, 0.0)
  d = slope - 1.0
  dd = dslope + U32 * np.abs(d)
  loss = lam * (d * d).sum() / b
  b_loss = lam / b * ((2 * np.abs(d) * dd + U32 * d * d).sum() + (-(-b // 256) + 12) * U32 * (d * d).sum()) + TINY
  coef = np.where(pos, lam * 2.0 * d / (sl * b), 0.0)
  b_coef = np.where(pos, lam * 2.0 / b * (dd / sl + np.abs(d) * dslope / sl ** 2) + 5 * U32 * np.abs(coef), 0.0) + TINY
  return (loss, coef), (b_loss, b_coef)


# ------------------------------------------------------------------------------------------------ Adam
def adam_step_bounds(th, g, m, v, lr_t, b1, b2, eps, gscale):
  """One step of apply_kernel's Adam rule (adam_element, csrc/reduce.hip) in float64 from the fp32 state it READS (the previous step's stored theta, m,
  v: inputs of this launch, not its output), with the fp32 scalars it is given, and the error of every fp32 operation on
  the way.  Each operation counts 2^-24 of its result (the compiler may contract a multiply into the following add, which
  only removes a rounding); sqrtf and the division are not required to be correctly rounded: one unit in the last place
  (2 x 2^-24) each; every operation may also flush a subnormal result: + 2^-126.
      gi = g gscale                                1 rounding
      mi = b1 m + (1 - b1) gi                      (1 - b1), two products, the sum, gi's own: 4 u32 (|b1 m| + |(1 - b1) gi|)
      vi = b2 v + (1 - b2) gi gi                   gi twice, (1 - b2), two products (three multiplies), the sum: 7 u32 vi
      r  = sqrtf(vi)                               |sqrt(a) - sqrt(b)| <= min(|a - b| / sqrt(b), sqrt|a - b|), + 2 u32 r
      d  = r + eps                                 1 rounding
      t  = th - lr_t mi / d                        one multiply, the division (2), the subtraction
  -> (theta, m, v) references and (b_theta, b_m, b_v) bounds, numpy float64 or torch float64 alike (operator syntax only)."""
  f32 = np.float32
  b1, b2, eps, gscale, lr_t = (float(f32(x)) for x in (b1, b2, eps, gscale, lr_t))
  c1, c2 = float(f32(1.0) - f32(b1)), float(f32(1.0) - f32(b2))
  sqrt = (lambda a: a.sqrt()) if hasattr(th, 'sqrt') else np.sqrt
  minimum = (lambda a, b: a.minimum(b)) if hasattr(th, 'minimum') else np.minimum
  gi = g * gscale
  mi = b1 * m + c1 * gi
  vi = b2 * v + c2 * gi * gi
  bm = 4.0 * U32 * (abs(b1 * m) + abs(c1 * gi)) + 2 * TINY
  bv = 7.0 * U32 * vi + 3 * TINY
  r = sqrt(vi)
  br = minimum(bv / (r + 1e-300), sqrt(bv)) + 2.0 * U32 * r + TINY
  d = r + eps
  bd = br + U32 * d + TINY
  upd = lr_t * mi / d
  # d is at least eps - bd away from zero; relative error of the quotient to first order, the denominator's taken at d - bd
  bupd = lr_t * bm / (d - bd) + abs(upd) * (bd / (d - bd) + 3.0 * U32) + 2 * TINY
  t = th - upd
  bt = U32 * abs(t) + (1.0 + U32) * bupd + TINY
  return (t, mi, vi), (bt, bm, bv)


# ------------------------------------------------------------------------------------------------ flash attention
K_STALE = 6.0      # csrc/flash.hip kStaleMax: the running maximum may lag the true one by this much (natural-log units)


def attention_terms(q, k, v):
  """float64 softmax attention of [n, len, d] operands and the magnitudes the bounds need -> dict(s, smax, p, lse, o, mag
  (= p |v|), A (= max_j |q_i| . |k_j|, per query), vsum (= sum_j |v_j|, per feature))."""
  s = np.einsum('nid,njd->nij', q, k)
  smax = s.max(-1)
  e = np.exp(s - smax[..., None])
  l = e.sum(-1)
  p = e / l[..., None]
  return dict(s=s, smax=smax, p=p, lse=smax + np.log(l), o=np.einsum('nij,njd->nid', p, v),
              mag=np.einsum('nij,njd->nid', p, np.abs(v)), A=np.einsum('nid,njd->nij', np.abs(q), np.abs(k)).max(-1),
              vsum=np.abs(v).sum(1))


def attention_eps(A, dqk, ln):
  """The relative error of one unnormalised fp32 probability exp(s_ij - m) of flash_fwd_kernel before it is packed, in units
  of 2^-24, counted from the kernel's own operations (A = max_j |q_i| . |k_j| bounds |s| and |m|):
      d_qk A      the score: d_qk exact products accumulated in fp32 by the MFMA (the zero padding to 16 adds nothing)
      2 A         fma(s, log2e, -m2): one rounding of a value of magnitude |s - m| log2e <= 2 A log2e, times ln 2
      2 A         log2e as an fp32 constant (relative 2^-24) scales s - m, |s - m| <= 2 A
      A           m2 = m_new * log2e, rounded once per rescale; it holds for the whole span of blocks that use it
      2           v_exp_f32: one unit in the last place
      4 A         the rescales: (m_run - m_new) and its product with log2e are rounded, each relative to |m_run - m_new|;
                  the increments of one row are all positive and sum to at most the range of its scores, 2 A
      3 len / 32  per rescale (at most one per 32-key block) one v_exp_f32 (2) and one multiply acc *= corr (1)
  -> ((d_qk + 9) A + 2 + 3 len / 32) 2^-24."""
  return ((dqk + 9.0) * A + 2.0 + 3.0 * (ln // 32)) * U32


def _attention_rho(eps, ln, dtype):
  """Relative error of the row sum l: every summand rounded to 16 bit (u) after its exponent error (eps), summed in fp32
  over len keys (len 2^-24), and -- l >= 1 - eps, the key that set the maximum has p = 1 -- the absolute 2^-25 of an fp16
  subnormal per key."""
  u = unit_roundoff(dtype)
  r = u + eps + ln * U32 + ln * tiny(dtype)
  assert np.all(r < 0.5), 'the exponent error alone exceeds one half: the bound says nothing at this score scale'
  return r


def attention_fwd_bound(t, dqk, dtype):
  """O = N / l, N = sum_j p_j v_j, both from the SAME packed probabilities.  |N^ - N| <= (u + eps + len 2^-24) mag l +
  2^-25 sum_j |v_j| (fp16 subnormal pack; l >= 1), |l^ - l| <= rho l; 1 / l and acc * inv are two fp32 operations; one storage
  rounding:
      u |ref| + (1 + u) [((u + eps + len 2^-24) (mag + |ref|) + tiny16 (sum_j |v_j| + len |ref|)) / (1 - rho) + 2 2^-24 |ref|] + tiny
  t = attention_terms(q, k, v)."""
  u = unit_roundoff(dtype)
  ln = t['s'].shape[-1]
  eps = attention_eps(t['A'], dqk, ln)[..., None]
  rho = _attention_rho(eps, ln, dtype)
  ref = np.abs(t['o'])
  num = (u + eps + ln * U32) * (t['mag'] + ref) + tiny(dtype) * (t['vsum'][:, None, :] + ln * ref)
  return u * ref + (1.0 + u) * (num / (1.0 - rho) + 2.0 * U32 * ref) + tiny(dtype)


def attention_lse_bound(t, dqk, dtype):
  """lse = m_run + __logf(l): l carries rho (relative), so log l carries -log(1 - rho); __logf is v_log_f32 (one unit in
  the last place) times ln 2, rounded: 3 2^-24 |log l| with |log l| <= lse - max_j s + kStaleMax + rho (the stale maximum);
  the final addition is one rounding of |lse|."""
  ln = t['s'].shape[-1]
  rho = _attention_rho(attention_eps(t['A'], dqk, ln), ln, dtype)
  logl = np.abs(t['lse'] - t['smax']) + K_STALE + rho
  return -np.log1p(-rho) + 3.0 * U32 * logl + U32 * np.abs(t['lse']) + TINY


def attention_grads_reference(q, k, v, go, t=None):
  """dQ, dK, dV of softmax attention in float64 and the magnitude terms of their bounds -> dict."""
  t = attention_terms(q, k, v) if t is None else t
  p = t['p']
  gp = np.einsum('nid,njd->nij', go, v)
  D = (gp * p).sum(-1, keepdims=True)
  ds = p * (gp - D)
  gpa = np.einsum('nid,njd->nij', np.abs(go), np.abs(v))
  Da = (p * gpa).sum(-1, keepdims=True)
  dsa = p * (gpa + Da)
  return dict(dq=np.einsum('nij,njd->nid', ds, k), dk=np.einsum('nij,nid->njd', ds, q), dv=np.einsum('nij,nid->njd', p, go),
              gpa=gpa, Da=Da, dsa=dsa, mag_dq=np.einsum('nij,njd->nid', dsa, np.abs(k)),
              mag_dk=np.einsum('nij,nid->njd', dsa, np.abs(q)), mag_dv=np.einsum('nij,nid->njd', p, np.abs(go)))


def attention_bwd_bounds(q, k, v, go, t, r, dqk, dtype):
  """flash_bwd_q_kernel / flash_bwd_kv_kernel, each bound of the form u_out |ref| + R u mag + A 2^-24 mag + T tiny16 S, every
  term named.  Per query i the recomputed probability p^ = exp2(fma(s, log2e, -lse2)) carries, relative,
      epb_i = ((d_qk + 2) A_i + 3 |lse_i| + 2) 2^-24 + Blse_i
  (the score's accumulation d_qk A; the fma's rounding and the fp32 log2e on |s - lse| <= A + |lse|: 2 (A + |lse|); lse2 = lse
  log2e rounded: |lse|; v_exp_f32: 2) -- and Blse_i, the forward's own lse bound: the lse this kernel READS is the forward
  kernel's output (R: "lse carrying the forward's error", about one u).
      dV_j = sum_i pack(p^_ij) dO_i       R u: P packed (1) + Blse;  A = len;  T S = 2^-25 sum_i |dO_i|
      D_i  = <dO_i, O_i> from the STORED O: |D^ - D| <= sum_d |dO_id| BO_id + d_v 2^-24 sum_d |dO_id| |O_id| =: dD_i with BO the
             forward's own element bound (R: "O stored in 16 bit")
      ds^_ij = pack(p^ (dp - D^)): dp = dO V^T over d_v products (d_v 2^-24 gpa), the subtraction and the multiply (2 2^-24
             of gpa + Da), the pack (u, and 2^-25 absolute in fp16):
             |ds^ - ds| <= (u + epb_i + (d_v + 3) 2^-24) dsa_ij + p_ij dD_i + tiny16
      dQ_i = sum_j ds^_ij k_j             A = len;  T S = 2^-25 sum_j |k_j|
      dK_j = sum_i ds^_ij q_i             A = len;  T S = 2^-25 sum_i |q_i|
  t = attention_terms, r = attention_grads_reference -> (b_dq, b_dk, b_dv)."""
  u = unit_roundoff(dtype)
  t16 = tiny(dtype)
  n, ln, _ = q.shape
  dv = v.shape[2]
  p = t['p']
  epb = ((dqk + 2.0) * t['A'] + 3.0 * np.abs(t['lse']) + 2.0) * U32 + attention_lse_bound(t, dqk, dtype)      # [n, len]
  ago, aq, ak = np.abs(go), np.abs(q), np.abs(k)
  dD = (ago * attention_fwd_bound(t, dqk, dtype)).sum(-1) + dv * U32 * (ago * np.abs(t['o'])).sum(-1)       # [n, len]
  rel = (u + epb + (dv + 3.0) * U32)[..., None]                                                              # per query
  eds = rel * r['dsa'] + p * dD[..., None]                                                                   # [n, i, j]
  b_dq = u * np.abs(r['dq']) + (1 + u) * (np.einsum('nij,njd->nid', eds, ak) + ln * U32 * r['mag_dq']
                                          + t16 * ak.sum(1)[:, None, :]) + t16
  b_dk = u * np.abs(r['dk']) + (1 + u) * (np.einsum('nij,nid->njd', eds, aq) + ln * U32 * r['mag_dk']
                                          + t16 * aq.sum(1)[:, None, :]) + t16
  epv = (u + epb)[..., None] * p
  b_dv = u * np.abs(r['dv']) + (1 + u) * (np.einsum('nij,nid->njd', epv, ago) + ln * U32 * r['mag_dv']
                                          + t16 * ago.sum(1)[:, None, :]) + t16
  return b_dq, b_dk, b_dv



def attention_bwd_bwd_bounds(q, k, v, go, aq, ak, av, t, r, dqk, dtype):
  """flash_bb_stats / flash_bb_q / flash_bb_kv (csrc/flash.hip), the closed form of oracle/np_ops.attention_backward_backward
  evaluated on the absolute values of its operands with every difference turned into a sum -- the magnitudes -- and the
  error of every fp32 quantity on the way, to first order, per (query i, key j).  With epb_i and dD_i as in
  attention_bwd_bounds (the recomputed probability's relative error with the forward's lse bound in it; D from the stored O):
      gp  = dO V^T      d_v products       |d gp| <= d_v 2^-24 gpa            gpa = |dO| |V|^T
      w   = aQ K^T + Q aK^T   2 d_qk       |d w|  <= 2 d_qk 2^-24 wa          wa  = |aQ| |K|^T + |Q| |aK|^T
      y   = dO aV^T     d_v products       |d y|  <= d_v 2^-24 ya             ya  = |dO| |aV|^T
      E_i = sum_j p w   (fp32 chain)       dE_i = (epb + (2 d_qk + 1 + len) 2^-24) Ea,   Ea = sum_j p wa
      F_i = J + H - 2 D E,  J = sum p y, H = sum p w gp:
            dF_i = (epb + (d_v + 1 + len) 2^-24) Ja + (epb + (2 d_qk + d_v + 2 + len) 2^-24) Ha + 2 (dD Ea + Da dE)
                   + 8 2^-24 Fa,     Ja = sum p ya, Ha = sum p wa gpa, Fa = Ja + Ha + 2 Da Ea
      the four packed maps (u each, 2^-25 absolute in fp16):
      pv = p                               (u + epb) p
      gs = p (gp - D)                      (u + epb + (d_v + 3) 2^-24) dsa + p dD                         dsa = p (gpa + Da)
      tv = p (w - E)                       (u + epb + (2 d_qk + 3) 2^-24) Ta + p dE                       Ta = p (wa + Ea)
      uv = p (x - F), x = fma(w, gp - D, y) - E gp:   Xa = ya + wa (gpa + Da) + Ea gpa,
            dx = (3 d_v + 2 d_qk + 3) 2^-24 Xa + wa dD + gpa dE;   (u + epb + 2 2^-24) Ua + p (dx + dF),   Ua = p (Xa + Fa)
      adj Q  = gs aK + uv K,  adj dO = pv aV + tv V   (sums over keys),   adj K = gs^T aQ + uv^T Q,  adj V = tv^T dO  (over queries):
      each the map errors times the other operand's magnitude, + 2 len 2^-24 mag (two MFMA chains of len), + 2^-25 S, + u_out |ref|.
  The saturated rows (late_spike): D, a fmaf chain over d_v products, and gP, an MFMA sum over the same products, differ by up
  to d_v 2^-24 gpa each where the exact difference is 0, and the difference meets |k| = 20 in adj Q: the (d_v + 3) 2^-24 dsa |K|
  term above -- absolute noise of that size next to a true value of 1e-29 is inside the bound, by derivation.
  -> bounds of (adj q, adj k, adj v, adj dO); `refs` = the float64 adjoints in that order."""
  u = unit_roundoff(dtype)
  t16 = tiny(dtype)
  n, ln, _ = q.shape
  dv = v.shape[2]
  p = t['p']
  A = lambda x: np.abs(x)
  mm = lambda a, b: np.einsum('nid,njd->nij', a, b)
  epb = (((dqk + 2.0) * t['A'] + 3.0 * np.abs(t['lse']) + 2.0) * U32 + attention_lse_bound(t, dqk, dtype))[..., None]
  dD = ((A(go) * attention_fwd_bound(t, dqk, dtype)).sum(-1) + dv * U32 * (A(go) * A(t['o'])).sum(-1))[..., None]
  gpa, Da, dsa = r['gpa'], r['Da'], r['dsa']
  wa = mm(A(aq), A(k)) + mm(A(q), A(ak))
  ya = mm(A(go), A(av))
  rs = lambda x: x.sum(-1, keepdims=True)
  Ea, Ja, Ha = rs(p * wa), rs(p * ya), rs(p * wa * gpa)
  Fa = Ja + Ha + 2 * Da * Ea
  dE = (epb + (2 * dqk + 1 + ln) * U32) * Ea
  dF = (epb + (dv + 1 + ln) * U32) * Ja + (epb + (2 * dqk + dv + 2 + ln) * U32) * Ha + 2 * (dD * Ea + Da * dE) + 8 * U32 * Fa
  Ta = p * (wa + Ea)
  Xa = ya + wa * (gpa + Da) + Ea * gpa
  Ua = p * (Xa + Fa)
  e_pv = (u + epb) * p
  e_gs = (u + epb + (dv + 3) * U32) * dsa + p * dD
  e_tv = (u + epb + (2 * dqk + 3) * U32) * Ta + p * dE
  dx = (3 * dv + 2 * dqk + 3) * U32 * Xa + wa * dD + gpa * dE
  e_uv = (u + epb + 2 * U32) * Ua + p * (dx + dF)
  kj = lambda m, x: np.einsum('nij,njd->nid', m, x)      # sum over keys
  qi = lambda m, x: np.einsum('nij,nid->njd', m, x)      # sum over queries
  colsum = lambda *xs: sum(A(x).sum(1) for x in xs)[:, None, :]

  def fin(ref, err, mag, S):
    return u * np.abs(ref) + (1 + u) * (err + 2 * ln * U32 * mag + t16 * S) + t16
  refs = r['bb']
  b_q = fin(refs[0], kj(e_gs, A(ak)) + kj(e_uv, A(k)), kj(dsa, A(ak)) + kj(Ua, A(k)), colsum(ak, k))
  b_k = fin(refs[1], qi(e_gs, A(aq)) + qi(e_uv, A(q)), qi(dsa, A(aq)) + qi(Ua, A(q)), colsum(aq, q))
  b_v = fin(refs[2], qi(e_tv, A(go)), qi(Ta, A(go)), colsum(go))
  b_go = fin(refs[3], kj(e_pv, A(av)) + kj(e_tv, A(v)), kj(p, A(av)) + kj(Ta, A(v)), colsum(av, v))
  return b_q, b_k, b_v, b_go


ATTENTION_FAMILIES = ('benign', 'ramp_up', 'ramp_down', 'slow_up', 'mixed', 'late_spike', 'big', 'equal')


def attention_family(name, n, ln, dk, rng, rnd):
  """q, k [n, len, d_qk] of one score family, built in float64 and rounded to the storage type by `rnd`.  benign: q =
  tanh(randn), k = tanh(2 randn); the others overwrite feature 0 (j = key index / len):
      ramp_up     q0 = 4, k0 = 16 j          every 32-key block raises the maximum by 2048 / len
      ramp_down   q0 = 4, k0 = -16 j         the maximum sits in block 0, later probabilities underflow the 16-bit pack
      slow_up     q0 = 4, k0 = 1.25 (len / 32) j     a rise of 5 per block: stale maximum, p > 1, a rescale every second block
      mixed       q0 = +4 (odd queries) / -4 (even), k0 = 16 j    the lanes of one wave disagree on `raise`
      late_spike  q0 = 4, k0 = 0 except k[len - 3][0] = 20        one rescale by e^80 in the last block, saturated rows
      big         q and k times 6
      equal       every key the same: uniform rows"""
  q = np.tanh(rng.randn(n, ln, dk))
  k = np.tanh(rng.randn(n, ln, dk) * 2)
  j = np.arange(ln) / float(ln)
  if name in ('ramp_up', 'ramp_down', 'slow_up', 'late_spike'):
    q[:, :, 0] = 4.0
  if name == 'ramp_up' or name == 'mixed':
    k[:, :, 0] = 16.0 * j
  elif name == 'ramp_down':
    k[:, :, 0] = -16.0 * j
  elif name == 'slow_up':
    k[:, :, 0] = 1.25 * (ln / 32.0) * j
  elif name == 'late_spike':
    k[:, :, 0] = 0.0
    k[:, ln - 3, 0] = 20.0
  elif name == 'big':
    q, k = q * 6.0, k * 6.0
  elif name == 'equal':
    k = np.repeat(k[:, :1], ln, axis=1)
  if name == 'mixed':
    q[:, :, 0] = np.where(np.arange(ln) % 2 == 1, 4.0, -4.0)
  assert name in ATTENTION_FAMILIES, name
  return rnd(q), rnd(k)


# ------------------------------------------------------------------------------------------------ spectral norm
def sn_formulas(w2, u, G, dt):
  """libs/sn.py:38-101 for one power iteration, literally, in torch dtype `dt` on the CPU (float64: the reference; float32:
  its restatement for E32), the gradient by autograd with nothing stopped:
      v_raw = u W^T,  v = l2n(v_raw),  u_raw = v W,  u' = l2n(u_raw),  sigma = v W u'^T,  W_bar = W / sigma,
      l2n(x) = x / sqrt(max(sum x^2, 1e-12))                              (tf.nn.l2_normalize)
  w2 [K, cout], u [1, cout], G = d L / d W_bar [K, cout] -> dict of numpy float64 arrays: w_bar, u_new, v, stats = {sigma,
  sqrt(max(|v_raw|^2, 1e-12))} (what the kernel saves for its backward), gw, and the float64 pieces of the gradient's
  magnitude (sigma, s = sum G o W, b = (a - v (v . a)) / |v_raw| with a = W u'^T)."""
  import torch
  w = w2.detach().to(dt).clone().requires_grad_(True)
  ut, g = u.detach().to(dt).reshape(1, -1), G.detach().to(dt)
  l2n = lambda x: x / x.pow(2).sum().clamp_min(1e-12).sqrt()
  v_raw = ut @ w.t()
  v = l2n(v_raw)
  u1 = l2n(v @ w)
  sigma = (v @ w @ u1.t()).reshape(())
  w_bar = w / sigma
  gw, = torch.autograd.grad((w_bar * g).sum(), w)
  nv = v_raw.pow(2).sum().clamp_min(1e-12).sqrt()
  a = w.detach() @ u1.detach().t()                                   # [K, 1]
  vd = v.detach().t()                                                # [K, 1]
  b = (a - vd * (vd * a).sum()) / nv.detach()
  f = lambda t: t.detach().double().numpy()
  return dict(w_bar=f(w_bar), u_new=f(u1).reshape(-1), v=f(v).reshape(-1), stats=np.array([float(sigma.detach()), float(nv.detach())]), gw=f(gw),
              sigma=float(sigma.detach()), s=float((g * w.detach()).sum()), b=f(b).reshape(-1))


def sn_bounds(w2, u, G):
  """tg_spectral_norm_fwd / _bwd (csrc/sn.hip): every output ends in a division by a norm and has no product structure, so
  the normaliser convention: e32_bound(ref, E, 'f32') = 2^-24 |ref| + 16 E + 2^-126 with, per output,
      E = max(max |float32 restatement - float64|, 2^-24 max(mag))
  of the literal formulas (sn_formulas) by torch on the CPU.  The floor: the float32 restatement can be EXACT where the
  kernel is not -- for cout = 1, u' = x / sqrt(x^2) is +-1 in any precision while the kernel's rsqrtf is one unit off; for a
  1 x 1 matrix the gradient cancels to exactly 0 in both -- and one fp32 rounding of the largest intermediate is the least
  any fp32 evaluation owes.  mag:
      w_bar, u', v, stats    |ref|
      gw                     the sum of the absolute summands of  G / sigma - (s / sigma^2) (v (x) u' + b (x) u):
                             |G| / sigma + |s| / sigma^2 (|v (x) u'| + |b (x) u|),   s = sum G o W, b = (a - v (v . a)) / |v_raw|
  m = 16 as for the normalisers: torch's float32 sums are pairwise, the kernels' are lane-strided fmaf chains of up to
  cout / 64 (rows) and K / 64 (columns) terms that meet in a butterfly and a two-stage sum in a fixed order.
  The saved v and stats = {sigma, |v_raw|} are checked too: a wrong stats[1] shows only in the b term of the gradient, which
  vanishes at a converged u.
  -> (ref, bound): dicts over w_bar, u_new, v, stats, gw (numpy float64)."""
  import torch
  r64, r32 = sn_formulas(w2, u, G, torch.float64), sn_formulas(w2, u, G, torch.float32)
  sig, s = r64['sigma'], r64['s']
  ud = u.detach().double().numpy().reshape(-1)
  mag = {k: np.abs(r64[k]) for k in ('w_bar', 'u_new', 'v', 'stats')}
  mag['gw'] = np.abs(G.detach().double().numpy()) / abs(sig) + abs(s) / sig ** 2 * (
      np.abs(np.outer(r64['v'], r64['u_new'])) + np.abs(np.outer(r64['b'], ud)))
  bound = {}
  for k in mag:
    E = max(e32(r32[k], r64[k]), U32 * float(mag[k].max()))
    bound[k] = e32_bound(r64[k], E, 'f32')
  return {k: r64[k] for k in mag}, bound


def sn_bwd_closed_form(G, W, u, u_new, v, stats, dt=np.float64):
  """The backward kernel's own closed form from the operands it READS (sn.hip's header comment), numpy dtype `dt`:
      gw = G / sigma - (s / sigma^2) (v (x) u' + b (x) u),  s = sum G o W,  a = W u'^T,  b = (a - v (v . a)) / stats[1]."""
  G, W, u, u_new, v, stats = (np.asarray(x, dt) for x in (G, W, u, u_new, v, stats))
  sigma, nv = stats[0], stats[1]
  a = W @ u_new
  b = (a - v * (v * a).sum(dtype=dt)) / nv
  s = (G * W).sum(dtype=dt)
  return G / sigma - (s / (sigma * sigma)) * (np.outer(v, u_new) + np.outer(b, u))


# ------------------------------------------------------------------------------------------------ the loss tail
def cosine_formulas(e, p, weight, gin, dt):
  """tf.losses.cosine_distance(l2n(expected), l2n(embedding), axis=-1, weights=w) as csrc/reduce.hip documents it, in torch dtype
  `dt` on the CPU: out = (w / B) sum_b (1 - e_b . p_b rsqrt(max(|e_b|^2, 1e-12)) rsqrt(max(|p_b|^2, 1e-12))); the gradient towards
  p by autograd times the incoming gradient `gin` -- the clamp's own derivative is 0, so below it phat = p 1e6 is linear in p.
  -> dict(out, gp [B, D], rows [B] = 1 - cos_b, cos [B]) as numpy float64."""
  import torch
  et, pt = e.detach().to(dt), p.detach().to(dt).clone().requires_grad_(True)
  ie = torch.rsqrt((et * et).sum(1).clamp_min(1e-12))
  ip = torch.rsqrt((pt * pt).sum(1).clamp_min(1e-12))
  cos = (et * pt).sum(1) * ie * ip
  rows = 1.0 - cos
  out = rows.sum() * (weight / e.shape[0])
  gp, = torch.autograd.grad(out * gin, pt)
  f = lambda t: t.detach().double().numpy()
  return dict(out=float(out.detach()), gp=f(gp), rows=f(rows), cos=f(cos))


def cosine_bounds(e, p, weight, gin):
  """cosine_distance_fwd_kernel / _bwd_kernel.  Forward: the b row terms 1 - cos_b, each an operation without product
  structure (three fmaf chains, two rsqrtf) -> e32_bound of a row with E = max(max_b |float32 - float64|, 2^-24 max_b (1 +
  |cos_b|)) (the floor: where p = 3 e the float32 restatement can return exactly 0), summed in row order by one thread (b
  additions) and scaled once: reduction_bound(sum |rows|, L = b + 1, w / B).  Backward, per element: e32_bound with E per row,
  floored at 2^-24 |k| / max(|p_b|, 1e-6), k = w gin / B: the two summands ehat / |p| and phat cos / |p| are each of that
  size and cancel where p is parallel to e.  -> (ref, b_out, b_gp)."""
  import torch
  r64, r32 = cosine_formulas(e, p, weight, gin, torch.float64), cosine_formulas(e, p, weight, gin, torch.float32)
  b = e.shape[0]
  scale = weight / b
  E_row = max(e32(r32['rows'], r64['rows']), U32 * float((1.0 + np.abs(r64['cos'])).max()))
  b_out = abs(scale) * float(e32_bound(r64['rows'], E_row, 'f32').sum()) + reduction_bound(np.abs(r64['rows']).sum(), b + 1, scale)
  pn = np.maximum(np.sqrt((p.detach().double().numpy() ** 2).sum(1)), 1e-6)
  E_g = np.maximum(np.abs(r32['gp'] - r64['gp']).max(1), U32 * abs(scale * gin) / pn)[:, None]
  return r64, b_out, e32_bound(r64['gp'], E_g, 'f32')


def pred_loss_reference(x, mode, a, b):
  """pred_loss_f / pred_loss_df (csrc/reduce.hip) in float64 -> (f, df, |parts| of f summed, term_ops, sigmoid or None):
      mode 1  relu(a + b x)         term_ops 2: the product, the addition (fmaxf is exact); derivative b where a + b x > 0, else
                                    0 -- at a + b x = 0 exactly it is 0, as tf.nn.relu's
      mode 2  max(x, 0) - x a + log1p(exp(-|x|))   term_ops 11: x a (1), the subtraction (1), expf one unit in the last place (2)
                                    carried through log1p (d log1p(t) = dt / (1 + t) <= 2 (2^-24) t <= 4 (2^-24) log1p(t)), log1pf
                                    itself (2), the addition (1)
      mode 3  x^2                   term_ops 1"""
  x = np.asarray(x, np.float64)
  if mode == 1:
    z = a + b * x
    return np.maximum(z, 0.0), np.where(z > 0, b, 0.0), np.maximum(z, 0.0), 2, None
  if mode == 2:
    sp = np.log1p(np.exp(-np.abs(x)))
    sig = np.where(x >= 0, 1.0 / (1.0 + np.exp(-np.abs(x))), np.exp(-np.abs(x)) / (1.0 + np.exp(-np.abs(x))))
    return np.maximum(x, 0.0) - x * a + sp, sig - a, np.maximum(x, 0.0) + np.abs(x * a) + sp, 11, sig
  if mode == 3:
    return x * x, 2.0 * x, x * x, 1, None
  return x, np.ones_like(x), np.abs(x), 0, None


def pred_loss_fwd_bound(parts_sum, n, scale, term_ops, extra_ops=0):
  """One 256-thread workgroup: ceil(n / 256) additions per thread, 6 butterfly levels, the 4 wave partials, the scale
  multiply (+ extra_ops: what a caller's epilogue adds)."""
  return reduction_bound(parts_sum, -(-n // 256) + 6 + 4 + 1 + extra_ops, scale, term_ops)


def pred_loss_bwd_bound(ref, g_abs, sig, ops=4):
  """gx = (gscale scale) df: per element ops 2^-24 |ref| + 2^-126 with the four fp32 operations g = gscale scale (1), df (2 x,
  or b: at most 1), g df (1), and one for the scale's own conversion to float.  Mode 2 needs one more term, by derivation: df =
  sigmoid(x) - label CANCELS where the sigmoid saturates (x = 20, label 1: the float64 difference is 2e-9, the fp32 one 0),
  and the error of the sigmoid itself -- expf (2), 1 + e (1), the division (2), relative to sigmoid(x) -- does not shrink with
  the difference: + 5 2^-24 |g| sigmoid(x)."""
  bnd = ops * U32 * np.abs(ref) + TINY
  return bnd if sig is None else bnd + 5.0 * U32 * g_abs * sig


def dot_chain(numel):
  """tg_dot (csrc/attention.hip): nparts = min(1024, ceil(numel / 16384)) workgroups of per = ceil(numel / nparts) elements:
  ceil(per / 256) fmaf per thread (64 at 16384), 6 + 4 levels of the block sum; dot_final: ceil(nparts / 256) additions per
  thread, 6 + 4 again.  -> (L, nparts, per)."""
  nparts = min(1024, -(-numel // 16384))
  per = -(-numel // nparts)
  return -(-per // 256) + 10 + -(-nparts // 256) + 10, nparts, per


def variance_bound(x, dtype, batch):
  """ops.batch_variance = tg_sum, tg_sample_sumsq, tg_var_from_sums: E[x^2] - E[x]^2, clamped at 0.  The kernel FORMS that
  difference, so no bound relative to the variance can hold (0.9 + 0.01 U: the variance is 1e-5 of E[x^2]); the bound is
  relative to E[x^2]:  (L + 3) 2^-24 E[x^2] + 2^-126,
      L = L_ss + 1 + L_b + 2 L_s:   L_ss the chain of one sample's sum of squares (cap 64; + 1: the fmaf that forms a term), L_b =
      ceil(batch / 256) + 10 the sum over the samples in var_from_sums, L_s the chain of tg_sum (cap 1024) -- twice, for m^2 =
      (sum / n)^2, with mean|x|^2 <= E[x^2];  3: the two multiplies by 1 / numel and the subtraction.
  x: the STORED values (float64 numpy).  -> (var, bound, L)."""
  numel = x.size
  per = numel // batch
  V = 4 if _name(dtype) in ('float32', 'f32') else 8
  L_ss, _ = reduction_chain(per, dtype, 64, vec=(batch == 1 or per % V == 0))
  L_s, _ = reduction_chain(numel, dtype, 1024)
  L = L_ss + 1 + (-(-batch // 256) + 10) + 2 * L_s
  ex2 = float((x * x).mean())
  return max(ex2 - float(x.mean()) ** 2, 0.0), (L + 3) * U32 * ex2 + TINY, L
