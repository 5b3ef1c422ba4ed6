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
