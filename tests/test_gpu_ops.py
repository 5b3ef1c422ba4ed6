"""GPU parity: every HIP operator (through the C ABI) against the oracle on the same seeded inputs.

Tolerances: fp32 kernels vs the float64 oracle: rel-L2 <= 2e-5 (single primitive);
bf16 kernels vs the oracle evaluated on the same bf16-rounded inputs: rel-L2 <= 1e-2 forward,
3e-2 gradients; MFMA bf16 kernels vs the direct bf16 kernels (same rounding, different summation
order): rel-L2 <= 2e-3.

Element-wise parity (the second half of this file and the three dispatch-threshold tests; tests/elementwise.py holds the
formulas and their derivation, DESIGN.md section 2 the table of the worst ratios per operator family, on the MI355X and over
the emulated kernels): every element against its own bound, built from the float64 reference and the inputs only --
  convs            u |ref| + (1 + u) K 2^-24 mag       K summands in fp32, mag the same sum over |operands|
  fp32 gradients   2^-24 |ref| + P 2^-24 mag            P summed pixels
  kernel vs kernel r u max(|a|, |b|) + 2 K 2^-24 mag    whole batch, on the device
  normalisers ...  u |ref| + 16 E32                     E32 = max |float32 restatement - float64| of the literal formula
  pool, upsample^T u |ref| (16-bit); fp32: + 3 2^-24 sum|x|  a sum of four stored values
  streaming ops    u |ref| + (1 + u) ops 2^-24 mag      the kernel's own 1-4 fp32 operations
  copies           array_equal
  flash forward    O: u |ref| + (1 + u) [((u + eps + len 2^-24) (mag + |ref|) + tiny16 (sum|v| + len |ref|)) / (1 - rho) + 2 2^-24 |ref|]
                   lse: -log(1 - rho) + 3 2^-24 (lse - max s + 6 + rho) + 2^-24 |lse|;  eps = ((d_qk + 9) A + 2 + 3 len / 32) 2^-24
  flash backward   u |ref| + R u mag + A 2^-24 mag + 2^-25 S    P, dS packed; the forward's lse and O bounds carried in
  flash 2nd order  the same over the packed maps P, gS, T, U and the statistics D, E, F; magnitudes from the closed form
  batched GEMM     the conv bound with K = k + 1 (alpha) + 1 (accumulate), mag = |alpha| |a| |b| + |C0|
  softmax kernels  u |ref| + 16 E32, each kernel on the operands it reads
  scalar sums      L 2^-24 |scale| sum|terms|            L: the longest chain of additions the launch geometry allows
  Adam             one step in float64 from the fp32 state it reads, each fp32 operation counted; the bf16 shadow bit-exact
  spectral norm    2^-24 |ref| + 16 E, E = max(E32, 2^-24 max(mag)); the multi-kernel launch bit-equal to the one-kernel path
  loss tail        reduction_bound over one workgroup's chain; gradients 4 2^-24 |ref| (+ 5 2^-24 |g| sigmoid for the cross entropy)
  small GEMM, FC   the conv bound with K = k (+ 1 per bias / accumulate); parameter gradients as fp32 gradients with P = m
  tanh, dot        u |ref| + 16 E32; ops 2^-24 mag for the pointwise pieces; tg_dot by its two-stage chain
  preprocessing    u |want| + 3e-6 against oracle.np_ops.preprocess_image, through the C ABI
with u = 2^-8 (bf16), 2^-11 (fp16), 2^-24 (fp32), `+ tiny` everywhere (2^-25 for fp16: half its subnormal spacing), and
every further storage rounding the product path defines named where it is added.  Each check prints
`[elementwise] <family> <dtype> worst ratio <r>` (run with -s).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import np_ops as N          # noqa: E402  (checker only)
from oracle import torch_ref as R       # noqa: E402

F32_TOL = 2e-5
BF16_FWD_TOL = 1e-2
BF16_GRAD_TOL = 3e-2
MFMA_VS_DIRECT_TOL = 2e-3


def dev():
  return torch.device('cuda:0')


def rel_l2(a, b):
  a = np.asarray(a, np.float64)
  b = np.asarray(b, np.float64)
  assert a.shape == b.shape, (a.shape, b.shape)
  return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))


def to_dev(a, dtype=torch.float32):
  return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev()).to(dtype).contiguous()


def host(t):
  return t.detach().float().cpu().numpy().astype(np.float64)


def bf16_round(a):
  return torch.from_numpy(np.asarray(a, np.float32)).to(torch.bfloat16).float().numpy().astype(np.float64)


def tol_for(dtype, grad=False):
  if dtype == torch.float32:
    return F32_TOL
  return BF16_GRAD_TOL if grad else BF16_FWD_TOL


# ---------------------------------------------------------------------------------------------- element-wise bookkeeping
import functools            # noqa: E402
import zlib                  # noqa: E402
import elementwise as E      # noqa: E402

EW_DTYPES = {'f32': torch.float32, 'bf16': torch.bfloat16, 'f16': torch.float16}
EW_WORST = {}      # operator family -> dtype -> worst ratio seen in this session (printed with -s: the table of DESIGN.md)


def _ew_note(family, dname, ratio):
  d = EW_WORST.setdefault(family, {})
  d[dname] = max(d.get(dname, 0.0), float(ratio))
  print('[elementwise] %-28s %-4s worst ratio %.3f' % (family, dname, ratio))


def _ew_dname(dtype):
  return {torch.float32: 'f32', torch.bfloat16: 'bf16', torch.float16: 'f16'}[dtype]


def _with_middle(sel, key, lo, hi):
  """sel plus one image of lo + 1 .. hi - 2, seeded by the case: the images a first / last check never meets."""
  return sorted(set(sel) | ({lo + 1 + zlib.crc32(key.encode()) % (hi - lo - 2)} if hi - lo > 2 else set()))


def _twice(ref, slope, dtype):
  """Where a mask is applied to a STORED tensor (capi.hip: "the plain conv, then the mask in place") the masked value is
  stored again: a second rounding, u |ref|, of the elements whose slope is not 1."""
  u = E.unit_roundoff(dtype)
  return (1 + u) * (u * np.abs(ref) + E.tiny(dtype)) * (slope != 1.0)


@pytest.fixture(scope='module')
def ops():
  from twingan_amd import ops as _ops
  return _ops


@pytest.fixture
def record_calls():
  """-> the list of (entry point, args) of every library call made while the test runs."""
  import twingan_amd.ops as O
  real, seen = O.call, []

  def spy(name, *a, **kw):
    seen.append((name, a))
    return real(name, *a, **kw)
  O.call = spy
  yield seen
  O.call = real


# ---------------------------------------------------------------------------------------------- conv
CONV_CASES = [
    # n, h, w, cin, cout, k, padding
    (2, 6, 6, 5, 7, 3, 'SAME'),
    (1, 9, 5, 3, 4, 3, 'SAME'),
    (2, 5, 5, 4, 6, 1, 'SAME'),
    (3, 4, 4, 5, 6, 4, 'VALID'),
    (2, 7, 7, 3, 5, 4, 'VALID'),
    (2, 8, 8, 16, 16, 3, 'SAME'),
]


@pytest.mark.parametrize('n,h,w,cin,cout,k,padding', CONV_CASES)
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_conv_direct_vs_oracle(ops, n, h, w, cin, cout, k, padding, dtype):
  rng = np.random.RandomState(1)
  x = rng.randn(n, h, w, cin)
  wt = rng.randn(k, k, cin, cout) / np.sqrt(k * k * cin)
  b = rng.randn(cout) * 0.1
  if dtype == torch.bfloat16:
    x, wr = bf16_round(x), bf16_round(wt)
  else:
    wr = wt
  import twingan_amd.ops as O
  saved = O._mfma_ok
  O._mfma_ok = lambda *a: False          # force the direct algorithm
  try:
    xd = to_dev(x, dtype).requires_grad_(True)
    wd = to_dev(wt).requires_grad_(True)
    bd = to_dev(b).requires_grad_(True)
    y = ops.conv2d(xd, wd, bd, k, padding, lrelu=True)
    ref = N.leaky_relu(N.conv2d(x, wr, padding) + b)
    assert rel_l2(host(y), ref) < tol_for(dtype)
    gy = rng.randn(*ref.shape)
    if dtype == torch.bfloat16:
      gy = bf16_round(gy)
    y.backward(to_dev(gy, dtype))
    gpre = gy * np.where(ref > 0, 1.0, 0.2)
    if dtype == torch.bfloat16:
      gpre = bf16_round(gpre)
    assert rel_l2(host(xd.grad), N.conv2d_bwd_data(gpre, wr, (h, w), padding)) < tol_for(dtype, True)
    assert rel_l2(host(wd.grad), N.conv2d_bwd_weight(x, gpre, (k, k), padding)) < tol_for(dtype, True)
    assert rel_l2(host(bd.grad), gpre.sum(axis=(0, 1, 2))) < tol_for(dtype, True)
  finally:
    O._mfma_ok = saved


MFMA_CASES = [
    # n, h, w, cin, cout, k, padding    (model layer shapes at reduced extent + ragged tiles)
    (2, 16, 16, 16, 16, 3, 'SAME'),
    (2, 16, 16, 16, 32, 3, 'SAME'),
    (1, 32, 32, 32, 64, 3, 'SAME'),
    (2, 8, 8, 64, 128, 3, 'SAME'),
    (2, 8, 8, 128, 256, 3, 'SAME'),
    (3, 4, 4, 256, 256, 3, 'SAME'),
    (2, 8, 8, 512, 256, 3, 'SAME'),
    (1, 16, 16, 256, 64, 3, 'SAME'),
    (1, 32, 32, 64, 16, 3, 'SAME'),
    (2, 16, 16, 128, 128, 3, 'SAME'),
    (2, 16, 32, 256, 256, 3, 'SAME'),
    (5, 4, 4, 264, 256, 3, 'SAME'),      # D tail conv after minibatch-stddev padding
    (5, 4, 4, 64, 64, 4, 'VALID'),       # dense rewrite of the 4x4 VALID conv
    (16, 4, 4, 256, 256, 4, 'VALID'),
    (1, 20, 12, 24, 40, 3, 'SAME'),      # ragged spatial tiles, channels not multiples of 16/32
    (3, 10, 18, 8, 8, 3, 'SAME'),
    (2, 12, 12, 32, 48, 1, 'SAME'),      # generic 1x1
    (1, 40, 24, 16, 16, 3, 'SAME'),
]


@pytest.mark.parametrize('n,h,w,cin,cout,k,padding', MFMA_CASES)
def test_conv_mfma_vs_direct_and_oracle(ops, n, h, w, cin, cout, k, padding):
  import twingan_amd.ops as O
  rng = np.random.RandomState(2)
  x = bf16_round(rng.randn(n, h, w, cin))
  wt = rng.randn(k, k, cin, cout) / np.sqrt(k * k * cin)
  b = rng.randn(cout) * 0.1
  spec = O.ConvSpec(k, padding)
  assert O._mfma_ok(torch.bfloat16, cin, cout, spec, h, w)
  res = {}
  for algo in ('mfma', 'direct'):
    saved = O._mfma_ok
    if algo == 'direct':
      O._mfma_ok = lambda *a: False
    try:
      xd = to_dev(x, torch.bfloat16).requires_grad_(True)
      wd = to_dev(wt).requires_grad_(True)
      bd = to_dev(b).requires_grad_(True)
      with torch.no_grad():
        y = ops.conv2d(xd, wd, bd, k, padding, lrelu=True)
      # gradients through the linear part only: with LeakyReLU the two algorithms' 1-ulp differences in z flip
      # masks near zero, which at 16 pixels (the dense 4x4 VALID case) moves gw by several percent
      y_lin = ops.conv2d(xd, wd, bd, k, padding, lrelu=False)
      gy = bf16_round(np.random.RandomState(3).randn(*y.shape))
      y_lin.backward(to_dev(gy, torch.bfloat16))
      res[algo] = (host(y), host(xd.grad), host(wd.grad), host(bd.grad))
    finally:
      O._mfma_ok = saved
  names = ('y', 'gx', 'gw', 'gb')
  for i, nm in enumerate(names):
    e = rel_l2(res['mfma'][i], res['direct'][i])
    assert e < MFMA_VS_DIRECT_TOL, '%s mfma vs direct rel-L2 %.3e' % (nm, e)
  ref = N.leaky_relu(N.conv2d(x, bf16_round(wt), padding) + b)
  assert rel_l2(res['mfma'][0], ref) < BF16_FWD_TOL


def test_conv_mfma_transpose_detecting(ops):
  """A = identity-like weights with an ASYMMETRIC pattern catch swapped rows/cols or flipped taps."""
  cin = cout = 32
  x = np.zeros((1, 8, 8, cin))
  x[0, 2, 5, 3] = 1.0
  x[0, 6, 1, 17] = 2.0
  w = np.zeros((3, 3, cin, cout))
  w[0, 2, 3, 9] = 1.0        # tap (dy=-1, dx=+1): out[y, x] += in[y-1, x+1]
  w[2, 1, 17, 30] = 0.5      # tap (dy=+1, dx=0)
  y = ops.conv2d(to_dev(x, torch.bfloat16), to_dev(w), None, 3, 'SAME')
  ref = N.conv2d(x, w)
  assert np.array_equal(host(y), ref)
  assert host(y)[0, 3, 4, 9] == 1.0 and host(y)[0, 5, 1, 30] == 1.0


def test_conv_double_backward_matches_oracle(ops):
  """Second-order path used by WGAN-GP: d/dw of ||d conv / d x||^2."""
  rng = np.random.RandomState(4)
  x = rng.randn(2, 6, 6, 4)
  w = rng.randn(3, 3, 4, 5) * 0.3
  xd = to_dev(x).requires_grad_(True)
  wd = to_dev(w).requires_grad_(True)
  y = ops.conv2d(xd, wd, None, 3, 'SAME', lrelu=True)
  gx, = torch.autograd.grad(y, xd, grad_outputs=torch.ones_like(y), create_graph=True)
  pen = ops.gradient_penalty(gx.contiguous(), 10.0)
  pen.backward()
  xt = torch.from_numpy(x).requires_grad_(True)
  wt = torch.from_numpy(w).requires_grad_(True)
  yt = R.leaky_relu(R.conv2d(xt, wt, 'SAME'))
  gxt, = torch.autograd.grad(yt.sum(), xt, create_graph=True)
  pt = ((torch.sqrt((gxt ** 2).sum(dim=(1, 2, 3))) - 1) ** 2).mean() * 10.0
  pt.backward()
  assert abs(pen.item() - pt.item()) < 1e-4 * abs(pt.item())
  assert rel_l2(host(wd.grad), wt.grad.numpy()) < 1e-4


# ---------------------------------------------------------------------------------------------- rgb 1x1
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('cin,cout', [(3, 16), (3, 256), (16, 3), (256, 3), (3, 12), (20, 3)])
def test_pointwise_conv(ops, dtype, cin, cout):
  rng = np.random.RandomState(5)
  x = rng.randn(3, 7, 5, cin)
  w = rng.randn(1, 1, cin, cout) / np.sqrt(cin)
  b = rng.randn(cout) * 0.1
  if dtype == torch.bfloat16:
    x, wr = bf16_round(x), bf16_round(w)
  else:
    wr = w
  xd, wd, bd = to_dev(x, dtype).requires_grad_(True), to_dev(w).requires_grad_(True), to_dev(b).requires_grad_(True)
  y = ops.pointwise_conv(xd, wd, bd, lrelu=True)
  ref = N.leaky_relu(x @ wr[0, 0] + b)
  assert rel_l2(host(y), ref) < tol_for(dtype)
  gy = rng.randn(*ref.shape)
  if dtype == torch.bfloat16:
    gy = bf16_round(gy)
  y.backward(to_dev(gy, dtype))
  gpre = gy * np.where(ref > 0, 1.0, 0.2)
  if dtype == torch.bfloat16:
    gpre = bf16_round(gpre)
  assert rel_l2(host(xd.grad), gpre @ wr[0, 0].T) < tol_for(dtype, True)
  assert rel_l2(host(wd.grad)[0, 0], np.einsum('nhwc,nhwo->co', x, gpre)) < tol_for(dtype, True)
  assert rel_l2(host(bd.grad), gpre.sum(axis=(0, 1, 2))) < tol_for(dtype, True)


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize('n,hw,cs,cb,small_in', [(2, 64, 3, 16, True), (16, 256, 3, 16, True), (3, 32, 3, 256, True),
                                                   (2, 64, 3, 16, False), (1, 6, 3, 16, True), (2, 8, 4, 16, True)])
def test_pointwise_rgb_filter_and_bias_gradient(ops, dtype, n, hw, cs, cb, small_in):
  """tg_pointwise_conv_bwd_weight(_bias) at the fromRGB / toRGB shapes (nets/pggan.py:233-240,176-200): the four-pixel RGB
  kernel (16-bit, 3 small channels, npix % 4 == 0; incl. the bench shape 16 x 256 x 256 x 3 -> 16) and the generic one,
  filter gradient with and without the bias gradient riding along, written and accumulated, against float64 sums of the
  same (rounded) inputs."""
  from twingan_amd import ops as O
  g = torch.Generator(device='cpu').manual_seed(7)
  small = torch.randn(n, hw, hw, cs, generator=g).to(dtype)
  big = torch.randn(n, hw, hw, cb, generator=g).to(dtype)
  x, gy = (small, big) if small_in else (big, small)
  cin, cout = x.shape[-1], gy.shape[-1]
  ref_w = np.einsum('pc,po->co', host(x).reshape(-1, cin), host(gy).reshape(-1, cout))
  ref_b = host(gy).reshape(-1, cout).sum(axis=0)
  xd, gyd = x.to(dev()), gy.to(dev())
  npix = n * hw * hw
  tol = 2e-5 if dtype == torch.float32 else 2e-4      # fp32 accumulation of exactly representable products
  for accumulate in (0, 1):
    gw = torch.full((cin, cout), 3.0 if accumulate else float('nan'), device=dev())
    O.call('tg_pointwise_conv_bwd_weight', xd.data_ptr(), gyd.data_ptr(), gw.data_ptr(), npix, cin, cout, accumulate,
           O._dt(xd), O._stream())
    assert rel_l2(host(gw) - (3.0 if accumulate else 0.0), ref_w) < tol
    if small_in:
      gw = torch.full((cin, cout), 3.0 if accumulate else float('nan'), device=dev())
      gb = torch.full((cout,), -2.0 if accumulate else float('nan'), device=dev())
      O.call('tg_pointwise_conv_bwd_weight_bias', xd.data_ptr(), gyd.data_ptr(), gw.data_ptr(), gb.data_ptr(), npix, cin, cout,
             accumulate, O._dt(xd), O._stream())
      assert rel_l2(host(gw) - (3.0 if accumulate else 0.0), ref_w) < tol
      assert rel_l2(host(gb) + (2.0 if accumulate else 0.0), ref_b) < tol


def test_pointwise_conv_bias_gradient_rides_in_the_filter_gradient(ops):
  """The discriminator's fromRGB under a trainer-style gradient sink: one tg_pointwise_conv_bwd_weight_bias launch instead of
  the filter gradient + a channel-sum pass -- same sums as the unfused autograd path."""
  from twingan_amd import ops as O
  g = torch.Generator(device='cpu').manual_seed(8)
  x = torch.randn(2, 32, 32, 3, generator=g).to(dev()).to(torch.bfloat16)
  w = (torch.randn(1, 1, 3, 16, generator=g) * 0.5).to(dev()).requires_grad_(True)
  b = (torch.randn(16, generator=g) * 0.1).to(dev()).requires_grad_(True)
  gy = torch.randn(2, 32, 32, 16, generator=g).to(dev()).to(torch.bfloat16)
  y = ops.pointwise_conv(x, w, b, lrelu=True)
  y.backward(gy)
  gw_ref, gb_ref = w.grad.clone(), b.grad.clone()
  sw, sb = torch.zeros_like(w), torch.zeros_like(b)
  O.GradSink.register(w, sw)
  O.GradSink.register(b, sb)
  try:
    y = ops.pointwise_conv(x, w, b, lrelu=True)
    y.grad_fn.tg_premasked = True      # as when the consumer conv's backward-data applied the LeakyReLU mask
    z = y.detach()
    gpre = (gy.float() * torch.where(z.float() > 0, 1.0, 0.2)).to(torch.bfloat16)
    torch.autograd.backward(y, gpre)
  finally:
    O.GradSink.unregister(w)
    O.GradSink.unregister(b)
  assert rel_l2(host(sw), host(gw_ref)) < 2e-3      # gpre is re-rounded to bf16 here, not in the unfused path
  assert rel_l2(host(sb), host(gb_ref)) < 2e-3


# ---------------------------------------------------------------------------------------------- norm_act
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('n,h,w,c,lrelu,pn', [(2, 8, 8, 16, True, True), (3, 4, 4, 256, True, True),
                                              (2, 16, 16, 32, True, False), (2, 8, 8, 3, False, False),
                                              (1, 32, 32, 64, True, True), (2, 5, 7, 8, True, True)])
def test_norm_act(ops, dtype, n, h, w, c, lrelu, pn):
  rng = np.random.RandomState(6)
  y = rng.randn(n, h, w, c) * 1.5 + 0.7
  gamma = 1.0 + 0.2 * rng.randn(c)
  beta = 0.1 * rng.randn(c)
  gz = rng.randn(n, h, w, c)
  if dtype == torch.bfloat16:
    y, gz = bf16_round(y), bf16_round(gz)
  yd = to_dev(y, dtype).requires_grad_(True)
  gd, bd = to_dev(gamma).requires_grad_(True), to_dev(beta).requires_grad_(True)
  z = ops.norm_act(yd, gd, bd, lrelu=lrelu, pixel_norm=pn)
  z.backward(to_dev(gz, dtype))
  yt = torch.from_numpy(y).requires_grad_(True)
  gt = torch.from_numpy(gamma).requires_grad_(True)
  bt = torch.from_numpy(beta).requires_grad_(True)
  zt = R.instance_norm(yt, gt, bt)
  if lrelu:
    zt = R.leaky_relu(zt)
  if pn:
    zt = R.pixel_norm(zt)
  zt.backward(torch.from_numpy(gz))
  assert rel_l2(host(z), zt.detach().numpy()) < tol_for(dtype)
  assert rel_l2(host(yd.grad), yt.grad.numpy()) < tol_for(dtype, True)
  assert rel_l2(host(gd.grad), gt.grad.numpy()) < tol_for(dtype, True)
  assert rel_l2(host(bd.grad), bt.grad.numpy()) < tol_for(dtype, True)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('n,h,w,c,lrelu,pn,pool,split', [(2, 8, 8, 16, True, True, False, None), (3, 4, 4, 256, True, True, False, 1),
                                                        (2, 16, 16, 32, True, False, True, None), (2, 8, 8, 3, False, False, False, None),
                                                        (4, 32, 32, 64, True, True, True, 2), (2, 5, 7, 8, True, True, False, None)])
def test_layer_norm_act(ops, dtype, n, h, w, c, lrelu, pn, pool, split):
  """ops.layer_norm_act = tf.contrib.layers.layer_norm (statistics of one image over (H, W, C), gamma / beta per channel,
  epsilon 1e-12; nets/pggan_utils.py:189-197) + LeakyReLU + pixel norm (+ the 2x2 pool), with per-domain parameters
  (images [split, n) use the second pair).  Outputs and all gradients against the same composition in float64."""
  rng = np.random.RandomState(61)
  y = rng.randn(n, h, w, c) * 1.5 + 0.7 + 0.5 * rng.randn(1, 1, 1, c)
  gam = [1.0 + 0.2 * rng.randn(c) for _ in range(2)]
  bet = [0.1 * rng.randn(c) for _ in range(2)]
  gz = rng.randn(n, h, w, c)
  gzp = rng.randn(n, h // 2, w // 2, c)
  if dtype == torch.bfloat16:
    y, gz, gzp = bf16_round(y), bf16_round(gz), bf16_round(gzp)
  yd = to_dev(y, dtype).requires_grad_(True)
  gd = [to_dev(g).requires_grad_(True) for g in gam]
  bd = [to_dev(b).requires_grad_(True) for b in bet]
  two = split is not None
  out = ops.layer_norm_act(yd, gd[0], bd[0], lrelu=lrelu, pixel_norm=pn, pool=pool, gamma2=gd[1] if two else None,
                           beta2=bd[1] if two else None, split=split)
  yt = torch.from_numpy(y).requires_grad_(True)
  gt = [torch.from_numpy(g).requires_grad_(True) for g in gam]
  bt = [torch.from_numpy(b).requires_grad_(True) for b in bet]
  mean = yt.mean(dim=(1, 2, 3), keepdim=True)
  var = ((yt - mean) ** 2).mean(dim=(1, 2, 3), keepdim=True)
  sel = (torch.arange(n) >= (split if two else n)).view(n, 1, 1, 1)
  zt = (yt - mean) * torch.rsqrt(var + 1e-12) * torch.where(sel, gt[1], gt[0]) + torch.where(sel, bt[1], bt[0])
  if lrelu:
    zt = R.leaky_relu(zt)
  if pn:
    zt = R.pixel_norm(zt)
  if pool:
    z, zp = out
    ztp = R.avg_pool2(zt)
    torch.autograd.backward([z, zp], [to_dev(gz, dtype), to_dev(gzp, dtype)])
    torch.autograd.backward([zt, ztp], [torch.from_numpy(gz), torch.from_numpy(gzp)])
    assert rel_l2(host(zp), ztp.detach().numpy()) < tol_for(dtype)
  else:
    z = out
    z.backward(to_dev(gz, dtype))
    zt.backward(torch.from_numpy(gz))
  assert rel_l2(host(z), zt.detach().numpy()) < tol_for(dtype)
  assert rel_l2(host(yd.grad), yt.grad.numpy()) < tol_for(dtype, True)
  for i in range(2 if two else 1):
    assert rel_l2(host(gd[i].grad), gt[i].grad.numpy()) < tol_for(dtype, True), i
    assert rel_l2(host(bd[i].grad), bt[i].grad.numpy()) < tol_for(dtype, True), i


def test_instance_norm_large_mean_is_stable(ops):
  """Shifted-sum statistics: a large common offset must not destroy the variance in fp32."""
  rng = np.random.RandomState(7)
  y = rng.randn(1, 64, 64, 8) * 0.01 + 100.0
  z = ops.norm_act(to_dev(y), to_dev(np.ones(8)), to_dev(np.zeros(8)), lrelu=False, pixel_norm=False)
  ref = N.instance_norm(np.asarray(to_dev(y).cpu().numpy(), np.float64), 1.0, 0.0)
  assert rel_l2(host(z), ref) < 1e-3


# ---------------------------------------------------------------------------------------------- resampling
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('c0,c1', [(8, 8), (16, 0), (3, 0), (256, 256), (5, 3)])
def test_upsample_concat(ops, dtype, c0, c1):
  rng = np.random.RandomState(8)
  x0 = rng.randn(2, 3, 5, c0)
  x1 = rng.randn(2, 6, 10, c1) if c1 else None
  if dtype == torch.bfloat16:
    x0 = bf16_round(x0)
    x1 = bf16_round(x1) if c1 else None
  else:                                   # exact-copy check: start from fp32-representable values
    x0 = x0.astype(np.float32).astype(np.float64)
    x1 = x1.astype(np.float32).astype(np.float64) if c1 else None
  a = to_dev(x0, dtype).requires_grad_(True)
  b = to_dev(x1, dtype).requires_grad_(True) if c1 else None
  out = ops.upsample2x_concat(a, b)
  ref = N.upsample2x(x0)
  if c1:
    ref = np.concatenate([ref, x1], axis=3)
  assert np.array_equal(host(out), ref)
  go = rng.randn(*ref.shape)
  go = bf16_round(go) if dtype == torch.bfloat16 else go.astype(np.float32).astype(np.float64)
  out.backward(to_dev(go, dtype))
  g0 = go[..., :c0].reshape(2, 3, 2, 5, 2, c0).sum(axis=(2, 4))
  assert rel_l2(host(a.grad), g0) < tol_for(dtype)
  if c1:
    assert np.array_equal(host(b.grad), go[..., c0:])


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('c', [16, 3, 256])
def test_avg_pool_and_double_backward(ops, dtype, c):
  rng = np.random.RandomState(9)
  x = rng.randn(2, 6, 8, c)
  if dtype == torch.bfloat16:
    x = bf16_round(x)
  xd = to_dev(x, dtype).requires_grad_(True)
  y = ops.avg_pool2(xd)
  assert rel_l2(host(y), N.avg_pool2(x)) < tol_for(dtype)
  gy = rng.randn(*y.shape)
  if dtype == torch.bfloat16:
    gy = bf16_round(gy)
  gyd = to_dev(gy, dtype).requires_grad_(True)
  gx, = torch.autograd.grad(y, xd, grad_outputs=gyd, create_graph=True)
  assert rel_l2(host(gx), N.upsample2x(gy) * 0.25) < tol_for(dtype)
  v = rng.randn(*x.shape)
  if dtype == torch.bfloat16:
    v = bf16_round(v)
  ggy, = torch.autograd.grad(gx, gyd, grad_outputs=to_dev(v, dtype))
  assert rel_l2(host(ggy), N.avg_pool2(v)) < tol_for(dtype)       # adjoint of the adjoint


def test_lerp_and_cast(ops):
  rng = np.random.RandomState(10)
  a, b = rng.randn(2, 4, 4, 6), rng.randn(2, 4, 4, 6)
  ad, bd = to_dev(a).requires_grad_(True), to_dev(b).requires_grad_(True)
  out = ops.lerp(ad, bd, 0.3)
  assert rel_l2(host(out), N.lerp(a, b, 0.3)) < F32_TOL
  out.backward(torch.ones_like(out))
  assert rel_l2(host(ad.grad), np.full(a.shape, 0.3)) < F32_TOL
  assert rel_l2(host(bd.grad), np.full(a.shape, 0.7)) < F32_TOL
  c = ops.cast(to_dev(a), torch.bfloat16)
  assert c.dtype == torch.bfloat16 and np.array_equal(host(c), bf16_round(a))


# ---------------------------------------------------------------------------------------------- mbstd
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('n,c', [(5, 8), (16, 256), (3, 32)])
def test_mbstd_fwd_bwd_bwdbwd(ops, dtype, n, c):
  from twingan_amd.params import mbstd_cpad
  rng = np.random.RandomState(11)
  x = rng.randn(n, 4, 4, c)
  if dtype == torch.bfloat16:
    x = bf16_round(x)
  cpad = mbstd_cpad(c)
  xd = to_dev(x, dtype).requires_grad_(True)
  out = ops.minibatch_state_concat(xd, cpad)
  assert out.shape == (n, 4, 4, cpad)
  eps = 1e-8 if dtype == torch.float32 else 1e-6
  ref = N.minibatch_state_concat(x, eps)
  assert rel_l2(host(out)[..., :c + 1], ref) < tol_for(dtype)
  assert np.all(host(out)[..., c + 1:] == 0)
  # first + second order vs torch autograd on the oracle
  go = rng.randn(n, 4, 4, cpad)
  v = rng.randn(n, 4, 4, c)
  if dtype == torch.bfloat16:
    go, v = bf16_round(go), bf16_round(v)
  god = to_dev(go, dtype).requires_grad_(True)
  gx, = torch.autograd.grad(out, xd, grad_outputs=god, create_graph=True)
  ggo, gx2 = torch.autograd.grad(gx, [god, xd], grad_outputs=to_dev(v, dtype))

  xt = torch.from_numpy(x).requires_grad_(True)
  got = torch.from_numpy(go[..., :c + 1].copy()).requires_grad_(True)
  mean = xt.mean(dim=0, keepdim=True)
  std = torch.sqrt(((xt - mean) ** 2).mean(dim=0, keepdim=True) + eps)
  outt = torch.cat([xt, std.mean().reshape(1, 1, 1, 1).expand(n, 4, 4, 1)], dim=3)
  gxt, = torch.autograd.grad(outt, xt, grad_outputs=got, create_graph=True)
  ggot, gx2t = torch.autograd.grad(gxt, [got, xt], grad_outputs=torch.from_numpy(v))
  gtol = tol_for(dtype, True)
  assert rel_l2(host(gx), gxt.detach().numpy()) < gtol
  assert rel_l2(host(ggo)[..., :c + 1], ggot.numpy()) < gtol
  if dtype == torch.float32:
    assert rel_l2(host(gx2), gx2t.numpy()) < gtol
  else:      # 16-bit second order: every element within u |ref| + 16 E32 (tests/elementwise.py) where a rel-L2 of 0.1 stood
    r32 = E.mbstd_reference(torch.from_numpy(x), torch.from_numpy(go[..., :c + 1].copy()), torch.from_numpy(v), 1, eps, torch.float32)
    ref = gx2t.numpy()
    E.assert_elementwise(host(gx2), ref, E.e32_bound(ref, E.e32(r32[3], ref), dtype), 'mbstd n%d c%d second-order gx2' % (n, c))


# ---------------------------------------------------------------------------------------------- dense, losses
def test_fully_connected_and_grads(ops):
  """layers.fully_connected: (a) inside ops.second_order() -- the gradient-penalty pass -- the twice-differentiable
  composition (cast, GEMM, bias add); (b) in first-order passes ONE launch each way (tg_fc_fwd / tg_fc_bwd: FcFn), with
  the parameter gradients written or, under gradient sinks, added in place; fp32 and 16-bit features."""
  rng = np.random.RandomState(12)
  x, w, b = rng.randn(6, 40), rng.randn(40, 3), rng.randn(3)
  xd, wd, bd = to_dev(x).requires_grad_(True), to_dev(w).requires_grad_(True), to_dev(b).requires_grad_(True)
  with ops.second_order():
    y = ops.fully_connected(xd, wd, bd)
  assert rel_l2(host(y), N.fully_connected(x, w, b)) < F32_TOL
  g = rng.randn(6, 3)
  gx, = torch.autograd.grad(y, xd, grad_outputs=to_dev(g), create_graph=True)
  assert rel_l2(host(gx), g @ w.T) < F32_TOL
  v = rng.randn(6, 40)
  (gx * to_dev(v)).sum().backward()            # d/dw of <v, g w^T> = v^T g
  assert rel_l2(host(wd.grad), v.T @ g) < F32_TOL
  # (b) first order
  for dtype in (torch.float32, torch.bfloat16):
    xr = bf16_round(x) if dtype == torch.bfloat16 else x
    xd = to_dev(xr, dtype).requires_grad_(True)
    wd, bd = to_dev(w).requires_grad_(True), to_dev(b).requires_grad_(True)
    y = ops.fully_connected(xd, wd, bd)
    assert type(y.grad_fn).__name__ == 'FcFnBackward' and y.dtype == torch.float32
    assert rel_l2(host(y), N.fully_connected(xr, w, b)) < F32_TOL
    y.backward(to_dev(g))
    assert rel_l2(host(xd.grad), g @ w.T) < tol_for(dtype, True)
    assert rel_l2(host(wd.grad), xr.T @ g) < F32_TOL and rel_l2(host(bd.grad), g.sum(0)) < F32_TOL
    # gradient sinks: added into the caller's buffers, twice
    ops.GradSink.clear()
    ws, bs = torch.ones_like(wd), torch.ones_like(bd)
    ops.GradSink.register(wd, ws)
    ops.GradSink.register(bd, bs)
    wd.grad = bd.grad = None
    for _ in range(2):
      ops.fully_connected(xd, wd, bd).backward(to_dev(g))
    ops.GradSink.clear()
    assert wd.grad is None and bd.grad is None
    assert rel_l2(host(ws), 1.0 + 2.0 * (xr.T @ g)) < F32_TOL and rel_l2(host(bs), 1.0 + 2.0 * g.sum(0)) < F32_TOL


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_losses(ops, dtype):
  rng = np.random.RandomState(13)
  a, b = rng.rand(2, 8, 8, 3), rng.rand(2, 8, 8, 3)
  if dtype == torch.bfloat16:
    a, b = bf16_round(a), bf16_round(b)
  ad, bd = to_dev(a, dtype).requires_grad_(True), to_dev(b, dtype).requires_grad_(True)
  l1 = ops.abs_diff_mean(ad, bd, 0.1)
  assert abs(l1.item() - N.absolute_difference(a, b, 0.1)) < 1e-6
  (l1 * 3.0).backward()
  assert rel_l2(host(ad.grad), 0.3 * np.sign(a - b) / a.size) < tol_for(dtype)
  assert rel_l2(host(bd.grad), -0.3 * np.sign(a - b) / a.size) < tol_for(dtype)
  p = rng.randn(7, 1)
  pd = to_dev(p).requires_grad_(True)
  m = ops.mean(pd, -1.0)
  assert abs(m.item() - N.wgan_g_loss(p)) < 1e-6
  m.backward()
  assert rel_l2(host(pd.grad), np.full(p.shape, -1.0 / 7)) < F32_TOL
  g = rng.randn(4, 8, 8, 3) * 0.05
  if dtype == torch.bfloat16:
    g = bf16_round(g)
  gd = to_dev(g, dtype).requires_grad_(True)
  gp = ops.gradient_penalty(gd, 10.0)
  assert abs(gp.item() - N.gradient_penalty(g, 10.0)) < 1e-4 * N.gradient_penalty(g, 10.0)
  gp.backward()
  gt = torch.from_numpy(g).requires_grad_(True)
  (((torch.sqrt((gt ** 2).sum(dim=(1, 2, 3))) - 1) ** 2).mean() * 10.0).backward()
  assert rel_l2(host(gd.grad), gt.grad.numpy()) < tol_for(dtype, True)


def test_gp_unit_linear_critic_is_zero(ops):
  w = np.random.RandomState(14).randn(4, 4, 3)
  w /= np.linalg.norm(w)
  g = np.tile(w[None], (5, 1, 1, 1))
  assert ops.gradient_penalty(to_dev(g), 10.0).item() < 1e-10


def test_sample_lerp(ops):
  rng = np.random.RandomState(15)
  x, y, a = rng.rand(4, 8, 8, 3), rng.rand(4, 8, 8, 3), rng.rand(4)
  out = ops.sample_lerp(to_dev(x), to_dev(y), to_dev(a))
  assert rel_l2(host(out), x + a[:, None, None, None] * (y - x)) < F32_TOL


def test_adam_kernel_tf_semantics():
  from twingan_amd._lib import call
  rng = np.random.RandomState(16)
  th, g = rng.randn(1000), rng.randn(1000)
  m, v = np.zeros(1000), np.zeros(1000)
  thd, md, vd = to_dev(th), to_dev(m), to_dev(v)
  for t in (1, 2, 3):
    g = rng.randn(1000)
    lr_t = 1e-4 * np.sqrt(1 - 0.99 ** t) / (1 - 0.5 ** t)
    call('tg_adam_step', thd.data_ptr(), to_dev(g).data_ptr(), md.data_ptr(), vd.data_ptr(), None, 1000, float(lr_t),
         None, 0.5, 0.99, 1e-8, 1.0, torch.cuda.current_stream().cuda_stream)
    th, m, v = N.adam_step(th, g, m, v, t)
  assert rel_l2(host(thd), th) < 1e-6
  assert rel_l2(host(md), m) < 1e-5 and rel_l2(host(vd), v) < 1e-5


def test_adam_device_tick_matches_host_schedule():
  """tg_adam_tick: the shared step counter and bias-corrected rate kept on the device (graph replay)."""
  from twingan_amd._lib import call
  rng = np.random.RandomState(17)
  th = rng.randn(512)
  m, v = np.zeros(512), np.zeros(512)
  thd, md, vd = to_dev(th), to_dev(m), to_dev(v)
  step = torch.zeros(1, dtype=torch.int64, device='cuda:0')
  lr_t = torch.zeros(1, dtype=torch.float32, device='cuda:0')
  st = torch.cuda.current_stream().cuda_stream
  for t in (1, 2, 3, 4):
    g = rng.randn(512)
    call('tg_adam_tick', step.data_ptr(), lr_t.data_ptr(), 1e-4, 0.5, 0.99, st)
    call('tg_adam_step', thd.data_ptr(), to_dev(g).data_ptr(), md.data_ptr(), vd.data_ptr(), None, 512, 0.0,
         lr_t.data_ptr(), 0.5, 0.99, 1e-8, 1.0, st)
    th, m, v = N.adam_step(th, g, m, v, t)
    assert int(step.item()) == t
    assert abs(lr_t.item() - 1e-4 * np.sqrt(1 - 0.99 ** t) / (1 - 0.5 ** t)) < 1e-10
  assert rel_l2(host(thd), th) < 1e-6


def test_errors_are_loud(ops):
  from twingan_amd._lib import TgError
  with pytest.raises(TgError):
    ops.conv2d(torch.zeros(1, 4, 4, 4), torch.zeros(3, 3, 4, 4))          # CPU tensors: no fallback
  with pytest.raises(TgError):
    ops.pointwise_conv(to_dev(np.zeros((1, 2, 2, 8))), to_dev(np.zeros((1, 1, 8, 8))))


# ---------------------------------------------------------------------------------------------- batched passes
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_norm_act_domain_split_equals_separate_calls(ops, dtype):
  """Two reference passes (domains s and t: different gamma/beta, nets/pggan_utils.py:102-113) batched along N."""
  rng = np.random.RandomState(21)
  x = to_dev(bf16_round(rng.randn(5, 8, 8, 16)), dtype)
  ga, be, ga2, be2 = (to_dev(a) for a in (1 + 0.1 * rng.randn(16), 0.1 * rng.randn(16), 1 + 0.2 * rng.randn(16),
                                          0.3 * rng.randn(16)))
  gz = to_dev(bf16_round(rng.randn(5, 8, 8, 16)), dtype)
  split = 2
  leaves = [t.clone().requires_grad_(True) for t in (x, ga, be, ga2, be2)]
  z = ops.norm_act(leaves[0], leaves[1], leaves[2], gamma2=leaves[3], beta2=leaves[4], split=split)
  z.backward(gz)
  parts, grads = [], []
  for lo, hi, g_, b_ in ((0, split, ga, be), (split, 5, ga2, be2)):
    xi = x[lo:hi].clone().requires_grad_(True)
    gi, bi = g_.clone().requires_grad_(True), b_.clone().requires_grad_(True)
    zi = ops.norm_act(xi, gi, bi)
    zi.backward(gz[lo:hi].contiguous())
    parts.append(zi)
    grads.append((xi.grad, gi.grad, bi.grad))
  tol = 1e-6 if dtype == torch.float32 else 1e-2
  assert rel_l2(host(z), host(torch.cat(parts))) < tol
  assert rel_l2(host(leaves[0].grad), host(torch.cat([grads[0][0], grads[1][0]]))) < tol
  for i, (a, b) in enumerate(((leaves[1].grad, grads[0][1]), (leaves[2].grad, grads[0][2]), (leaves[3].grad, grads[1][1]),
                              (leaves[4].grad, grads[1][2]))):
    assert rel_l2(host(a), host(b)) < 1e-4, i


def test_mbstd_groups_equal_separate_calls(ops):
  """Three discriminator calls batched along N keep their own minibatch-stddev statistic (pggan_utils.py:353-366)."""
  rng = np.random.RandomState(22)
  x = to_dev(rng.randn(6, 4, 4, 16)).requires_grad_(True)
  go = to_dev(rng.randn(6, 4, 4, 24))
  out = ops.minibatch_state_concat(x, 24, groups=3)
  out.backward(go)
  for g in range(3):
    xi = x.detach()[2 * g:2 * g + 2].clone().requires_grad_(True)
    oi = ops.minibatch_state_concat(xi, 24)
    oi.backward(go[2 * g:2 * g + 2].contiguous())
    assert rel_l2(host(out[2 * g:2 * g + 2]), host(oi)) < 1e-6
    assert rel_l2(host(x.grad[2 * g:2 * g + 2]), host(xi.grad)) < 1e-5


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_upsample_concat_group_permutation(ops, dtype):
  """Four generator passes batched along N read the skips of the [s; t] encoder batch as groups (t, s, s, t)."""
  rng = np.random.RandomState(23)
  gsz, perm = 2, (1, 0, 0, 1)
  x0 = to_dev(bf16_round(rng.randn(8, 3, 4, 8)), dtype).requires_grad_(True)
  x1 = to_dev(bf16_round(rng.randn(4, 6, 8, 16)), dtype).requires_grad_(True)
  out = ops.upsample2x_concat(x0, x1, gsz, perm)
  go = to_dev(bf16_round(rng.randn(8, 6, 8, 24)), dtype)
  out.backward(go)
  a = x0.detach().clone().requires_grad_(True)
  b = x1.detach().clone().requires_grad_(True)
  bs, bt = b[:2], b[2:]
  ref = ops.upsample2x_concat(a, torch.cat([bt, bs, bs, bt], dim=0).contiguous())
  ref.backward(go)
  assert np.array_equal(host(out), host(ref))
  assert rel_l2(host(x0.grad), host(a.grad)) < 1e-6
  assert rel_l2(host(x1.grad), host(b.grad)) < (1e-6 if dtype == torch.float32 else 1e-2)


# ---------------------------------------------------------------------------------------------- fused pooling
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_conv_pool_fused_backward_equals_composition(ops, dtype):
  """conv + bias + LeakyReLU followed by tf.nn.avg_pool (nets/pggan.py:304-306): the fused op's backward (pool folded
  into the LeakyReLU / bias-gradient kernel) against conv2d -> avg_pool2, with and without the pre-pool output used."""
  rng = np.random.RandomState(31)
  x0 = bf16_round(rng.randn(2, 8, 16, 16))
  w0 = rng.randn(3, 3, 16, 16) / 12.0
  b0 = rng.randn(16) * 0.1
  gp = bf16_round(rng.randn(2, 4, 8, 16))
  gf = bf16_round(rng.randn(2, 8, 16, 16))
  for use_full in (False, True):
    res = []
    for fused in (True, False):
      x = to_dev(x0, dtype).requires_grad_(True)
      w = to_dev(w0).requires_grad_(True)
      b = to_dev(b0).requires_grad_(True)
      if fused:
        z, zp = ops.conv2d(x, w, b, 3, 'SAME', lrelu=True, pool=True)
      else:
        z = ops.conv2d(x, w, b, 3, 'SAME', lrelu=True)
        zp = ops.avg_pool2(z)
      outs, grads = [zp], [to_dev(gp, dtype)]
      if use_full:
        outs.append(z)
        grads.append(to_dev(gf, dtype))
      torch.autograd.backward(outs, grads)
      res.append((host(zp), host(x.grad), host(w.grad), host(b.grad)))
    tol = 1e-5 if dtype == torch.float32 else 2e-2
    for i, nm in enumerate(('zp', 'gx', 'gw', 'gb')):
      assert rel_l2(res[0][i], res[1][i]) < tol, (use_full, nm, rel_l2(res[0][i], res[1][i]))


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_norm_act_pool_fused_backward_equals_composition(ops, dtype):
  """Last layer of an encoder block + avg_pool (nets/pggan.py:466-468) with the UNet skip also consuming z."""
  rng = np.random.RandomState(32)
  y0 = bf16_round(rng.randn(3, 8, 8, 16) * 1.5 + 0.3)
  ga0, be0 = 1 + 0.1 * rng.randn(16), 0.1 * rng.randn(16)
  gp = bf16_round(rng.randn(3, 4, 4, 16))
  gf = bf16_round(rng.randn(3, 8, 8, 16))
  for use_full in (False, True):
    res = []
    for fused in (True, False):
      y = to_dev(y0, dtype).requires_grad_(True)
      ga, be = to_dev(ga0).requires_grad_(True), to_dev(be0).requires_grad_(True)
      if fused:
        z, zp = ops.norm_act(y, ga, be, pool=True)
      else:
        z = ops.norm_act(y, ga, be)
        zp = ops.avg_pool2(z)
      outs, grads = [zp], [to_dev(gp, dtype)]
      if use_full:
        outs.append(z)
        grads.append(to_dev(gf, dtype))
      torch.autograd.backward(outs, grads)
      res.append((host(zp), host(y.grad), host(ga.grad), host(be.grad)))
    tol = 1e-5 if dtype == torch.float32 else 2e-2
    for i, nm in enumerate(('zp', 'gy', 'ggamma', 'gbeta')):
      assert rel_l2(res[0][i], res[1][i]) < tol, (use_full, nm, rel_l2(res[0][i], res[1][i]))


def test_multi_tensor_pack_matches_single_packs(ops):
  """PackCache.refresh (one tg_conv2d_pack_weights_multi launch) == one tg_conv2d_pack_weights per pack."""
  from twingan_amd.ops import PackCache
  PackCache.clear()
  g = torch.Generator().manual_seed(5)
  ws = [torch.randn(3, 3, ci, co, generator=g).to(dev()) for ci, co in ((16, 32), (40, 16), (64, 64))]
  ws.append(torch.randn(4, 4, 32, 32, generator=g).to(dev()))
  # 8x8 maps (conv_img): fragment-ordered packs, tg_conv2d_pack_layout = 1 -- a 32-channel kernel (two K chunks) and wider
  on8 = [torch.randn(3, 3, ci, co, generator=g).to(dev()) for ci, co in ((32, 64), (128, 32))]
  ws += on8
  for w in ws:
    PackCache.register(w)
  packs = []
  for w in ws:
    k = w.shape[0]
    hw = 8 if any(w is v for v in on8) else (16 if k == 3 else 4)
    x = torch.randn(2, hw, hw, w.shape[2], generator=g).to(dev()).bfloat16()
    if hw == 8:
      from twingan_amd import _lib
      d8 = ops._desc(x.shape, w.shape[3], ops.ConvSpec(3, 'SAME'), x.dtype, 0)
      import ctypes
      assert _lib.load().tg_conv2d_pack_layout(ctypes.byref(d8), 0) == 1 and _lib.load().tg_conv2d_pack_layout(ctypes.byref(d8), 1) == 1
    spec = ops.ConvSpec(k, 'SAME' if k == 3 else 'VALID')
    d = ops._desc(x.shape, w.shape[3], spec, x.dtype, 0)
    for mode in (0, 1):
      packs.append((w, mode, PackCache.get(w, d, mode)))
  want = [p.clone() for _, _, p in packs]
  with torch.no_grad():
    for w in ws:
      w.mul_(2.0)
  PackCache.version += 1
  assert PackCache.refresh(ws) == len(packs)
  torch.cuda.synchronize()
  for (w, mode, p), ref in zip(packs, want):
    assert torch.equal(p.float(), (ref.float() * 2.0)), (tuple(w.shape), mode)
  PackCache.clear()


@pytest.mark.parametrize('n,h,c0,c1,cout,gsz,perm', [(2, 8, 32, 32, 16, 0, ()), (4, 16, 64, 64, 64, 1, (1, 0, 0, 1)),
                                                        (2, 8, 64, 32, 128, 0, ())])
def test_upcat_conv_matches_materialised_path(ops, n, h, c0, c1, cout, gsz, perm):
  """conv3x3(concat(up2(x0), skip)) read from the two sources (tg_conv2d_upcat_fwd / _bwd_weight) == the same conv
  over the materialised tg_upsample2x_concat_fwd tensor: output, both input gradients and the filter gradient."""
  g = torch.Generator().manual_seed(11)
  n1 = (max(perm) + 1) * gsz if gsz else n
  x0 = torch.randn(n, h, h, c0, generator=g).to(dev()).bfloat16().requires_grad_(True)
  x1 = torch.randn(n1, 2 * h, 2 * h, c1, generator=g).to(dev()).bfloat16().requires_grad_(True)
  w = (torch.randn(3, 3, c0 + c1, cout, generator=g) * (2.0 / (9 * (c0 + c1))) ** 0.5).to(dev()).requires_grad_(True)
  gy = torch.randn(n, 2 * h, 2 * h, cout, generator=g).to(dev()).bfloat16()
  assert ops.upcat_conv_supported(x0, x1, w)
  y_ref = ops.conv2d(ops.upsample2x_concat(x0, x1, gsz, perm), w, None, 3, 'SAME')
  y_ref.backward(gy)
  ref = [t.grad.clone() for t in (x0, x1, w)]
  for t in (x0, x1, w):
    t.grad = None
  y = ops.upcat_conv(x0, x1, w, gsz, perm)
  y.backward(gy)
  assert rel_l2(host(y), host(y_ref)) < 1e-6           # same kernel arithmetic, same accumulation order per tile
  # input gradients: with the concat adjoint in the backward-data epilogue (tg_conv2d_upcat_bwd_data, 16 x 16 maps and up)
  # the fp32 sums are rounded ONCE; the materialised path rounds the concat-layout gradient and then its 2x2 / group sums
  gtol = 4e-3 if (ops.USE_UPCAT_BWD_FUSED and 2 * h >= 16) else 1e-6
  assert rel_l2(host(x0.grad), host(ref[0])) < gtol
  assert rel_l2(host(x1.grad), host(ref[1])) < gtol
  assert rel_l2(host(w.grad), host(ref[2])) < 1e-5


UPBWD_CASES = [
    # n, hw, c0, c1, cout, gsz, perm                      kernel the shape dispatches
    (4, 256, 32, 32, 16, 1, (1, 0, 0, 1)),              # conv_tile_wres_kernel<3,16,64,1,upboth>: a 32 + 32 concat in one block
    (8, 128, 64, 64, 32, 2, (1, 0, 0, 1)),              # conv_tile_wres_kernel<3,32,64,1,upbwd>
    (8, 128, 32, 32, 32, 2, (0, 1, 1, 0)),              # conv_tile_wres_kernel<3,32,32,1,upbwd>
    (8, 128, 64, 64, 16, 0, ()),                        # conv_tile_wres_kernel<3,16,64,1,upbwd>, no groups
    (4, 128, 64, 64, 16, 1, (0, 0, 0, 1)),              # conv_tile_kernel<3,16,64,1,upbwd>, three sources / one source
    (8, 64, 128, 128, 64, 2, (1, 0, 0, 1)),             # conv_tile_kernel<3,32,64,2,upbwd>
    (16, 64, 64, 64, 32, 4, (1, 0, 0, 1)),              # conv_tile_kernel<3,32,64,1,upbwd>
    (8, 32, 256, 256, 128, 2, (1, 0, 0, 1)),            # conv_tile_kernel<3,32,32,2,upbwd>
    (2, 16, 32, 32, 32, 1, (1, 1)),                     # conv_tile_kernel<3,32,32,1,upbwd>, skip group 0 unread (zeros)
    (2, 32, 32, 32, 16, 0, ()),                         # conv_tile_kernel<3,16,32,1,upbwd>
    (3, 48, 32, 64, 40, 0, ()),                         # ragged: 48 x 48 map, cout 40 (cin_pad 48), c1 = 64
    (4, 256, 32, 64, 16, 1, (1, 0, 0, 1)),              # conv_tile_wres_kernel<3,16,32,1,upbwd> (c1 = 64: two-block form)
    (4, 256, 32, 32, 16, 1, (0, 0, 0, 1)),              # upboth: three sources / one source
    (4, 256, 32, 32, 16, 1, (1, 1, 1, 1)),              # upboth: skip image 0 unread (zeros), image 1 read four times
    (6, 256, 32, 32, 16, 0, ()),                        # upboth without groups
]
UPBWD_KERNELS = ['conv_tile_wres_kernel<3,16,64,1,upboth>', 'conv_tile_wres_kernel<3,32,64,1,upbwd>', 'conv_tile_wres_kernel<3,32,32,1,upbwd>',
                 'conv_tile_wres_kernel<3,16,64,1,upbwd>', 'conv_tile_kernel<3,16,64,1,upbwd>', 'conv_tile_kernel<3,32,64,2,upbwd>',
                 'conv_tile_kernel<3,32,64,1,upbwd>', 'conv_tile_kernel<3,32,32,2,upbwd>', 'conv_tile_kernel<3,32,32,1,upbwd>',
                 'conv_tile_kernel<3,16,32,1,upbwd>', None, 'conv_tile_wres_kernel<3,16,32,1,upbwd>',
                 'conv_tile_wres_kernel<3,16,64,1,upboth>', 'conv_tile_wres_kernel<3,16,64,1,upboth>',
                 'conv_tile_wres_kernel<3,16,64,1,upboth>']


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
@pytest.mark.parametrize('case', range(len(UPBWD_CASES)))
def test_upcat_backward_data_epilogue(ops, dtype, case):
  """tg_conv2d_upcat_bwd_data: the input gradient of conv3x3(concat(up2(x0), skip)) (nets/pggan.py:69-78,
  nets/pggan_utils.py:281-298,349-350) written by the backward-data kernel itself -- 2x2 sums of the first c0 channels into
  g0, the rest summed over the groups that read a skip image into g1 -- for every kernel variant the dispatch can pick, with
  and without group permutations (incl. a skip group nobody reads and one read three times), against float64 sums of the
  float64 backward-data of the same rounded operands (one rounding: <= 2e-3; fp16 3e-4) and against the composed path."""
  from twingan_amd import ops as O, _lib
  n, hw, c0, c1, cout, gsz, perm = UPBWD_CASES[case]
  g = torch.Generator().manual_seed(100 + case)
  n1 = (max(perm) + 1) * gsz if gsz else n
  gy = torch.randn(n, hw, hw, cout, generator=g).to(dtype)
  w = (torch.randn(3, 3, c0 + c1, cout, generator=g) * (2.0 / (9 * cout)) ** 0.5).to(dtype).float()
  gyd, wd = gy.to(dev()), w.to(dev())
  spec = O.ConvSpec(3, 'SAME')
  d = O._desc((n, hw, hw, c0 + c1), cout, spec, dtype, 0)
  g0 = torch.full((n, hw // 2, hw // 2, c0), float('nan'), dtype=dtype, device=dev())
  g1 = torch.full((n1, hw, hw, c1), float('nan'), dtype=dtype, device=dev())
  wpack = O.PackCache.get(wd, d, 1)      # held in a local: an uncached pack must outlive the launch
  O.call('tg_conv2d_upcat_bwd_data', gyd.data_ptr(), wpack.data_ptr(), g0.data_ptr(), g1.data_ptr(), n, hw, hw,
         c0, c1, cout, gsz, O._pack_perm(perm), O._dt(gyd), O._stream())
  sym = _lib.load().tg_last_kernel().decode()
  want = UPBWD_KERNELS[case]
  if want is not None:
    assert sym == (want if dtype == torch.bfloat16 else want.replace('upbwd', 'upbwd,f16').replace('upboth', 'upboth,f16')), sym
  assert bool(torch.isfinite(g0.float()).all()) and bool(torch.isfinite(g1.float()).all())
  # composed path on the device: same values up to the extra rounding of the concat-layout tensor
  gcat = O.conv_bwd_data_raw(gyd, wd, (n, hw, hw, c0 + c1), spec)
  r0, r1 = torch.empty_like(g0), torch.empty_like(g1)
  O.call('tg_upsample2x_concat_bwd', gcat.data_ptr(), r0.data_ptr(), r1.data_ptr(), n, hw // 2, hw // 2, c0, c1, gsz,
         O._pack_perm(perm), O._dt(gcat), O._stream())
  ctol = 4e-3 if dtype == torch.bfloat16 else 6e-4
  unread = [sg for sg in range(n1 // gsz) if sg not in perm] if gsz else []
  for sg in unread:      # nobody read this skip group: exact zeros from both
    assert float(g1[sg * gsz:(sg + 1) * gsz].abs().max()) == 0.0 and float(r1[sg * gsz:(sg + 1) * gsz].abs().max()) == 0.0
  assert rel_l2(host(g0), host(r0)) < ctol, ('g0 vs composed', rel_l2(host(g0), host(r0)))
  assert rel_l2(host(g1), host(r1)) < ctol, ('g1 vs composed', rel_l2(host(g1), host(r1)))
  # float64 reference for one generator image (g0) and one skip image (g1)
  wn, gyn = host(wd), host(gyd)
  tol = 2e-3 if dtype == torch.bfloat16 else 3e-4
  i = n - 1
  gc = N.conv2d_bwd_data_gemm(gyn[i:i + 1], wn, (hw, hw))
  e = rel_l2(host(g0[i:i + 1]), gc[..., :c0].reshape(1, hw // 2, 2, hw // 2, 2, c0).sum(axis=(2, 4)))
  assert e < tol, ('g0 vs float64', e)
  j = n1 - 1
  if gsz:
    srcs = [og * gsz + j % gsz for og in range(n // gsz) if perm[og] == j // gsz]
  else:
    srcs = [j]
  tot = sum(N.conv2d_bwd_data_gemm(gyn[k:k + 1], wn, (hw, hw))[..., c0:] for k in srcs)
  e = rel_l2(host(g1[j:j + 1]), tot)
  assert e < tol, ('g1 vs float64', e, srcs)
  # one output not wanted: the other is unchanged
  g0b = torch.empty_like(g0)
  wpack = O.PackCache.get(wd, d, 1)      # held in a local: an uncached pack must outlive the launch
  O.call('tg_conv2d_upcat_bwd_data', gyd.data_ptr(), wpack.data_ptr(), g0b.data_ptr(), None, n, hw, hw,
         c0, c1, cout, gsz, O._pack_perm(perm), O._dt(gyd), O._stream())
  assert torch.equal(g0b, g0)


@pytest.mark.parametrize('hw,cin,cout,na,nb', [(16, 64, 32, 2, 3), (8, 256, 64, 3, 2), (32, 16, 16, 1, 4)])
def test_paired_filter_gradient_matches_two_launches(ops, hw, cin, cout, na, nb):
  """tg_conv2d_bwd_weight2 (two batches of one layer in one launch) == two tg_conv2d_bwd_weight launches."""
  g = torch.Generator().manual_seed(7)
  mk = lambda n, c: torch.randn(n, hw, hw, c, generator=g).to(dev()).bfloat16()
  xa, gya, xb, gyb = mk(na, cin), mk(na, cout), mk(nb, cin), mk(nb, cout)
  spec = ops.ConvSpec(3, 'SAME')
  ref = torch.zeros(3, 3, cin, cout, device=dev())
  ops.conv_bwd_weight_raw(xa, gya, spec, out=ref)
  ops.conv_bwd_weight_raw(xb, gyb, spec, out=ref)
  out = torch.zeros_like(ref)
  assert ops.conv_bwd_weight2_raw(xa, gya, xb, gyb, spec, out)
  assert rel_l2(host(out), host(ref)) < 1e-5


@pytest.mark.parametrize('dtype,hw,c1,c2', [(torch.bfloat16, 16, 32, 64), (torch.bfloat16, 32, 16, 16), (torch.float32, 8, 8, 8),
                                            (torch.bfloat16, 8, 64, 32)])
def test_lrelu_backward_folded_into_next_backward_data(ops, dtype, hw, c1, c2):
  """conv+bias+lrelu -> conv+bias+lrelu: with fuse_input_lrelu the first layer's LeakyReLU backward runs in the second
  layer's backward-data epilogue and its bias gradient in its own filter-gradient kernel (gradient sinks); all
  gradients must match the unfused chain."""
  g = torch.Generator().manual_seed(21)
  x = torch.randn(3, hw, hw, 16, generator=g).to(dev()).to(dtype)
  w1 = (torch.randn(3, 3, 16, c1, generator=g) * 0.1).to(dev())
  b1 = (torch.randn(c1, generator=g) * 0.1).to(dev())
  w2 = (torch.randn(3, 3, c1, c2, generator=g) * 0.1).to(dev())
  b2 = (torch.randn(c2, generator=g) * 0.1).to(dev())
  gy = torch.randn(3, hw, hw, c2, generator=g).to(dev()).to(dtype)
  res = []
  for fuse, sinks in ((False, False), (True, False), (True, True)):
    ops.GradSink.clear()
    ps = [t.clone().requires_grad_(True) for t in (w1, b1, w2, b2)]
    xin = x.clone().requires_grad_(True)
    bufs = [torch.zeros_like(p) for p in ps]
    if sinks:
      for p, b in zip(ps, bufs):
        ops.GradSink.register(p, b)
    z1 = ops.conv2d(xin, ps[0], ps[1], 3, 'SAME', lrelu=True)
    z2 = ops.conv2d(z1, ps[2], ps[3], 3, 'SAME', lrelu=True, fuse_input_lrelu=fuse)
    z2.backward(gy)
    ops.GradSink.flush()
    grads = [b if sinks else p.grad for p, b in zip(ps, bufs)]
    res.append([host(xin.grad)] + [host(t) for t in grads])
  ops.GradSink.clear()
  tol = 1e-5 if dtype == torch.float32 else 2e-2      # bf16: the fused path rounds gx once instead of twice
  for other in res[1:]:
    for a, b in zip(other, res[0]):
      assert rel_l2(a, b) < tol


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_gdrop_op(ops, dtype):
  """tg_gdrop (libs/gdrop.py:20-36, mode 'prop'): x * (noise[N,1,1,C] * strength * sqrt(C) + 1) with a host or a device
  strength, a channel-padded tensor (c_logical < C), and the node differentiated twice (it is linear: its backward is
  itself)."""
  rng = np.random.RandomState(8)
  n, hw, c, cl = 3, 4, 16, 9
  x = rng.randn(n, hw, hw, c)
  x[..., cl:] = 0.0
  if dtype == torch.bfloat16:
    x = bf16_round(x)
  noise = rng.randn(n, c).astype(np.float32)
  strength = 0.37
  f = noise.astype(np.float64) * (strength * float(np.sqrt(np.float32(cl)))) + 1.0
  ref = x * f[:, None, None, :]
  xd = to_dev(x, dtype).requires_grad_(True)
  nd = torch.from_numpy(noise).to(dev())
  y = ops.gdrop(xd, strength, noise=nd, c_logical=cl)
  assert rel_l2(host(y), ref) < tol_for(dtype)
  sdev = torch.tensor([strength], dtype=torch.float32, device=dev())      # the gdrop_strength variable
  assert torch.equal(ops.gdrop(xd.detach(), sdev, noise=nd, c_logical=cl), y.detach())
  gy = rng.randn(n, hw, hw, c)
  gyd = to_dev(gy, dtype).requires_grad_(True)
  gx, = torch.autograd.grad(y, xd, gyd, create_graph=True)
  assert rel_l2(host(gx), gy * f[:, None, None, :]) < tol_for(dtype, True)
  v = rng.randn(n, hw, hw, c)
  ggy, = torch.autograd.grad(gx, gyd, to_dev(v, dtype))      # d/d gy of gy * f, contracted with v
  assert rel_l2(host(ggy), v * f[:, None, None, :]) < tol_for(dtype, True)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize('inner', [(4, 4, 8), (5,), (3, 3)])      # 16-byte rows, and rows only the scalar path can take
def test_rows_and_cat_rows(ops, record_calls, dtype, inner):
  """ops.rows / ops.cat_rows (tg_rows_assemble): the batched towers' tf.concat / split glue (twingan.py:233-288).  Views
  forward; repeats and concatenations one launch; the backward ONE launch that writes each row block once -- the fp32 sum
  of every gradient covering it, zeros where none does -- against the framework's chunk / cat / add arithmetic in fp64."""
  rng = np.random.RandomState(5)
  b = 3
  x = to_dev(rng.randn(*((2 * b,) + inner)), dtype).double().cpu().numpy()      # values the dtype holds exactly
  xd = to_dev(x, dtype).requires_grad_(True)
  s_rows, t_rows = (0, b), (b, 2 * b)
  record_calls.clear()
  es, et, rep, unused, mid = ops.rows(xd, [s_rows, t_rows, (t_rows, s_rows, s_rows, t_rows), (1, 4), (2, 5)])
  assert [c[0] for c in record_calls] == ['tg_rows_assemble']
  assert es.data_ptr() == xd.data_ptr() and et.data_ptr() == xd.data_ptr() + b * xd[0].numel() * xd.element_size()
  np.testing.assert_array_equal(host(rep), np.concatenate([x[b:], x[:b], x[:b], x[b:]]))
  np.testing.assert_array_equal(host(mid), x[2:5])
  g_es, g_rep, g_mid = rng.randn(*es.shape), rng.randn(*rep.shape), rng.randn(*mid.shape)
  g_es, g_rep, g_mid = (to_dev(g, dtype).double().cpu().numpy() for g in (g_es, g_rep, g_mid))
  want = np.zeros_like(x)
  want[:b] += g_es
  want[b:] += g_rep[:b] + g_rep[3 * b:]
  want[:b] += g_rep[b:2 * b] + g_rep[2 * b:3 * b]
  want[2:5] += g_mid
  record_calls.clear()
  gx, = torch.autograd.grad([es, rep, mid], xd, [to_dev(g_es, dtype), to_dev(g_rep, dtype), to_dev(g_mid, dtype)])
  assert [c[0] for c in record_calls] == ['tg_rows_assemble']      # et and `unused` bring no gradient and no zero tensor
  assert rel_l2(host(gx), want) < (1e-6 if dtype == torch.float32 else 4e-3)
  # a lone gradient over all rows is passed through; no gradient at all is None
  whole, = ops.rows(xd, [(0, 2 * b)])
  record_calls.clear()
  g1, = torch.autograd.grad(whole, xd, to_dev(x, dtype))
  assert record_calls == [] and torch.equal(g1, to_dev(x, dtype))
  # concatenation: a copy with a tape (the gradients are views), a view of adjacent rows without one
  a, c = to_dev(x[:2], dtype).requires_grad_(True), to_dev(x[2:], dtype)
  both = ops.cat_rows([a, c, a])
  np.testing.assert_array_equal(host(both), np.concatenate([x[:2], x[2:], x[:2]]))
  ga, = torch.autograd.grad(both, a, both.detach())
  assert rel_l2(host(ga), 2 * x[:2]) < (1e-6 if dtype == torch.float32 else 4e-3)
  base = to_dev(x, dtype)
  record_calls.clear()
  view = ops.cat_rows([base[:2], base[2:]])
  assert record_calls == [] and view.data_ptr() == base.data_ptr() and torch.equal(view, base)
  apart = ops.cat_rows([base[:2], base[3:]])
  np.testing.assert_array_equal(host(apart), np.concatenate([x[:2], x[3:]]))
  # more blocks than one launch takes, more sources than one job takes
  many = ops.cat_rows([base[k:k + 1] for k in (0, 1, 2, 3, 4, 5, 0, 1, 2, 3)])
  np.testing.assert_array_equal(host(many), x[[0, 1, 2, 3, 4, 5, 0, 1, 2, 3]])
  dst = torch.empty_like(base[:1])
  ops.assemble_rows(dst, [(0, 1, [base[k:k + 1] for k in range(6)])])
  assert rel_l2(host(dst), x.sum(0, keepdims=True)) < (1e-6 if dtype == torch.float32 else 8e-3)


def test_uniform_draws(ops):
  """tg_uniform: Philox4x32-10 keyed by (seed, draw counter) -- U[0,1) values, a new draw per launch (the counter is
  advanced on the device, ticket word back at 0), the same stream for the same seed, ragged lengths, and sane moments."""
  state = torch.zeros(2, dtype=torch.int32, device=dev())
  a = ops.uniform(32, 7, state)
  b = ops.uniform(32, 7, state)
  assert state.tolist() == [2, 0]
  assert float(a.min()) >= 0.0 and float(a.max()) < 1.0 and not torch.equal(a, b)
  again = torch.zeros(2, dtype=torch.int32, device=dev())
  assert torch.equal(ops.uniform(32, 7, again), a) and torch.equal(ops.uniform(32, 7, again), b)
  assert not torch.equal(ops.uniform(32, 8, torch.zeros(2, dtype=torch.int32, device=dev())), a)
  # a prefix of a longer draw is the shorter draw (counter = block index), whatever the grid
  long = ops.uniform(300001, 7, torch.zeros(2, dtype=torch.int32, device=dev()))
  assert torch.equal(long[:32], a)
  x = host(long)
  assert abs(x.mean() - 0.5) < 3e-3 and abs(x.var() - 1.0 / 12.0) < 2e-3 and x.min() >= 0.0 and x.max() < 1.0
  assert abs(np.corrcoef(x[:-1], x[1:])[0, 1]) < 1e-2
  r = host(ops.uniform(1000, 3, torch.zeros(2, dtype=torch.int32, device=dev()), lo=-1.0, hi=1.0))
  assert r.min() >= -1.0 and r.max() < 1.0 and abs(r.mean()) < 0.1
  # the known-answer vector of Philox4x32-10 (Random123 kat_vectors: counter 0, key 0)
  z = ops.uniform(4, 0, torch.zeros(2, dtype=torch.int32, device=dev()))
  words = [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
  assert host(z).tolist() == [float(np.float32(w >> 8) * np.float32(1.0 / 16777216.0)) for w in words]


def test_no_backward_work_without_a_gradient(ops, record_calls):
  """A conv / minibatch-stddev node the backward reaches WITHOUT a gradient (the gradient penalty's second backward
  reaches the layers after the minibatch stddev only through LeakyReLU masks) launches nothing and passes None on --
  the default would materialise a tensor of zeros and run backward-data, filter-gradient and mbstd kernels on it."""
  class Drop(torch.autograd.Function):      # a consumer whose backward has nothing to say about its input
    @staticmethod
    def forward(ctx, t):
      return t.view_as(t)

    @staticmethod
    def backward(ctx, g):
      return None

  rng = np.random.RandomState(2)
  x = to_dev(rng.randn(4, 4, 4, 16), torch.bfloat16).requires_grad_(True)
  w1, w2 = (to_dev(rng.randn(3, 3, c, 16) * 0.1).requires_grad_(True) for c in (16, 24))
  b = to_dev(rng.randn(16) * 0.1).requires_grad_(True)
  h = ops.conv2d(x, w1, b, 3, 'SAME', lrelu=True)
  y = ops.conv2d(ops.minibatch_state_concat(h, 24, 2), w2, None, 3, 'SAME', lrelu=False)
  record_calls.clear()
  (Drop.apply(y).float().sum() + x.float().sum()).backward()
  assert [c[0] for c in record_calls if c[0].startswith(('tg_conv2d', 'tg_mbstd', 'tg_lrelu'))] == []
  assert w1.grad is None and w2.grad is None and b.grad is None
  assert torch.equal(x.grad, torch.ones_like(x))


def test_first_order_only_input(ops, record_calls):
  """ops.first_order_only: the gradient penalty differentiates D with respect to the interpolates under create_graph;
  the FINAL backward then wants parameter gradients only -- the first layer skips its input gradient (a full-resolution
  backward-data launch and a copy into .grad), the parameter gradients are those of the unmarked run."""
  rng = np.random.RandomState(3)
  xv = to_dev(rng.randn(2, 8, 8, 3), torch.bfloat16)
  wv, bv = to_dev(rng.randn(1, 1, 3, 16) * 0.5), to_dev(rng.randn(16) * 0.1)
  res = []
  for mark in (False, True):
    x = xv.clone().requires_grad_(True)
    if mark:
      ops.first_order_only(x)
    w, b = wv.clone().requires_grad_(True), bv.clone().requires_grad_(True)
    with ops.second_order():
      y = ops.pointwise_conv(ops.scale(x, 0.7), w, b, lrelu=True)
    gx, = torch.autograd.grad(y, x, torch.ones_like(y), create_graph=True)      # first order: wanted either way
    record_calls.clear()
    (gx.float().pow(2).sum() + y.float().sum()).backward()
    res.append((gx.detach(), w.grad, b.grad, x.grad, [c[0] for c in record_calls]))
  (gx0, w0, b0, x0, calls0), (gx1, w1, b1, x1, calls1) = res
  assert torch.equal(gx0, gx1) and torch.equal(w0, w1) and torch.equal(b0, b1)
  assert x0 is not None and x1 is None
  assert calls0.count('tg_pointwise_conv_fwd') == calls1.count('tg_pointwise_conv_fwd') + 1, (calls0, calls1)
  assert calls0.count('tg_axpby') == calls1.count('tg_axpby') + 1, (calls0, calls1)


SMALL_MASK_CASES = [
    # n, hw, cin, cout, k, padding, kernel family of the backward-data
    (5, 8, 256, 256, 3, 'SAME', 'conv_img'),
    (3, 8, 512, 256, 3, 'SAME', 'conv_img'),
    (5, 4, 256, 256, 3, 'SAME', 'conv_small'),
    (6, 4, 264, 256, 3, 'SAME', 'conv_small'),      # the minibatch-stddev layer: 264 input channels (a partial last block)
    (6, 4, 64, 64, 4, 'VALID', 'conv_small'),       # the dense rewrite of the discriminator's 4x4 VALID conv
]


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
@pytest.mark.parametrize('n,hw,cin,cout,k,padding,family', SMALL_MASK_CASES)
def test_masked_backward_data_on_the_small_maps(ops, dtype, n, hw, cin, cout, k, padding, family):
  """tg_conv2d_bwd_data_masked at the 8x8 / 4x4 maps and the dense 4x4-VALID layer: the LeakyReLU backward of the layer
  below rides in the epilogue of conv_img / conv_small (as it does in conv_tile's from 16x16 up) -- ONE launch, no
  tg_lrelu_bwd pass over the result -- against the float64 oracle on rounded operands (one rounding of the product)."""
  from twingan_amd import _lib
  rng = np.random.RandomState(31)
  rnd = bf16_round if dtype == torch.bfloat16 else f16_round
  x = rnd(rng.randn(n, hw, hw, cin))
  wt = rnd(rng.randn(k, k, cin, cout) / np.sqrt(k * k * cin))
  spec = ops.ConvSpec(k, padding)
  ho, wo = spec.out_hw(hw, hw)
  gy = rnd(rng.randn(n, ho, wo, cout))
  xd, gyd, wd = to_dev(x, dtype), to_dev(gy, dtype), to_dev(wt)
  names = []
  import twingan_amd.ops as O
  real = O.call

  def spy(name, *a, **kw):
    names.append(name)
    return real(name, *a, **kw)
  O.call = spy
  try:
    gxm = ops.conv_bwd_data_masked_raw(gyd, wd, xd, spec)
  finally:
    O.call = real
  kern = _lib.load().tg_last_kernel().decode()
  assert names[-1] == 'tg_conv2d_bwd_data_masked' and 'tg_lrelu_bwd' not in names and family in kern, (names, kern)      # the conv kernel ran LAST: no mask pass after it
  ref = N.conv2d_bwd_data(gy, wt, (hw, hw), padding) * np.where(x > 0, 1.0, 0.2)
  assert rel_l2(host(gxm), ref) < (8e-4 if dtype == torch.float16 else 5e-3)
  plain = ops.conv_bwd_data_raw(gyd, wd, (n, hw, hw, cin), spec)      # the same kernel without the mask: untouched
  assert rel_l2(host(plain), N.conv2d_bwd_data(gy, wt, (hw, hw), padding)) < (8e-4 if dtype == torch.float16 else 5e-3)
  # ... and the forward conv with the mask of its OUTPUT's shape (tg_conv2d_fwd_masked: the gradient penalty's second pass)
  msrc = rnd(rng.randn(n, ho, wo, cout))
  ym = ops.conv_fwd_masked_raw(xd, wd, to_dev(msrc, dtype), spec)
  assert family in _lib.load().tg_last_kernel().decode()
  assert rel_l2(host(ym), N.conv2d(x, wt, padding) * np.where(msrc > 0, 1.0, 0.2)) < (8e-4 if dtype == torch.float16 else 5e-3)


@pytest.mark.parametrize('dtype,hw,c1,c2', [(torch.bfloat16, 16, 32, 64), (torch.float32, 8, 8, 8), (torch.bfloat16, 32, 16, 16)])
def test_lrelu_fold_under_create_graph_matches_unfused(ops, dtype, hw, c1, c2):
  """Gradient-penalty shaped double backward through conv+bias+lrelu -> conv+bias+lrelu -> conv: with fuse_input_lrelu
  the first backward runs MaskedDgradFn (mask in the backward-data epilogue) instead of LeakyReLU-backward + backward-
  data nodes (and the pooled last layer one unpool+mask node); the input gradient, the penalty and every parameter
  gradient of the penalty must match the unfused chain and a float64 torch reference."""
  g = torch.Generator().manual_seed(33)
  x = torch.randn(2, hw, hw, 16, generator=g).to(dev()).to(dtype)
  shapes = [(3, 3, 16, c1), (c1,), (3, 3, c1, c2), (c2,), (3, 3, c2, 16), (16,)]
  ws = [(torch.randn(*s, generator=g) * (0.1 if len(s) == 4 else 0.05)).to(dev()) for s in shapes]
  res = []
  for fuse in (False, True):
    ops.GradSink.clear()
    ps = [t.clone().requires_grad_(True) for t in ws]
    xin = x.clone().requires_grad_(True)
    z1 = ops.conv2d(xin, ps[0], ps[1], 3, 'SAME', lrelu=True)
    z2 = ops.conv2d(z1, ps[2], ps[3], 3, 'SAME', lrelu=True, fuse_input_lrelu=fuse)
    _, z3 = ops.conv2d(z2, ps[4], ps[5], 3, 'SAME', lrelu=True, fuse_input_lrelu=fuse, pool=True)      # block end: pooled
    gx, = torch.autograd.grad(z3.float().sum(), xin, create_graph=True)
    pen = ((gx.float().pow(2).sum(dim=(1, 2, 3)).sqrt() - 1.0) ** 2).mean()
    grads = torch.autograd.grad(pen, [ps[0], ps[2], ps[4]])
    res.append([host(gx.detach()), host(pen.detach().reshape(1))] + [host(t) for t in grads])
  tol = 1e-5 if dtype == torch.float32 else 3e-2
  for a, b in zip(res[1], res[0]):
    assert rel_l2(a, b) < tol, (rel_l2(a, b))
  # independent reference: the same graph in float64 torch on the host
  import torch.nn.functional as F
  xr = x.double().cpu().requires_grad_(True)
  pr = [t.double().cpu().requires_grad_(True) for t in ws]
  def layer(a, w, b):
    y = F.conv2d(a.permute(0, 3, 1, 2), w.permute(3, 2, 0, 1), b, padding=1).permute(0, 2, 3, 1)
    return torch.maximum(y, 0.2 * y)
  a3 = layer(layer(layer(xr, pr[0], pr[1]), pr[2], pr[3]), pr[4], pr[5])
  z3r = F.avg_pool2d(a3.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
  gxr, = torch.autograd.grad(z3r.sum(), xr, create_graph=True)
  penr = ((gxr.pow(2).sum(dim=(1, 2, 3)).sqrt() - 1.0) ** 2).mean()
  gr = torch.autograd.grad(penr, [pr[0], pr[2], pr[4]])
  want = [gxr.detach().numpy(), penr.detach().reshape(1).numpy()] + [t.numpy() for t in gr]
  rtol = 1e-4 if dtype == torch.float32 else 6e-2
  for a, b in zip(res[1], want):
    assert rel_l2(a, b) < rtol, rel_l2(a, b)


@pytest.mark.parametrize('dtype,hw,c1,c2', [(torch.bfloat16, 16, 32, 64), (torch.float32, 8, 8, 8), (torch.bfloat16, 32, 16, 16),
                                            (torch.float16, 64, 16, 32)])
def test_gradient_penalty_second_pass_masks_in_the_conv_epilogue(ops, monkeypatch, dtype, hw, c1, c2):
  """The trainer's gradient-penalty flow (image_generation.py:414-439): inner gradient under ops.no_param_grads with
  create_graph, parameters through the double backward.  With USE_GP_PREMASK the LeakyReLU mask every node of the second
  pass applies to its incoming cotangent sits in the epilogue of the conv that produces it (tg_conv2d_fwd_masked; the
  producer is flagged and skips its tg_lrelu_bwd launch): fewer launches, same penalty gradients as the unflagged chain and
  as a float64 torch reference; the launch counts are checked through the profiler hook."""
  from twingan_amd import _lib
  g = torch.Generator().manual_seed(34)
  x = torch.randn(2, hw, hw, 16, generator=g).to(dev()).to(dtype)
  shapes = [(3, 3, 16, c1), (c1,), (3, 3, c1, c2), (c2,), (3, 3, c2, c2), (c2,), (3, 3, c2, 16), (16,)]
  ws = [(torch.randn(*s, generator=g) * (0.1 if len(s) == 4 else 0.05)).to(dev()) for s in shapes]
  res, launches = [], []
  # third run: the block end's unpool + mask + masked backward-data as ONE differentiable node (UnpoolMaskedDgradFn)
  for premask, one_node in ((False, False), (True, False), (True, True)):
    monkeypatch.setattr(ops, 'USE_GP_PREMASK', premask)
    monkeypatch.setattr(ops, 'USE_DGRAD_UNPOOL_GP', one_node)
    ops.GradSink.clear()
    ps = [t.clone().requires_grad_(True) for t in ws]
    xin = x.clone().requires_grad_(True)
    with ops.second_order():
      z1 = ops.conv2d(xin, ps[0], ps[1], 3, 'SAME', lrelu=True)
      z2 = ops.conv2d(z1, ps[2], ps[3], 3, 'SAME', lrelu=True, fuse_input_lrelu=True)
      _, z3 = ops.conv2d(z2, ps[4], ps[5], 3, 'SAME', lrelu=True, fuse_input_lrelu=True, pool=True, pool_only=True)      # block end
      z4 = ops.conv2d(z3, ps[6], ps[7], 3, 'SAME', lrelu=True, fuse_input_lrelu=True)
    with ops.no_param_grads():
      gx, = torch.autograd.grad(z4.float().sum(), xin, create_graph=True)
    pen = ((gx.float().pow(2).sum(dim=(1, 2, 3)).sqrt() - 1.0) ** 2).mean()
    _lib.profiler = []
    try:
      grads = torch.autograd.grad(pen, [ps[0], ps[2], ps[4], ps[6]])
      torch.cuda.synchronize()
      names = [r[0] for r in _lib.profiler]
    finally:
      _lib.profiler = None
    launches.append((names.count('tg_lrelu_bwd'), names.count('tg_conv2d_fwd_masked')))
    res.append([host(gx.detach()), host(pen.detach().reshape(1))] + [host(t) for t in grads])
    node = gx.grad_fn
    seen = set()
    stack = [node]
    while stack:      # is the one-node form in the graph of the inner gradient exactly when it should be?
      nd = stack.pop()
      if nd is None or nd in seen:
        continue
      seen.add(nd)
      stack.extend(f for f, _ in nd.next_functions)
    has = any('UnpoolMaskedDgradFn' in type(nd).__name__ for nd in seen)
    assert has == (one_node and dtype != torch.float32 and c2 % 32 == 0), (has, one_node)
  # three masks move into conv epilogues: z1's (into conv 2's node), z2's (conv 3's node), z3-block-end's (the unpool node)
  assert launches[1][1] >= 2 and launches[1][0] <= launches[0][0] - launches[1][1], launches
  tol = 1e-5 if dtype == torch.float32 else 3e-2
  for a, b in zip(res[1], res[0]):
    assert rel_l2(a, b) < tol, (rel_l2(a, b))
  for a, b in zip(res[2], res[0]):
    assert rel_l2(a, b) < tol, (rel_l2(a, b))
  import torch.nn.functional as F
  xr = x.double().cpu().requires_grad_(True)
  pr = [t.double().cpu().requires_grad_(True) for t in ws]
  def layer(a, w, b):
    y = F.conv2d(a.permute(0, 3, 1, 2), w.permute(3, 2, 0, 1), b, padding=1).permute(0, 2, 3, 1)
    return torch.maximum(y, 0.2 * y)
  a3 = layer(layer(layer(xr, pr[0], pr[1]), pr[2], pr[3]), pr[4], pr[5])
  z3r = F.avg_pool2d(a3.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
  z4r = layer(z3r, pr[6], pr[7])
  gxr, = torch.autograd.grad(z4r.sum(), xr, create_graph=True)
  penr = ((gxr.pow(2).sum(dim=(1, 2, 3)).sqrt() - 1.0) ** 2).mean()
  gr = torch.autograd.grad(penr, [pr[0], pr[2], pr[4], pr[6]])
  want = [gxr.detach().numpy(), penr.detach().reshape(1).numpy()] + [t.numpy() for t in gr]
  rtol = 1e-4 if dtype == torch.float32 else 1e-1      # four 16-bit layers (the three-layer test above: 6e-2; measured 7.4e-2)
  for r in (res[1], res[2]):
    for a, b in zip(r, want):
      assert rel_l2(a, b) < rtol, rel_l2(a, b)


@pytest.mark.parametrize('k,cin,cout', [(3, 16, 32), (1, 3, 16), (4, 64, 64), (3, 264, 256), (3, 5, 7)])
def test_spectral_norm_matches_oracle(ops, k, cin, cout):
  """tg_spectral_norm_fwd / _bwd (libs/sn.py:38-101): w_bar, the next power-iteration vector, and d L / d w with the
  gradient flowing through sigma, v and u' -- against float64 autograd of the literal formulas."""
  rng = np.random.RandomState(6)
  w = rng.randn(k, k, cin, cout) * 0.1
  u = rng.randn(1, cout)
  gq = rng.randn(k, k, cin, cout)
  wd = to_dev(w).requires_grad_(True)
  w_bar, u_new = ops.spectral_norm(wd, to_dev(u))
  (w_bar * to_dev(gq)).sum().backward()
  wt = torch.from_numpy(w).requires_grad_(True)
  w2 = wt.reshape(-1, cout)
  ut = torch.from_numpy(u)
  v = R.l2_normalize(ut @ w2.t())
  u1 = R.l2_normalize(v @ w2)
  sigma = (v @ w2 @ u1.t()).reshape(())
  ref = (w2 / sigma).reshape(wt.shape)
  (ref * torch.from_numpy(gq)).sum().backward()
  assert rel_l2(host(w_bar), ref.detach().numpy()) < F32_TOL
  assert rel_l2(host(u_new), u1.detach().numpy()) < F32_TOL
  assert rel_l2(host(wd.grad), wt.grad.numpy()) < 5 * F32_TOL


def test_spectral_norm_of_many_kernels_in_three_launches(ops):
  """tg_spectral_norm_fwd_multi (ops.spectral_norm_multi, what pggan.prepare_run uses): the power iterations of several kernels of
  different shapes from one job table -- w_bar, u', and the gradients through the per-kernel nodes equal the one-kernel
  entry point's bit for bit (the same kernel bodies in the same order), also when the table is reused for a second run."""
  g = torch.Generator().manual_seed(37)
  shapes = [(3, 3, 16, 32), (1, 1, 3, 16), (4, 4, 64, 64), (3, 3, 264, 256), (3, 3, 5, 7), (3, 3, 128, 40)]
  ws = [(torch.randn(*sh, generator=g) * 0.1).to(dev()) for sh in shapes]
  us = [torch.randn(1, sh[3], generator=g).to(dev()) for sh in shapes]
  gq = [torch.randn(*sh, generator=g).to(dev()) for sh in shapes]
  outs = [torch.empty(w.numel(), dtype=torch.float32, device=w.device) for w in ws]
  table = None
  for run in range(2):
    single = []
    for w, u, q in zip(ws, us, gq):
      wd = w.clone().requires_grad_(True)
      wb, un = ops.spectral_norm(wd, u)
      (wb * q).sum().backward()
      single.append((wb.detach().clone(), un.detach().clone(), wd.grad.clone()))
    wds = [w.clone().requires_grad_(True) for w in ws]
    if run == 1:      # the same addresses: the table of run 0 is reused
      for wd, keep in zip(wds, kept):
        keep.data.copy_(wd.data)
      wds = kept
      for wd in wds:
        wd.grad = None
    res, table2 = ops.spectral_norm_multi(list(zip(wds, us, outs)), table)
    assert run == 0 or table2 is table
    table, kept = table2, wds
    loss = sum((wb * q).sum() for (wb, _), q in zip(res, gq))
    loss.backward()
    for (wb, un), wd, (wb1, un1, g1) in zip(res, wds, single):
      assert torch.equal(wb.detach(), wb1) and torch.equal(un.detach().reshape(-1), un1.reshape(-1))
      assert torch.equal(wd.grad, g1)
    for u, (_, un) in zip(us, res):      # the next run starts from u', assigned in place as pggan.end_run does
      u.copy_(un.detach().reshape(1, -1))
  # the nodes save the table's PERSISTENT buffers: a backward after the table has run again must refuse, not use them
  for wd in wds:
    wd.grad = None
  res, _ = ops.spectral_norm_multi(list(zip(wds, us, outs)), table)
  stale = sum((wb * q).sum() for (wb, _), q in zip(res, gq))
  ops.spectral_norm_multi(list(zip(wds, us, outs)), table)
  with pytest.raises(RuntimeError, match='one outstanding graph'):
    stale.backward()


BGEMM_CASES = [
    # batch, m, n, k     (attention: s = f g^T is (N, N, c/8); o = beta h is (N, c, N); their gradients transpose them)
    (2, 64, 64, 2), (2, 64, 16, 64), (3, 256, 256, 8), (2, 256, 64, 256), (1, 130, 70, 36), (2, 33, 9, 5),
    (2, 1024, 1024, 8), (2, 1024, 64, 1024),
]


@pytest.mark.parametrize('batch,m,n,k', BGEMM_CASES)
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_batched_gemm_all_transposes(ops, batch, m, n, k, dtype):
  """tg_batched_gemm (csrc/attention.hip): all four operand layouts of the MFMA kernel (ds_read_b128 for a K-contiguous
  operand, the LDS transpose read for the other kind), ragged tiles and unaligned leading dimensions, against float64."""
  rng = np.random.RandomState(11)
  for ta in (False, True):
    for tb in (False, True):
      a = rng.randn(batch, k, m) if ta else rng.randn(batch, m, k)
      b = rng.randn(batch, n, k) if tb else rng.randn(batch, k, n)
      if dtype == torch.bfloat16:
        a, b = bf16_round(a), bf16_round(b)
      ref = np.matmul(a.transpose(0, 2, 1) if ta else a, b.transpose(0, 2, 1) if tb else b) * 0.5
      c = ops.bgemm(to_dev(a, dtype), to_dev(b, dtype), ta, tb, 0.5)
      assert rel_l2(host(c), ref) < (F32_TOL if dtype == torch.float32 else 4e-3), (ta, tb)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('rows,cols', [(6, 64), (10, 100), (4, 4096)])
def test_softmax_rows_first_and_second_order(ops, rows, cols, dtype):
  """Row softmax, its backward and the backward OF that backward (the gradient-penalty pass differentiates the
  discriminator's attention twice) against float64 autograd."""
  rng = np.random.RandomState(12)
  s = rng.randn(rows, cols) * 2.0
  w1 = rng.randn(rows, cols)
  w2 = rng.randn(rows, cols)
  if dtype == torch.bfloat16:
    s, w1, w2 = bf16_round(s), bf16_round(w1), bf16_round(w2)
  sd = to_dev(s, dtype).requires_grad_(True)
  p = ops.softmax_rows(sd)
  gs, = torch.autograd.grad(p, sd, grad_outputs=to_dev(w1, dtype), create_graph=True)
  (gs * to_dev(w2, dtype)).sum().backward()
  st = torch.from_numpy(s).requires_grad_(True)
  pt = torch.softmax(st, dim=-1)
  gst, = torch.autograd.grad(pt, st, grad_outputs=torch.from_numpy(w1), create_graph=True)
  (gst * torch.from_numpy(w2)).sum().backward()
  tol = F32_TOL if dtype == torch.float32 else 2e-2
  assert rel_l2(host(p), pt.detach().numpy()) < (F32_TOL if dtype == torch.float32 else 4e-3)
  assert rel_l2(host(gs), gst.detach().numpy()) < tol
  assert rel_l2(host(sd.grad), st.grad.numpy()) < (5 * F32_TOL if dtype == torch.float32 else 5e-2)


def test_tanh_and_scale_second_order(ops):
  rng = np.random.RandomState(13)
  x, w1, w2 = rng.randn(4, 33), rng.randn(4, 33), rng.randn(4, 33)
  gam = np.array([0.7])
  xd = to_dev(x).requires_grad_(True)
  gd = to_dev(gam).requires_grad_(True)
  y = ops.scale_dev(ops.tanh(xd), gd)
  gx, = torch.autograd.grad(y, xd, grad_outputs=to_dev(w1), create_graph=True)
  (gx * to_dev(w2)).sum().backward()
  xt = torch.from_numpy(x).requires_grad_(True)
  gt = torch.from_numpy(gam).requires_grad_(True)
  yt = torch.tanh(xt) * gt
  gxt, = torch.autograd.grad(yt, xt, grad_outputs=torch.from_numpy(w1), create_graph=True)
  (gxt * torch.from_numpy(w2)).sum().backward()
  assert rel_l2(host(y), yt.detach().numpy()) < F32_TOL and rel_l2(host(gx), gxt.detach().numpy()) < F32_TOL
  assert rel_l2(host(xd.grad), xt.grad.numpy()) < 5 * F32_TOL and rel_l2(host(gd.grad), gt.grad.numpy()) < 5 * F32_TOL


@pytest.mark.parametrize('hw,c,n', [(64, 64, 4), (16, 32, 3)])
def test_self_attention_layer_bf16_at_config4_shape(hw, c, n):
  """The whole SAGAN layer as the discriminator of BASELINE configs[4] runs it (64x64 map, 64 channels: N = 4096,
  d = 8) on the MFMA batched GEMM, bf16, forward and first-order backward, against the float64 oracle on the same
  bf16-rounded inputs and weights."""
  from oracle import torch_ref as R2
  from twingan_amd import Config, pggan
  from twingan_amd.params import ParamStore
  rng = np.random.RandomState(14)
  sc = 'discriminator_s/self_attention_%dx%dx%d' % (hw, hw, c)
  st = ParamStore('cuda:0')
  for nm, co in (('sa_f', c // 8), ('sa_g', c // 8), ('sa_h', c)):
    st.add_conv('%s/%s' % (sc, nm), 1, c, co, 'd', True, ())
  st.add(sc + '/sa_gamma', (1,), 'd', 'beta')
  st.build(0)
  vals = {}
  for k, spec in st.specs.items():
    v = rng.randn(*spec['shape']) * (0.6 if k.endswith('weights') else 0.1)
    vals[k] = bf16_round(v) if k.endswith('weights') else np.float32(v).astype(np.float64)
  vals[sc + '/sa_gamma'] = np.array([0.8])
  st.load_state_dict({k: torch.from_numpy(v) for k, v in vals.items()})
  x = bf16_round(rng.randn(n, hw, hw, c) * 0.5)
  cfg = Config(hw=hw, max_ch=c, precision='bf16', do_self_attention=True, self_attention_hw=hw)
  for p_ in st.P.values():
    p_.requires_grad_(True)
  xd = to_dev(x, torch.bfloat16).requires_grad_(True)
  y = pggan.self_attention_layer(st.P, sc, xd, None, cfg, True)
  gy = bf16_round(rng.randn(*x.shape))
  y.backward(to_dev(gy, torch.bfloat16))
  Pt = {k: torch.from_numpy(v).requires_grad_(True) for k, v in vals.items()}
  xt = torch.from_numpy(x).requires_grad_(True)
  rcfg = R2.Config(hw=hw, max_ch=c, do_self_attention=True, self_attention_hw=hw)
  yt = R2.self_attention(Pt, sc, xt, None, rcfg, True)
  yt.backward(torch.from_numpy(gy))
  assert rel_l2(host(y), yt.detach().numpy()) < 1e-2
  assert rel_l2(host(xd.grad), xt.grad.numpy()) < 3e-2
  gd = st.grad_dict()
  for k in vals:
    ref = Pt[k].grad.numpy()
    assert rel_l2(gd[k].double().cpu().numpy(), ref) < 3e-2, k


# ------------------------------------------------------------------------- conv with the statistics epilogue
STATS_CASES = [
    # n, hw, cin, cout  -> kernel family
    (4, 256, 16, 16),     # weight-resident thin kernel, several tiles per workgroup
    (4, 256, 16, 32),
    (8, 128, 32, 64),     # weight-resident, 64-channel blocks
    (3, 64, 64, 64),      # tile kernel, two sub-tiles per wave
    (2, 32, 128, 256),    # tile kernel, channel blocks along grid y
    (3, 16, 256, 256),    # tile kernel, 2 tiles per image
    (2, 16, 40, 24),      # ragged channel counts (partial 32-channel blocks; no pixel norm at c = 24)
    (5, 8, 256, 256),     # conv_img: a whole 8x8 image per workgroup, ONE chunk per image
    (3, 8, 512, 256),
    (6, 4, 256, 256),     # conv_small: a 4x4 image is 16 lanes of a column block, ONE chunk per image
    (64, 4, 256, 64),     # ... two column blocks per workgroup
    (200, 4, 64, 32),     # ... four
]


@pytest.mark.parametrize('n,hw,cin,cout', STATS_CASES)
def test_conv_statistics_epilogue(ops, n, hw, cin, cout):
  """tg_conv2d_fwd_stats: the tensor is bit-identical to tg_conv2d_fwd's, and the per-workgroup partial sums add up
  to the sums of THAT tensor (value and square, per image and channel) -- fp32 summation error only.  Then the
  normaliser fed by those partials (tg_norm_act_fwd_conv_stats) equals the one that reads the tensor itself."""
  g = torch.Generator().manual_seed(5)
  x = (torch.randn(n, hw, hw, cin, generator=g) + 0.3).to(dev()).bfloat16()
  w = (torch.randn(3, 3, cin, cout, generator=g) * (2.0 / (9 * cin)) ** 0.5).to(dev())
  spec = ops.ConvSpec(3, 'SAME')
  y_ref = ops.conv_fwd_raw(x, w, None, spec, 0)
  y, st = ops.conv_fwd_stats_raw(x, w, spec)
  assert st is not None, 'this shape should dispatch a kernel with the statistics epilogue'
  assert torch.equal(y, y_ref)
  part = st.part.view(n, st.chunks, 2, cout).double().sum(dim=1).cpu().numpy()
  yd = y.double().cpu().numpy().reshape(n, hw * hw, cout)
  s1, s2 = yd.sum(axis=1), (yd * yd).sum(axis=1)
  assert np.abs(part[:, 0] - s1).max() <= 2e-6 * np.sqrt(s2 * hw * hw).max()
  assert np.abs(part[:, 1] / s2 - 1).max() <= 2e-6
  gamma = (1 + 0.1 * torch.randn(cout, generator=g)).to(dev())
  beta = (0.1 * torch.randn(cout, generator=g)).to(dev())
  pn = cout % 8 == 0 and (cout // 8) & (cout // 8 - 1) == 0      # the pixel-norm kernel wants c = 8 * 2^k
  z_ref = ops.norm_act(y, gamma, beta, pixel_norm=pn)
  z = ops.norm_act(y, gamma, beta, pixel_norm=pn, conv_stats=st)
  assert rel_l2(host(z), host(z_ref)) < 2e-3      # one bf16 rounding of the output is 1.1e-3; statistics differ by ~1e-6
  zp_ref = ops.norm_act(y, gamma, beta, pixel_norm=pn, pool=True)
  zp = ops.norm_act(y, gamma, beta, pixel_norm=pn, pool=True, conv_stats=st)
  assert rel_l2(host(zp[1]), host(zp_ref[1])) < 2e-3


def test_upcat_conv_statistics_epilogue(ops):
  g = torch.Generator().manual_seed(6)
  n, h, c0, c1, cout = 4, 32, 32, 32, 16
  x0 = torch.randn(n, h, h, c0, generator=g).to(dev()).bfloat16()
  x1 = torch.randn(2, 2 * h, 2 * h, c1, generator=g).to(dev()).bfloat16()
  w = (torch.randn(3, 3, c0 + c1, cout, generator=g) * (2.0 / (9 * (c0 + c1))) ** 0.5).to(dev())
  y_ref = ops.upcat_conv(x0, x1, w, 1, (1, 0, 0, 1))
  y, st = ops.upcat_conv_stats(x0, x1, w, 1, (1, 0, 0, 1))
  assert st is not None and torch.equal(y, y_ref)
  part = st.part.view(n, st.chunks, 2, cout).double().sum(dim=1).cpu().numpy()
  yd = y.double().cpu().numpy().reshape(n, 4 * h * h, cout)
  s2 = (yd * yd).sum(axis=1)
  assert np.abs(part[:, 0] - yd.sum(axis=1)).max() <= 2e-6 * np.sqrt(s2 * 4 * h * h).max()
  assert np.abs(part[:, 1] / s2 - 1).max() <= 2e-6


# ------------------------------------------------------------------------- conv that also writes its 2x2 average pool
@pytest.mark.parametrize('n,hw,cin,cout', [(4, 256, 16, 32), (5, 128, 32, 64), (3, 64, 64, 128), (2, 32, 128, 256),
                                           (3, 16, 256, 256), (2, 16, 40, 24)])
def test_conv_with_pooled_output(ops, monkeypatch, n, hw, cin, cout):
  """tg_conv2d_fwd_pool (last conv of a discriminator block + the avg_pool after it): z is bit-identical to
  tg_conv2d_fwd's, the pooled tensor equals tg_pool2x2_fwd of z (the 4 rounded values are added in another order: at
  most an ulp of bf16 on rare elements)."""
  from twingan_amd._lib import TG_EPI_BIAS, TG_EPI_LRELU
  g = torch.Generator().manual_seed(9)
  x = torch.randn(n, hw, hw, cin, generator=g).to(dev()).bfloat16()
  w = (torch.randn(3, 3, cin, cout, generator=g) * (2.0 / (9 * cin)) ** 0.5).to(dev())
  b = (0.1 * torch.randn(cout, generator=g)).to(dev())
  spec = ops.ConvSpec(3, 'SAME')
  epi = TG_EPI_BIAS | TG_EPI_LRELU
  monkeypatch.setattr(ops, 'USE_CONV_POOL', False)
  z_ref, zp_ref = ops.conv_fwd_pool_raw(x, w, b, spec, epi)
  monkeypatch.setattr(ops, 'USE_CONV_POOL', True)
  z, zp = ops.conv_fwd_pool_raw(x, w, b, spec, epi)
  from twingan_amd import _lib
  assert 'pool' in _lib.load().tg_last_kernel().decode()
  assert torch.equal(z, z_ref)
  assert rel_l2(host(zp), host(zp_ref)) < 1e-4
  assert float((zp.float() - zp_ref.float()).abs().max()) <= 2.0 ** -7 * float(zp_ref.float().abs().max())


def test_rccl_allreduce_wrapper_single_rank():
  """tg_comm_* / tg_allreduce (the C-ABI RCCL wrapper for callers without torch.distributed): a one-rank communicator on
  this GPU -- all a 1-GPU box allows -- initialises, sums in place (= identity for one rank) on a side stream, for fp32
  and bf16, and tears down.  RCCL is bound lazily: the library has no link dependency on it."""
  import ctypes
  from twingan_amd import _lib
  lib = _lib.load()
  nbytes = lib.tg_comm_unique_id_bytes()
  assert nbytes == 128
  uid = ctypes.create_string_buffer(nbytes)
  rc = lib.tg_comm_unique_id(ctypes.cast(uid, ctypes.c_void_p))
  assert rc == 0, lib.tg_last_error().decode()
  comm = ctypes.c_void_p()
  with torch.cuda.device(0):
    rc = lib.tg_comm_init(ctypes.cast(uid, ctypes.c_void_p), 1, 0, ctypes.byref(comm))
    assert rc == 0 and comm.value, lib.tg_last_error().decode()
    st = torch.cuda.Stream()
    for dt, code in ((torch.float32, _lib.TG_F32), (torch.bfloat16, _lib.TG_BF16)):
      x = torch.randn(1 << 20, device='cuda:0').to(dt)
      want = x.clone()
      st.wait_stream(torch.cuda.current_stream())
      rc = lib.tg_allreduce(comm, x.data_ptr(), x.numel(), code, st.cuda_stream)
      assert rc == 0, lib.tg_last_error().decode()
      st.synchronize()
      assert torch.equal(x, want)
    assert lib.tg_allreduce(comm, 0, 16, _lib.TG_F32, 0) != 0 and b'bad arguments' in lib.tg_last_error()
    assert lib.tg_comm_destroy(comm) == 0


# ------------------------------------------------------------------------- fp16 storage (TG_F16)
def f16_round(a):
  return np.asarray(a, np.float32).astype(np.float16).astype(np.float64)


F16_CASES = [
    # n, hw, cin, cout, k, padding   -> kernel family
    (4, 128, 16, 32, 3, 'SAME'),      # weight-resident thin kernel; thin (16x16x32 MFMA) filter gradient
    (4, 64, 32, 64, 3, 'SAME'),       # weight-resident, 64-channel blocks
    (3, 32, 64, 128, 3, 'SAME'),      # tile kernel
    (2, 16, 256, 256, 3, 'SAME'),     # tile kernel, two tiles per image
    (5, 8, 256, 256, 3, 'SAME'),      # small-map kernel
    (5, 4, 264, 256, 3, 'SAME'),
    (6, 4, 64, 64, 4, 'VALID'),       # dense rewrite
    (1, 20, 24, 40, 3, 'SAME'),       # (20 x 12 map) first-generation fallback kernels
    (2, 12, 32, 48, 1, 'SAME'),
]


@pytest.mark.parametrize('n,hw,cin,cout,k,padding', F16_CASES)
def test_fp16_conv_kernels_vs_oracle(ops, n, hw, cin, cout, k, padding):
  """TG_F16 through the same MFMA kernels as bf16 (v_mfma_f32_*_f16 instead of *_bf16): forward with bias + LeakyReLU,
  backward-data plain and with the producer's mask, filter gradient with and without the bias gradient, against the
  float64 oracle on fp16-rounded operands.  fp16 keeps 11 significand bits: outputs within 6e-4 (one rounding is
  2.4e-4), fp32-accumulated filter / bias gradients within 1e-4."""
  import twingan_amd.ops as O
  from twingan_amd import _lib
  from twingan_amd._lib import TG_EPI_BIAS, TG_EPI_LRELU
  rng = np.random.RandomState(4)
  h = w = hw
  if (n, hw, cin) == (1, 20, 24):
    w = 12
  x = f16_round(rng.randn(n, h, w, cin))
  wt = f16_round(rng.randn(k, k, cin, cout) / np.sqrt(k * k * cin))
  b = rng.randn(cout) * 0.1
  spec = O.ConvSpec(k, padding)
  ho, wo = spec.out_hw(h, w)
  gy = f16_round(rng.randn(n, ho, wo, cout))
  xd, gyd = to_dev(x, torch.float16), to_dev(gy, torch.float16)
  wd, bd = to_dev(wt), to_dev(b)
  assert O._mfma_ok(torch.float16, cin, cout, spec, h, w)
  y = O.conv_fwd_raw(xd, wd, bd, spec, TG_EPI_BIAS | TG_EPI_LRELU)
  kern = _lib.load().tg_last_kernel().decode()
  assert 'f16' in kern, kern
  assert rel_l2(host(y), N.leaky_relu(N.conv2d(x, wt, padding) + b)) < 6e-4
  gx = O.conv_bwd_data_raw(gyd, wd, (n, h, w, cin), spec)
  ref_gx = N.conv2d_bwd_data(gy, wt, (h, w), padding)
  assert rel_l2(host(gx), ref_gx) < 6e-4
  if k == 3 and padding == 'SAME':
    gxm = O.conv_bwd_data_masked_raw(gyd, wd, xd, spec)
    assert rel_l2(host(gxm), ref_gx * np.where(x > 0, 1.0, 0.2)) < 8e-4
  gw = O.conv_bwd_weight_raw(xd, gyd, spec)
  assert rel_l2(host(gw), N.conv2d_bwd_weight(x, gy, (k, k), padding)) < 1e-4
  if k == 3 and padding == 'SAME' and hw >= 16 and h == w:      # layers whose filter-gradient kernel also sums gy (bias gradient)
    gb = torch.zeros(cout, device=dev())
    gw2 = O.conv_bwd_weight_raw(xd, gyd, spec, gbias=gb)
    assert rel_l2(host(gw2), host(gw)) < 1e-6 and rel_l2(host(gb), gy.sum(axis=(0, 1, 2))) < 1e-4
  # the bf16 instantiation is untouched by the element format of the previous calls
  yb = O.conv_fwd_raw(xd.bfloat16(), wd, bd, spec, TG_EPI_BIAS | TG_EPI_LRELU)
  assert 'f16' not in _lib.load().tg_last_kernel().decode()
  assert rel_l2(host(yb), host(y)) < 6e-3


@pytest.mark.parametrize('n,hw,c', [(3, 16, 32), (2, 64, 16), (4, 4, 256)])
def test_fp16_norm_pointwise_and_attention_pieces(ops, n, hw, c):
  rng = np.random.RandomState(6)
  y = f16_round(rng.randn(n, hw, hw, c) * 1.5 + 0.3)
  g, b = 1 + 0.1 * rng.randn(c), 0.1 * rng.randn(c)
  yd = to_dev(y, torch.float16).requires_grad_(True)
  gd, bd = to_dev(g).requires_grad_(True), to_dev(b).requires_grad_(True)
  z = ops.norm_act(yd, gd, bd)
  ref = N.pixel_norm(N.leaky_relu(N.instance_norm(y, g, b)))
  assert z.dtype == torch.float16 and rel_l2(host(z), ref) < 8e-4
  gz = f16_round(rng.randn(*y.shape))
  z.backward(to_dev(gz, torch.float16))
  yt = torch.tensor(y, dtype=torch.float64, requires_grad=True)
  gt, bt = torch.tensor(g, requires_grad=True), torch.tensor(b, requires_grad=True)
  from oracle import torch_ref as R
  zr = R.pixel_norm(torch.nn.functional.leaky_relu(R.instance_norm(yt, gt, bt), 0.2))
  zr.backward(torch.tensor(gz))
  assert rel_l2(host(yd.grad), yt.grad.numpy()) < 2e-3
  assert rel_l2(host(gd.grad), gt.grad.numpy()) < 1e-3 and rel_l2(host(bd.grad), bt.grad.numpy()) < 1e-3
  # fromRGB / toRGB and the batched GEMM of the attention layer
  x3 = to_dev(f16_round(rng.rand(n, hw, hw, 3)), torch.float16)
  w3 = to_dev(rng.randn(1, 1, 3, c) * 0.5)
  assert rel_l2(host(ops.pointwise_conv(x3, w3)), N.conv2d(host(x3), host(w3), 'SAME')) < 6e-4
  a = to_dev(f16_round(rng.randn(n, 40, 24)), torch.float16)
  bm = to_dev(f16_round(rng.randn(n, 24, 56)), torch.float16)
  assert rel_l2(host(ops.bgemm(a, bm)), host(a) @ host(bm)) < 6e-4


# ------------------------------------------------------------------------- flash attention
def _attention_ref(q, k, v):
  s = np.einsum('nid,njd->nij', q, k)
  s = s - s.max(axis=-1, keepdims=True)
  p = np.exp(s)
  p /= p.sum(axis=-1, keepdims=True)
  return np.einsum('nij,njd->nid', p, v)


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
@pytest.mark.parametrize('n,ln,dk,dv', [(2, 256, 8, 64), (1, 1024, 16, 128), (3, 128, 8, 256)])
def test_flash_attention_forward(ops, dtype, n, ln, dk, dv):
  """tg_flash_attention_fwd against softmax(q k^T) v in float64 on the 16-bit-rounded operands: the map is never
  written, the softmax statistics stay fp32 (the composed path rounds the scores to 16 bit first)."""
  rng = np.random.RandomState(7)
  rnd = bf16_round if dtype == torch.bfloat16 else f16_round
  q, k, v = rnd(np.tanh(rng.randn(n, ln, dk))), rnd(np.tanh(rng.randn(n, ln, dk) * 2)), rnd(rng.randn(n, ln, dv))
  qd, kd, vd = (to_dev(t, dtype) for t in (q, k, v))
  assert ops.flash_attention_supported(qd, vd)
  o, lse = ops.flash_attention_fwd_raw(qd, kd, vd)
  ref = _attention_ref(q, k, v)
  tol = 6e-3 if dtype == torch.bfloat16 else 8e-4      # P is rounded to the storage type before the second product
  assert rel_l2(host(o), ref) < tol
  s = np.einsum('nid,njd->nij', q, k)
  want = np.log(np.exp(s - s.max(-1, keepdims=True)).sum(-1)) + s.max(-1)
  # the row sums are sums of the 16-bit-rounded probabilities (the MFMA unit adds them up), as the numerator's are
  assert np.abs(host(lse) - want).max() < (2e-3 if dtype == torch.bfloat16 else 3e-4)


def _attention_grads_ref(q, k, v, go):
  s = np.einsum('nid,njd->nij', q, k)
  p = np.exp(s - s.max(-1, keepdims=True))
  p /= p.sum(-1, keepdims=True)
  gv = np.einsum('nij,nid->njd', p, go)
  gp = np.einsum('nid,njd->nij', go, v)
  gs = p * (gp - (gp * p).sum(-1, keepdims=True))
  return np.einsum('nij,njd->nid', gs, k), np.einsum('nij,nid->njd', gs, q), gv


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
@pytest.mark.parametrize('n,ln,dk,dv', [(2, 256, 8, 64), (1, 512, 16, 128), (3, 128, 16, 64)])
def test_flash_attention_backward(ops, dtype, n, ln, dk, dv):
  """tg_flash_attention_bwd (dq, dk, dv) against the float64 softmax-attention gradients, and against the composed
  batched-GEMM / softmax path's own gradients on the same inputs (both 16-bit; the flash path keeps fp32 scores)."""
  rng = np.random.RandomState(11)
  rnd = bf16_round if dtype == torch.bfloat16 else f16_round
  q, k, v = rnd(np.tanh(rng.randn(n, ln, dk))), rnd(np.tanh(rng.randn(n, ln, dk) * 2)), rnd(rng.randn(n, ln, dv))
  go = rnd(rng.randn(n, ln, dv))
  qd, kd, vd = (to_dev(t, dtype).requires_grad_(True) for t in (q, k, v))
  assert ops.flash_attention_trainable(qd, vd)
  o = ops.flash_attention(qd, kd, vd)
  gq, gk, gv = torch.autograd.grad(o, (qd, kd, vd), to_dev(go, dtype))
  rq, rk, rv = _attention_grads_ref(q, k, v, go)
  tol = 1.2e-2 if dtype == torch.bfloat16 else 2e-3
  for got, ref, nm in ((gq, rq, 'dq'), (gk, rk, 'dk'), (gv, rv, 'dv')):
    assert rel_l2(host(got), ref) < tol, nm
  oc = ops.bgemm(ops.softmax_rows(ops.bgemm(qd, kd, False, True)), vd, False, False)
  cq, ck, cv = torch.autograd.grad(oc, (qd, kd, vd), to_dev(go, dtype))
  for got, ref, cmp_, nm in ((gq, rq, cq, 'dq'), (gk, rk, ck, 'dk'), (gv, rv, cv, 'dv')):
    assert rel_l2(host(got), ref) <= rel_l2(host(cmp_), ref) * 1.5 + 1e-4, nm      # at least as close as the composed path


def _attention_second_order_ref(q, k, v, go, aq, ak, av):
  """Gradients of <dq, aq> + <dk, ak> + <dv, av> (dq, dk, dv = the attention backward) wrt q, k, v, go: torch autograd
  in float64 on the CPU (oracle/np_ops.attention_backward_backward is the closed form of the same, pinned against this
  in tests/test_oracle.py)."""
  t = [torch.tensor(x, dtype=torch.float64, requires_grad=True) for x in (q, k, v, go)]
  tq, tk, tv, tg = t
  o = torch.softmax(tq @ tk.transpose(1, 2), -1) @ tv
  gq, gk, gv = torch.autograd.grad(o, (tq, tk, tv), tg, create_graph=True)
  loss = (gq * torch.tensor(aq)).sum() + (gk * torch.tensor(ak)).sum() + (gv * torch.tensor(av)).sum()
  return [x.numpy() for x in torch.autograd.grad(loss, t)]


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
@pytest.mark.parametrize('n,ln,dk,dv', [(2, 256, 8, 64), (1, 128, 16, 128)])
def test_flash_attention_second_order(ops, dtype, n, ln, dk, dv):
  """The gradient-penalty pattern through a flash node: create_graph backward (FlashAttnBwdFn) and then the backward of
  that (tg_flash_attention_bwd_bwd), against float64 autograd of the same composition and against the batched-GEMM /
  softmax path's own double backward."""
  rng = np.random.RandomState(5)
  rnd = bf16_round if dtype == torch.bfloat16 else f16_round
  q, k = rnd(np.tanh(rng.randn(n, ln, dk))), rnd(np.tanh(rng.randn(n, ln, dk) * 2))
  v, go = rnd(rng.randn(n, ln, dv)), rnd(rng.randn(n, ln, dv))
  aq, ak, av = rnd(rng.randn(n, ln, dk)), rnd(rng.randn(n, ln, dk)), rnd(rng.randn(n, ln, dv))
  ref = _attention_second_order_ref(q, k, v, go, aq, ak, av)
  res = {}
  for flash in (True, False):
    qd, kd, vd, gd = (to_dev(t, dtype).requires_grad_(True) for t in (q, k, v, go))
    if flash:
      with ops.second_order():
        assert ops.flash_attention_trainable(qd, vd) == ops.USE_FLASH_BWD_BWD
      o = ops.flash_attention(qd, kd, vd)
    else:
      o = ops.bgemm(ops.softmax_rows(ops.bgemm(qd, kd, False, True)), vd, False, False)
    gq, gk, gv = torch.autograd.grad(o, (qd, kd, vd), gd, create_graph=True)
    loss = (gq.float() * to_dev(aq, torch.float32)).sum() + (gk.float() * to_dev(ak, torch.float32)).sum() + \
        (gv.float() * to_dev(av, torch.float32)).sum()
    res[flash] = [host(t) for t in torch.autograd.grad(loss, (qd, kd, vd, gd))]
  tol = 2.5e-2 if dtype == torch.bfloat16 else 4e-3
  for got, cmp_, want, nm in zip(res[True], res[False], ref, ('adj q', 'adj k', 'adj v', 'adj dO')):
    e, ec = rel_l2(got, want), rel_l2(cmp_, want)
    print('[flash2] %s %s: flash %.2e composed %.2e' % (dtype, nm, e, ec))
    assert e < tol and e <= ec * 1.5 + 1e-4, (nm, e, ec)


# --------------------------------------------------------------- thin-output kernel (<= 16 output channels, TG_THIN16=1)
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
@pytest.mark.parametrize('cin,cout', [(16, 16), (32, 16), (16, 8)])
def test_thin_output_kernel_matches_the_wide_block_kernels(ops, monkeypatch, dtype, cin, cout):
  """conv_thin16_kernel (v_mfma_f32_16x16x32, weights in registers; an A/B switch, off by default): forward with bias +
  LeakyReLU, forward with the statistics epilogue, backward-data with and without the LeakyReLU mask -- against the
  32-wide-block kernels the dispatch uses otherwise (same products, another summation order inside the MFMA: <= 2e-3) and
  against the float64 oracle on the same rounded operands."""
  import twingan_amd.ops as O
  from twingan_amd import _lib
  from twingan_amd._lib import TG_EPI_BIAS, TG_EPI_LRELU
  n, hw = 16, 128      # 2048 tiles: where the dispatch goes to the thin kernels
  g = torch.Generator().manual_seed(17)
  x = torch.randn(n, hw, hw, cin, generator=g).to(dtype).to(dev())
  w = (torch.randn(3, 3, cin, cout, generator=g) * (2.0 / (9 * cin)) ** 0.5).to(dev())
  b = (torch.randn(cout, generator=g) * 0.1).to(dev())
  spec = O.ConvSpec(3, 'SAME')
  f16 = ',f16' if dtype == torch.float16 else ''

  def both(fn):
    out = []
    for on in ('0', '1'):
      monkeypatch.setenv('TG_THIN16', on)
      out.append((fn(), _lib.load().tg_last_kernel().decode()))
    monkeypatch.setenv('TG_THIN16', '0')
    return out
  (ya, ka), (yb, kb) = both(lambda: O.conv_fwd_raw(x, w, b, spec, TG_EPI_BIAS | TG_EPI_LRELU))
  assert 'thin16' not in ka and kb == 'conv_thin16_kernel<%d%s>' % (cin, f16), (ka, kb)
  assert rel_l2(host(yb), host(ya)) < 2e-3
  rnd = bf16_round if dtype == torch.bfloat16 else f16_round
  sub = slice(0, 2)      # the oracle on two images
  ref = N.leaky_relu(N.conv2d(host(x[sub]), rnd(host(w)), 'SAME') + host(b))
  assert rel_l2(host(yb[sub]), ref) < (6e-3 if dtype == torch.bfloat16 else 8e-4)
  if cout % 8 == 0:
    ((y1, s1), k1), ((y2, s2), k2) = both(lambda: O.conv_fwd_stats_raw(x, w, spec))
    assert k2 == 'conv_thin16_kernel<%d,stats%s>' % (cin, f16), k2
    assert rel_l2(host(y2), host(y1)) < 2e-3
    part = s2.part.view(n, s2.chunks, 2, cout).double().sum(dim=1).cpu().numpy()
    yd = y2.double()
    want = torch.stack([yd.sum(dim=(1, 2)), (yd * yd).sum(dim=(1, 2))], dim=1).cpu().numpy()
    assert rel_l2(part, want) < 1e-5      # the partials are sums of THIS tensor
  if cin <= 16:      # backward-data of this layer writes cin <= 16 channels: thin as well
    gy = torch.randn(n, hw, hw, cout, generator=g).to(dtype).to(dev())
    if cout == 16:
      (ga, _), (gb, k3) = both(lambda: O.conv_bwd_data_masked_raw(gy, w, x, spec))
      assert k3 == 'conv_thin16_kernel<16%s>' % f16, k3
      assert rel_l2(host(gb), host(ga)) < 2e-3
      want_g = N.conv2d_bwd_data(host(gy[sub]), rnd(host(w)), (hw, hw), 'SAME') * np.where(host(x[sub]) > 0, 1.0, 0.2)
      assert rel_l2(host(gb[sub]), want_g) < (6e-3 if dtype == torch.bfloat16 else 8e-4)


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
def test_thin_output_kernel_over_the_concat_input(ops, monkeypatch, dtype):
  """conv_thin16_upcat_kernel (TG_THIN16=1): the generator's concat conv with 16 outputs -- concat(nearest_up2(x0), skip),
  32 + 32 channels read in place, groups permuted as the trainer does -- forward with and without the statistics epilogue
  against the 32-wide-block UPCAT kernels (<= 2e-3: another summation order inside the MFMA)."""
  from twingan_amd import _lib
  g = torch.Generator().manual_seed(19)
  b, h, c0, c1, cout = 4, 64, 32, 32, 16      # 4 groups of 4 images at 128 x 128: 2048 tiles
  n = 4 * b
  x0 = torch.randn(n, h, h, c0, generator=g).to(dtype).to(dev())
  x1 = torch.randn(2 * b, 2 * h, 2 * h, c1, generator=g).to(dtype).to(dev())
  w = (torch.randn(3, 3, c0 + c1, cout, generator=g) * (2.0 / (9 * (c0 + c1))) ** 0.5).to(dev())
  f16 = ',f16' if dtype == torch.float16 else ''
  res = {}
  for on in ('0', '1'):
    monkeypatch.setenv('TG_THIN16', on)
    y_plain = ops.upcat_conv(x0, x1, w, b, (1, 0, 0, 1))
    k_plain = _lib.load().tg_last_kernel().decode()
    y, st = ops.upcat_conv_stats(x0, x1, w, b, (1, 0, 0, 1))
    res[on] = (y_plain, k_plain, y, st, _lib.load().tg_last_kernel().decode())
  monkeypatch.setenv('TG_THIN16', '0')
  assert 'thin16' not in res['0'][1] and res['1'][1] == 'conv_thin16_upcat_kernel<plain%s>' % f16, (res['0'][1], res['1'][1])
  assert res['1'][4] == 'conv_thin16_upcat_kernel<stats%s>' % f16
  y_plain, _, y, st, _ = res['1']
  assert st is not None and torch.equal(y, y_plain)
  assert rel_l2(host(y), host(res['0'][2])) < 2e-3
  part = st.part.view(n, st.chunks, 2, cout).double().sum(dim=1).cpu().numpy()
  yd = y.double()
  want = torch.stack([yd.sum(dim=(1, 2)), (yd * yd).sum(dim=(1, 2))], dim=1).cpu().numpy()
  assert rel_l2(part, want) < 1e-5
  # the float64 oracle on the first image of the last group (skip group 1)
  up = host(x0[3 * b:3 * b + 1]).repeat(2, axis=1).repeat(2, axis=2)
  cat = np.concatenate([up, host(x1[b:b + 1])], axis=-1)
  rnd = bf16_round if dtype == torch.bfloat16 else f16_round
  ref = N.conv2d(cat, rnd(host(w)), 'SAME')
  assert rel_l2(host(y[3 * b:3 * b + 1]), ref) < (6e-3 if dtype == torch.bfloat16 else 8e-4)


# ------------------------------------------------ backward-data of a block's last conv from the pooled gradient + sign bytes
UNPOOL_CASES = [
    # n, hw, cin, cout, masked, kernel the dispatch picks (bf16 name)
    (2, 16, 16, 32, True, 'conv_tile_kernel<3,32,32,1,unpool>'),
    (1, 32, 32, 64, False, 'conv_tile_kernel<3,32,32,1,unpool>'),
    (2, 16, 128, 256, True, 'conv_tile_kernel<3,32,32,1,unpool>'),
    (16, 64, 64, 128, True, 'conv_tile_kernel<3,32,32,2,unpool>'),     # two sub-tiles per wave (>= 1024 tiles, cin_pad >= 64)
    (32, 64, 64, 32, True, 'conv_tile_kernel<3,32,64,1,unpool>'),      # 64-channel output blocks
    (32, 64, 64, 128, False, 'conv_tile_kernel<3,32,64,2,unpool>'),
    (16, 128, 16, 32, True, 'conv_tile_wres_kernel<3,32,32,1,unpool>'),      # weight-resident thin kernel (the 256 x 256 block end)
    (1, 48, 16, 32, True, 'conv_tile_kernel<3,32,32,1,unpool>'),       # 48 rows / columns: three column tiles
]


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
@pytest.mark.parametrize('case', range(len(UNPOOL_CASES)))
def test_unpool_backward_data_equals_the_two_launch_path(ops, dtype, case):
  """tg_conv2d_bwd_data_unpool: the backward-data of a discriminator block's last conv (nets/pggan.py:304-306) with
  AvgPoolGrad + LeakyReluGrad applied while its tiles are staged -- bit-identical to tg_lrelu_pool_bwd_signs followed by
  tg_conv2d_bwd_data(_masked) for every kernel variant the dispatch picks, and within the rounding bound of the float64
  oracle evaluated on the same rounded operands."""
  import twingan_amd.ops as O
  from twingan_amd import _lib
  n, hw, cin, cout, masked, want = UNPOOL_CASES[case]
  g = torch.Generator().manual_seed(300 + case)
  spec = O.ConvSpec(3, 'SAME')
  x = torch.randn(n, hw, hw, cin, generator=g).to(dtype).to(dev())               # the conv's forward input: the mask source
  w = (torch.randn(3, 3, cin, cout, generator=g) * (2.0 / (9 * cin)) ** 0.5).to(dev())
  gzp = torch.randn(n, hw // 2, hw // 2, cout, generator=g).to(dtype).to(dev())
  gzp[0, 0, 0, :8] = 0.0                                                         # zeros stay zeros whatever their sign bit
  signs = torch.randint(0, 256, (n, hw, hw, cout // 8), generator=g, dtype=torch.uint8).to(dev())
  g2, _ = O.lrelu_pool_bwd_signs(gzp, signs, spec.alpha, None, False)
  ref = O.conv_bwd_data_masked_raw(g2, w, x, spec) if masked else O.conv_bwd_data_raw(g2, w, (n, hw, hw, cin), spec)
  got = O.conv_bwd_data_unpool_raw(gzp, signs, w, x if masked else None, (n, hw, hw, cin), spec)
  assert got is not None, 'the tile kernels take this layer'
  sym = _lib.load().tg_last_kernel().decode()
  assert sym == (want if dtype == torch.bfloat16 else want.replace('unpool', 'unpool,f16')), sym
  assert torch.equal(got, ref), float((got.float() - ref.float()).abs().max())
  # keep mode (a discriminator step): the same kernel also writes the gradient tensor itself, each element exactly once
  got2, g2w = O.conv_bwd_data_unpool_raw(gzp, signs, w, x if masked else None, (n, hw, hw, cin), spec, True)
  assert _lib.load().tg_last_kernel().decode() == sym
  assert torch.equal(got2, ref) and torch.equal(g2w, g2), float((g2w.float() - g2.float()).abs().max())
  # the signs taken from the activation tensor itself (a pass that kept it): same kernels, 'unpoolz'
  zact = torch.randn(n, hw, hw, cout, generator=g).to(dtype).to(dev())
  zact[0, 0, :, :4] = 0.0                                                        # exact zeros count as "not positive"
  g3, _ = O.lrelu_pool_bwd(None, gzp, zact, spec.alpha, None, False)
  ref3 = O.conv_bwd_data_masked_raw(g3, w, x, spec) if masked else O.conv_bwd_data_raw(g3, w, (n, hw, hw, cin), spec)
  got3, g3w = O.conv_bwd_data_unpool_raw(gzp, zact, w, x if masked else None, (n, hw, hw, cin), spec, True)
  assert _lib.load().tg_last_kernel().decode() == sym.replace('unpool', 'unpoolz')
  assert torch.equal(got3, ref3) and torch.equal(g3w, g3)
  if n * hw * hw * cout <= 1 << 21:      # the float64 oracle on the small cases
    bits = ((signs.to(torch.int32).unsqueeze(-1) >> torch.arange(8, dtype=torch.int32, device=signs.device)) & 1).reshape(n, hw, hw, cout)
    up = host(gzp).repeat(2, axis=1).repeat(2, axis=2) * 0.25 * np.where(host(bits) > 0, 1.0, 0.2)
    rnd = bf16_round if dtype == torch.bfloat16 else f16_round
    wr = rnd(host(w))
    want_gx = N.conv2d_bwd_data(rnd(up), wr, (hw, hw), 'SAME')
    if masked:
      want_gx = want_gx * np.where(host(x) > 0, 1.0, 0.2)
    assert rel_l2(host(got), want_gx) < (4e-3 if dtype == torch.bfloat16 else 5e-4)


@pytest.mark.parametrize('train_d', [False, True])
def test_backward_through_a_block_end_uses_the_unpool_kernel(ops, train_d):
  """A discriminator block end: conv2d(pool_only=True) backpropagates through tg_conv2d_bwd_data_unpool -- differentiated for
  its INPUT only (a generator step: the discriminator's parameters are frozen) the layer's gradient is never in memory;
  with the filter and bias gradients wanted too (a discriminator step) the same kernel writes it for them.  Every gradient
  equals the two-launch path's (TG_DGRAD_UNPOOL=0): the input gradient bit for bit, the parameter gradients to fp32
  summation order."""
  import twingan_amd.ops as O
  g = torch.Generator().manual_seed(41)
  n, hw, cin, cout = 2, 32, 32, 64
  x0 = torch.randn(n, hw, hw, cin, generator=g).bfloat16().to(dev())
  w0 = (torch.randn(3, 3, cin, cout, generator=g) * (2.0 / (9 * cin)) ** 0.5).to(dev())
  b0 = (torch.randn(cout, generator=g) * 0.1).to(dev())
  gz = torch.randn(n, hw // 2, hw // 2, cout, generator=g).bfloat16().to(dev())
  res, used = {}, []
  real = O.conv_bwd_data_unpool_raw

  def counted(*a, **k):
    out = real(*a, **k)
    used.append(out is not None)
    return out
  saved = O.USE_DGRAD_UNPOOL
  O.conv_bwd_data_unpool_raw = counted
  try:
    for on in (True, False):
      O.USE_DGRAD_UNPOOL = on
      x = x0.clone().requires_grad_(True)
      w, b = w0.clone().requires_grad_(train_d), b0.clone().requires_grad_(train_d)
      out = O.conv2d(x, w, b, 3, 'SAME', lrelu=True, pool=True, pool_only=True)
      zp = out[1] if isinstance(out, tuple) else out
      zp.backward(gz)
      res[on] = (x.grad, w.grad, b.grad)
  finally:
    O.USE_DGRAD_UNPOOL = saved
    O.conv_bwd_data_unpool_raw = real
  assert used == [True]
  assert torch.equal(res[True][0], res[False][0])
  if train_d:
    assert rel_l2(host(res[True][1]), host(res[False][1])) < 1e-5 and rel_l2(host(res[True][2]), host(res[False][2])) < 1e-5


# ------------------------------------------------------------------------- sign bits instead of a pooled layer's output
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
@pytest.mark.parametrize('n,hw,cin,cout', [(3, 32, 16, 32), (2, 16, 64, 64), (2, 64, 16, 24), (5, 16, 32, 72), (1, 16, 256, 256)])
def test_conv_pool_sign_bits(ops, dtype, n, hw, cin, cout):
  """tg_conv2d_fwd_pool_signs / tg_lrelu_pool_bwd_signs (the discriminator blocks' last conv when the pool is the only
  consumer of its output, nets/pggan.py:304-306): the pooled tensor equals tg_conv2d_fwd_pool's bit for bit, the sign
  bytes are (z > 0) of the z that launch stores (incl. a channel count that ends on a lone byte: 24, 72), and the
  LeakyReLU + unpool backward rebuilt from the bits equals the one rebuilt from z -- both against the float64 oracle
  too.  Zeros in z (bias-free rows that cancel) count as "not positive", as lrelu'(0) = alpha in util_misc.py:86."""
  import twingan_amd.ops as O
  from twingan_amd._lib import TG_EPI_BIAS, TG_EPI_LRELU
  rng = np.random.RandomState(31)
  rnd = bf16_round if dtype == torch.bfloat16 else f16_round
  x = rnd(rng.randn(n, hw, hw, cin))
  x[0, :4] = 0.0                                   # a patch whose pre-activation is exactly the bias
  w = rnd(rng.randn(3, 3, cin, cout) / np.sqrt(9 * cin))
  b = rng.randn(cout) * 0.1
  b[:3] = 0.0                                      # ... which is zero for three channels: z == 0 there
  xd, wd, bd = to_dev(x, dtype), to_dev(w), to_dev(b)
  spec = O.ConvSpec(3, 'SAME')
  epi = TG_EPI_BIAS | TG_EPI_LRELU
  assert O.conv_fwd_pool_signs_supported(xd, wd, spec, epi)
  z, zp = O.conv_fwd_pool_raw(xd, wd, bd, spec, epi)
  signs, zp2 = O.conv_fwd_pool_signs_raw(xd, wd, bd, spec, epi)
  assert torch.equal(zp, zp2)
  assert signs.shape == (n, hw, hw, cout // 8) and signs.dtype == torch.uint8
  bits = (z > 0).view(n, hw, hw, cout // 8, 8).to(torch.int32)
  want = (bits << torch.arange(8, device=z.device, dtype=torch.int32)).sum(dim=-1).to(torch.uint8)
  assert torch.equal(signs, want), int((signs != want).sum())
  assert int((z[0, :3, :, :3] == 0).sum()) > 0      # the zero case is really in the data
  ref = N.leaky_relu(N.conv2d(x, w, 'SAME') + b)
  assert rel_l2(host(z), ref) < (6e-3 if dtype == torch.bfloat16 else 8e-4)
  gzp = rnd(rng.randn(n, hw // 2, hw // 2, cout))
  gd = to_dev(gzp, dtype)
  g_ref, gb_ref = O.lrelu_pool_bwd(None, gd, z, 0.2, bd, True)
  g_sig, gb_sig = O.lrelu_pool_bwd_signs(gd, signs, 0.2, bd, True)
  assert torch.equal(g_sig, g_ref)
  up = np.repeat(np.repeat(gzp, 2, axis=1), 2, axis=2) * 0.25
  want_g = up * np.where(host(z) > 0, 1.0, 0.2)
  assert rel_l2(host(g_sig), want_g) < (4e-3 if dtype == torch.bfloat16 else 5e-4)
  assert rel_l2(host(gb_sig), host(g_sig).sum(axis=(0, 1, 2))) < 1e-5 and rel_l2(host(gb_sig), host(gb_ref)) < 1e-5
  # through autograd: conv2d(pool_only=True) -> (None, pooled); its gradients equal the z-keeping node's
  res = {}
  for only in (True, False):
    xa = xd.clone().requires_grad_(True)
    wa, ba = wd.clone().requires_grad_(True), bd.clone().requires_grad_(True)
    full, pooled = O.conv2d(xa, wa, ba, 3, 'SAME', lrelu=True, pool=True, pool_only=only)
    assert (full is None) == only
    pooled.backward(gd)
    res[only] = (pooled.detach(), xa.grad, wa.grad, ba.grad)
  assert torch.equal(res[True][0], res[False][0]) and torch.equal(res[True][1], res[False][1])
  assert rel_l2(host(res[True][2]), host(res[False][2])) < 1e-6 and rel_l2(host(res[True][3]), host(res[False][3])) < 1e-5
  # a create_graph pass keeps z
  with O.second_order():
    full, _ = O.conv2d(xd, wd, bd, 3, 'SAME', lrelu=True, pool=True, pool_only=True)
  assert full is not None


# ------------------------------------------------------------------------- ordered (fixed-order) sums
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16, torch.float32])
def test_ordered_sums_are_bit_reproducible_and_right(ops, dtype):
  """tg_channel_sum_ordered / tg_sum_ordered / tg_pointwise_conv_bwd_weight_ordered (what deterministic mode routes the
  bias gradients, loss sums and fromRGB / toRGB filter gradients through): per-workgroup partials in a workspace added in
  workgroup order -- the same bits on every call (the atomic forms differ run to run in their last ulp at these sizes),
  the float64 value to fp32 summation error, also with fewer workspace rows than workgroups wanted."""
  import twingan_amd.ops as O
  from twingan_amd import _lib
  lib = _lib.load()
  rng = np.random.RandomState(41)
  n, hw, c = 6, 64, 32
  g = rng.randn(n, hw, hw, c).astype(np.float32)
  gd = to_dev(g, dtype)
  gref = host(gd)
  st = torch.cuda.current_stream().cuda_stream
  dt = O._dt(gd)
  outs = []
  for rows in (512, 512, 7):
    ws = torch.empty(rows * c, dtype=torch.float32, device='cuda')
    out = torch.full((c,), 3.0, dtype=torch.float32, device='cuda')
    O.call('tg_channel_sum_ordered', gd.data_ptr(), out.data_ptr(), n * hw * hw, c, 1, ws.data_ptr(), ws.numel(), dt, st)
    outs.append(out.clone())
    assert rel_l2(host(out) - 3.0, gref.sum(axis=(0, 1, 2))) < 2e-6
  assert torch.equal(outs[0], outs[1])
  # loss sums
  a, b = gd, to_dev(rng.randn(n, hw, hw, c).astype(np.float32), dtype)
  vals = []
  for _ in range(2):
    ws = torch.empty(512, dtype=torch.float32, device='cuda')
    o1 = torch.empty(1, dtype=torch.float32, device='cuda')
    o2 = torch.empty(1, dtype=torch.float32, device='cuda')
    O.call('tg_sum_ordered', a.data_ptr(), None, o1.data_ptr(), a.numel(), 0.5, 0, ws.data_ptr(), ws.numel(), dt, st)
    O.call('tg_sum_ordered', a.data_ptr(), b.data_ptr(), o2.data_ptr(), a.numel(), 2.0, 0, ws.data_ptr(), ws.numel(), dt, st)
    vals.append((float(o1), float(o2)))
  assert vals[0] == vals[1]
  assert abs(vals[0][0] - 0.5 * host(a).sum()) < 1e-5 * np.abs(host(a)).sum()
  assert abs(vals[0][1] - 2.0 * np.abs(host(a) - host(b)).sum()) < 1e-5 * 2.0 * np.abs(host(a) - host(b)).sum()
  # fromRGB filter gradient (cin 3) and toRGB (cout 3)
  if dtype != torch.float32:
    x3 = to_dev(rng.rand(n, hw, hw, 3).astype(np.float32), dtype)
    for xa, xb in ((x3, gd), (gd, x3)):
      ca, cb = xa.shape[-1], xb.shape[-1]
      res = []
      for _ in range(2):
        ws = torch.empty(256 * ca * cb, dtype=torch.float32, device='cuda')
        gw = torch.zeros((ca, cb), dtype=torch.float32, device='cuda')
        O.call('tg_pointwise_conv_bwd_weight_ordered', xa.data_ptr(), xb.data_ptr(), gw.data_ptr(), n * hw * hw, ca, cb, 1,
               ws.data_ptr(), ws.numel(), dt, st)
        res.append(gw.clone())
      assert torch.equal(res[0], res[1])
      want = host(xa).reshape(-1, ca).T @ host(xb).reshape(-1, cb)
      assert rel_l2(host(res[0]), want) < 2e-6
  # the host routes through them exactly when the mode is on
  was = lib.tg_set_deterministic(1)
  try:
    assert O.deterministic()
    s1, s2 = O.channel_sum_raw(gd), O.channel_sum_raw(gd)
    assert torch.equal(s1, s2)
  finally:
    lib.tg_set_deterministic(was)
  assert O.deterministic() == bool(was)


def test_deferred_slab_reductions_equal_immediate_ones(ops):
  """tg_wgrad_defer / tg_wgrad_defer_flush: the split-K slab reductions of filter gradients that accumulate into a sink are
  queued and issued as ONE launch.  Each job keeps the slice-group shape and summation order of its stand-alone kernel, so
  a sink that starts at zero receives the same bits; two jobs into one sink add up; a queue of more than 120 jobs falls
  back to immediate launches for the rest; outside a defer window nothing changes."""
  spec = ops.ConvSpec(3, 'SAME')
  g = torch.Generator(device='cpu').manual_seed(5)
  cases = [(4, 16, 16, 32, 32), (8, 32, 32, 64, 64), (2, 64, 64, 16, 16), (16, 8, 8, 256, 256), (4, 16, 16, 512, 256)]
  data = []
  for n, h, w, cin, cout in cases:      # weight sizes on both sides of the 16 384 / 131 072 element thresholds
    x = torch.randn(n, h, w, cin, generator=g).to(dev()).to(torch.bfloat16)
    gy = torch.randn(n, h, w, cout, generator=g).to(dev()).to(torch.bfloat16)
    data.append((x, gy, torch.zeros(3, 3, cin, cout, device=dev()), torch.zeros(3, 3, cin, cout, device=dev())))
  for x, gy, now, _ in data:
    ops.conv_bwd_weight_raw(x, gy, spec, out=now)
  ops.defer_slab_reductions(True)
  try:
    for x, gy, _, later in data:
      ops.conv_bwd_weight_raw(x, gy, spec, out=later)
    torch.cuda.synchronize()
    queued = [float(later.abs().max()) for _, _, _, later in data]
    n_flushed = ops.flush_slab_reductions()
  finally:
    ops.defer_slab_reductions(False)
  torch.cuda.synchronize()
  assert n_flushed >= 1 and ops.flush_slab_reductions() == 0
  assert sum(1 for q in queued if q == 0.0) == n_flushed      # the queued sinks were untouched before the flush
  for (x, gy, now, later), q in zip(data, queued):
    assert torch.equal(now, later), (tuple(x.shape), float((now - later).abs().max()))
  # two jobs into one sink, and more jobs than the table holds
  x, gy, now, later = data[[i for i, q in enumerate(queued) if q == 0.0][0]]      # a layer whose reduction is a slab job
  ops.conv_bwd_weight_raw(x, gy, spec, out=now)
  many = [torch.zeros_like(now) for _ in range(130)]
  ref = torch.zeros_like(now)
  ops.conv_bwd_weight_raw(x, gy, spec, out=ref)
  ops.defer_slab_reductions(True)
  try:
    ops.conv_bwd_weight_raw(x, gy, spec, out=later)
    for m in many:
      ops.conv_bwd_weight_raw(x, gy, spec, out=m)
    n2 = ops.flush_slab_reductions()
  finally:
    ops.defer_slab_reductions(False)
  torch.cuda.synchronize()
  assert n2 == 120
  assert rel_l2(host(later), host(now)) < 1e-6
  for m in many:
    assert torch.equal(m, ref)


# ---------------------------------------------------------------------------------------------- grouped convs
GROUPED_CASES = [
    # n (both groups), hw, cin, cout, k, padding        -- what the two discriminators run from 32 x 32 down
    (4, 32, 16, 32, 3, 'SAME'),      # conv_tile
    (4, 16, 32, 32, 3, 'SAME'),      # conv_tile
    (4, 8, 32, 32, 3, 'SAME'),       # conv_img
    (6, 4, 24, 32, 3, 'SAME'),       # conv_small (the minibatch-stddev layer's padded channel count is no multiple of 16)
    (4, 4, 32, 32, 4, 'VALID'),      # the dense layer
]


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize('case', range(len(GROUPED_CASES)))
def test_grouped_conv_equals_one_call_per_weight_set(ops, dtype, case):
  """TgConvDesc.groups = 2 (a stacked [2, kh, kw, cin, cout] kernel: the layers of discriminator_s and discriminator_t,
  twingan.py:105-110, as ONE call over the batch [D_s rows; D_t rows]): every conv entry point the discriminators' layers
  reach gives each image range exactly what the single-set call with its own weights gives it -- bit for bit in the
  forward and backward-data forms (per-image arithmetic), to fp32 summation order in the filter / bias gradients."""
  import twingan_amd.ops as O
  n, hw, cin, cout, k, padding = GROUPED_CASES[case]
  g = torch.Generator().manual_seed(500 + case)
  spec = O.ConvSpec(k, padding)
  ho = hw if padding == 'SAME' else hw - k + 1
  h = n // 2
  x = torch.randn(n, hw, hw, cin, generator=g).to(dtype).to(dev())
  w2 = (torch.randn(2, k, k, cin, cout, generator=g) * (2.0 / (k * k * cin)) ** 0.5).to(dev())
  b2 = (torch.randn(2, cout, generator=g) * 0.1).to(dev())
  gy = torch.randn(n, ho, ho, cout, generator=g).to(dtype).to(dev())
  epi = O.TG_EPI_BIAS | O.TG_EPI_LRELU

  def per_set(fn):
    return [fn(i, slice(i * h, (i + 1) * h)) for i in range(2)]

  def same(got, parts):
    want = torch.cat(parts)
    assert got.shape == want.shape and torch.equal(got, want), float((got.float() - want.float()).abs().max())

  # forward, bias + LeakyReLU epilogue
  y = O.conv_fwd_raw(x, w2, b2, spec, epi)
  if dtype != torch.float32:      # the MFMA kernels of these shapes pick the weight set per image: ONE launch
    from twingan_amd import _lib
    sym = _lib.load().tg_last_kernel().decode()
    assert sym.startswith(('conv_tile_kernel', 'conv_img_kernel', 'conv_small_kernel')[min(case, 3) - (1 if case > 0 else 0)]) and \
        sym.endswith(',sets>'), sym
  same(y, per_set(lambda i, r: O.conv_fwd_raw(x[r].contiguous(), w2[i], b2[i], spec, epi)))
  # backward-data, plain and with the producer's LeakyReLU mask
  same(O.conv_bwd_data_raw(gy, w2, tuple(x.shape), spec),
       per_set(lambda i, r: O.conv_bwd_data_raw(gy[r].contiguous(), w2[i], (h,) + tuple(x.shape[1:]), spec)))
  same(O.conv_bwd_data_masked_raw(gy, w2, x, spec),
       per_set(lambda i, r: O.conv_bwd_data_masked_raw(gy[r].contiguous(), w2[i], x[r].contiguous(), spec)))
  # forward with the mask epilogue (the gradient penalty's second backward)
  same(O.conv_fwd_masked_raw(x, w2, y, spec),
       per_set(lambda i, r: O.conv_fwd_masked_raw(x[r].contiguous(), w2[i], y[r].contiguous(), spec)))
  if padding == 'SAME' and dtype != torch.float32 and hw >= 16:
    # block ends: pooled output (+ sign bytes), and the backward-data that unpools
    z, zp = O.conv_fwd_pool_raw(x, w2, b2, spec, epi)
    ref = per_set(lambda i, r: O.conv_fwd_pool_raw(x[r].contiguous(), w2[i], b2[i], spec, epi))
    same(z, [p[0] for p in ref])
    same(zp, [p[1] for p in ref])
    assert O.conv_fwd_pool_signs_supported(x, w2, spec, epi)
    sg, zp2 = O.conv_fwd_pool_signs_raw(x, w2, b2, spec, epi)
    ref = per_set(lambda i, r: O.conv_fwd_pool_signs_raw(x[r].contiguous(), w2[i], b2[i], spec, epi))
    same(sg, [p[0] for p in ref])
    same(zp2, [p[1] for p in ref])
    gzp = torch.randn(n, ho // 2, ho // 2, cout, generator=g).to(dtype).to(dev())
    out = O.conv_bwd_data_unpool_raw(gzp, sg, w2, x, tuple(x.shape), spec, True)
    assert out is not None
    ref = per_set(lambda i, r: O.conv_bwd_data_unpool_raw(gzp[r].contiguous(), sg[r].contiguous(), w2[i], x[r].contiguous(),
                                                          (h,) + tuple(x.shape[1:]), spec, True))
    same(out[0], [p[0] for p in ref])
    same(out[1], [p[1] for p in ref])
  # filter (+ bias) gradients: into zeroed stacked sinks
  tol = 1e-6 if dtype == torch.float32 else 2e-5
  gw = O.conv_bwd_weight_raw(x, gy, spec, groups=2)
  ref = torch.stack(per_set(lambda i, r: O.conv_bwd_weight_raw(x[r].contiguous(), gy[r].contiguous(), spec)))
  assert gw.shape == ref.shape and rel_l2(host(gw), host(ref)) < tol
  if dtype != torch.float32:
    sink, bsink = torch.zeros_like(w2), torch.zeros_like(b2)
    O.conv_bwd_weight_raw(x, gy, spec, out=sink, gbias=bsink)
    assert rel_l2(host(sink), host(ref)) < tol
    assert rel_l2(host(bsink), host(gy.float().reshape(2, -1, cout).sum(1))) < 1e-3
    if O.conv_bwd_weight2_raw(x, gy, x[:n].contiguous(), gy[:n].contiguous(), spec, sink, bsink, 3):      # two segments, both grouped
      assert rel_l2(host(sink), 3.0 * host(ref)) < tol


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
def test_latent_layer_as_a_gemm_equals_the_padded_valid_conv(ops, dtype, monkeypatch):
  """ops.latent_conv: the plain PGGAN generator's first layer (nets/pggan.py:135-153, a 4x4 VALID conv over the latent noise
  zero-padded to 7x7) as [B, C] @ [C, 16 C'] of the flipped kernel -- output, kernel gradient and noise gradient against the
  float64 oracle's conv over the padded tensor, and against the conv kernel it replaces (which the 16-bit MFMA dispatch does
  not take: under TG_STRICT_DISPATCH=1 that fallback is an error, not a 100x slower launch)."""
  import twingan_amd.ops as O
  from twingan_amd import _lib
  g = torch.Generator().manual_seed(77)
  b, c, co, k = 6, 32, 24, 4
  rnd = bf16_round if dtype == torch.bfloat16 else f16_round
  noise = torch.randn(b, 1, 1, c, generator=g)
  w = torch.randn(k, k, c, co, generator=g) * (2.0 / (k * k * c)) ** 0.5
  gy = torch.randn(b, k, k, co, generator=g)
  nd = noise.to(dtype).to(dev()).requires_grad_(True)
  wd = w.to(dev()).requires_grad_(True)
  y = O.latent_conv(nd, wd)
  assert y.shape == (b, k, k, co) and y.dtype == dtype
  y.backward(gy.to(dtype).to(dev()))
  # oracle: the VALID conv over the zero-padded noise, operands as stored
  xpad = np.zeros((b, 2 * k - 1, 2 * k - 1, c))
  xpad[:, k - 1, k - 1, :] = rnd(host(noise))[:, 0, 0, :]
  want = N.conv2d(xpad, host(w), 'VALID')
  assert rel_l2(host(y), want) < (1e-2 if dtype == torch.bfloat16 else 2e-3)
  gyr = rnd(host(gy))
  want_gw = N.conv2d_bwd_weight(xpad, gyr, (k, k), 'VALID')
  assert rel_l2(host(wd.grad), want_gw) < 1e-5      # fp32 products of the stored operands, fp32 sums
  want_gx = N.conv2d_bwd_data(gyr, host(w), (2 * k - 1, 2 * k - 1), 'VALID')[:, k - 1, k - 1, :]
  assert rel_l2(host(nd.grad).reshape(b, c), want_gx) < (1e-2 if dtype == torch.bfloat16 else 2e-3)
  # the conv it replaces: same numbers from the direct kernel -- with a warning, and an error in strict mode
  xp = torch.nn.functional.pad(noise.to(dtype).to(dev()), (0, 0, k - 1, k - 1, k - 1, k - 1)).contiguous()
  O._SLOW_SEEN.clear()
  c2, co2 = 64, 64      # above the 1 MFLOP threshold
  xp2 = torch.zeros(b, 7, 7, c2, dtype=dtype, device=dev())
  w2 = torch.zeros(4, 4, c2, co2, device=dev())
  with pytest.warns(UserWarning, match='conv_\\*_direct'):
    O.conv2d(xp2, w2, None, 4, 'VALID')
  monkeypatch.setenv('TG_STRICT_DISPATCH', '1')
  with pytest.raises(_lib.TgError, match='TG_STRICT_DISPATCH'):
    O.conv2d(xp2, w2, None, 4, 'VALID')
  monkeypatch.delenv('TG_STRICT_DISPATCH')
  ref = O.conv2d(xp, wd.detach(), None, 4, 'VALID')
  assert rel_l2(host(y), host(ref)) < (1e-2 if dtype == torch.bfloat16 else 2e-3)


# ---------------------------------------------------------------------------------------------- conv dispatch across its batch thresholds
# Which conv kernel a call lands on depends on the BATCH, not only on the layer ("Dispatch thresholds"): conv_small
# takes n * hout * wout <= 4096 pixels (and its packs are fragment-ordered, the first-generation kernel's are not), the tile
# family changes its output block (blocks >= 1024), its sub-tiles per wave (tiles >= 1024) and the kernel itself (tiles >=
# 2048 with 16 / 32 input channels: weight-resident / thin-output kernels).  The pairs below sit one batch on each side of
# one such flip.  They are DATA: the tests do not recompute the dispatch arithmetic, they assert with tg_last_kernel() that
# the two sides ran different kernels, and tests/golden/dispatch_edge_kernels.json pins every symbol
# (TG_RECORD_EDGE_KERNELS=<path> re-records into <path>).
import ctypes    # noqa: E402
import json      # noqa: E402
import os        # noqa: E402

EDGE_KERNELS_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'dispatch_edge_kernels.json')
# the bounds of tests/test_gpu_bench_shapes.py: 16-bit outputs vs the float64 oracle / vs the direct kernel, fp32 outputs
EDGE_TOL = {torch.bfloat16: (4e-3, 2e-3), torch.float16: (6e-4, 4e-4)}
EDGE_F32_TOL = 1e-4
EDGE_DTYPES = {'bf16': torch.bfloat16, 'f16': torch.float16}

EDGE_CASES = [
    # id, k, padding, hw, cin, cout, n below, n above, entry points whose kernel must differ between the two
    # conv_small <-> first-generation kernel, and with it the element order of the pack (4096 pixels)
    ('small_k1_hw8', 1, 'SAME', 8, 32, 32, 64, 65, ('fwd', 'fwd_masked', 'bwd_data', 'bwd_data_masked')),
    ('small_k3_hw4', 3, 'SAME', 4, 32, 32, 256, 257, ('fwd', 'fwd_masked', 'fwd_stats', 'bwd_data', 'bwd_data_masked')),
    ('small_k3_hw8_c24', 3, 'SAME', 8, 24, 40, 64, 65, ('fwd', 'fwd_masked', 'bwd_data', 'bwd_data_masked')),      # conv_img refuses cin 24
    # the dense 4x4 VALID layer is rewritten as a 1x1 conv over 16 cin channels of a 1x1 map: n pixels in BOTH directions
    ('dense', 4, 'VALID', 4, 8, 8, 4096, 4097, ('fwd', 'fwd_masked', 'bwd_data', 'bwd_data_masked')),
    # tile family: 32- <-> 64-channel output blocks (1024 blocks, cout > 32)
    ('tile_bn', 3, 'SAME', 128, 48, 64, 7, 8, ('fwd', 'fwd_masked', 'fwd_stats', 'fwd_pool', 'bwd_data')),
    # one <-> two sub-tiles per wave (1024 tiles, h % 16 == 0, cin_pad >= 64)
    ('tile_mt', 3, 'SAME', 128, 64, 32, 7, 8, ('fwd', 'fwd_masked', 'fwd_stats', 'fwd_pool')),
    # conv_tile_kernel <-> conv_tile_wres_kernel / conv_thin16_kernel (2048 tiles, cin_pad 16 / 32)
    ('tile_wres16', 3, 'SAME', 128, 16, 32, 15, 16, ('fwd', 'fwd_masked', 'fwd_stats', 'fwd_pool', 'bwd_data', 'bwd_data_masked')),
    ('tile_wres32', 3, 'SAME', 128, 32, 32, 15, 16, ('fwd', 'fwd_masked', 'fwd_stats', 'fwd_pool', 'bwd_data', 'bwd_data_masked')),
    ('tile_thin16', 3, 'SAME', 128, 16, 16, 15, 16, ('fwd', 'fwd_masked', 'fwd_stats', 'bwd_data', 'bwd_data_masked')),
    ('tile_k1_wres', 1, 'SAME', 128, 32, 32, 15, 16, ('fwd', 'fwd_masked', 'bwd_data', 'bwd_data_masked')),
]


def _last_kernel():
  from twingan_amd import _lib
  return _lib.load().tg_last_kernel().decode()


class _Direct:
  """Forces the direct (one thread per output) algorithm inside the block."""

  def __enter__(self):
    import twingan_amd.ops as O
    self.O, self.saved = O, O._mfma_ok
    O._mfma_ok = lambda *a: False

  def __exit__(self, *a):
    self.O._mfma_ok = self.saved


def _edge_operands(seed, n, k, hin, ho, cin, cout, dtype, groups=1):
  """16-bit activations, an fp32 master kernel holding 16-bit values (its pack is then exact), a bias."""
  g = torch.Generator().manual_seed(seed)
  x = torch.randn(n, hin, hin, cin, generator=g).to(dtype).to(dev())
  gy = torch.randn(n, ho, ho, cout, generator=g).to(dtype).to(dev())
  lead = (groups,) if groups > 1 else ()
  w = (torch.randn(lead + (k, k, cin, cout), generator=g) / (k * k * cin) ** 0.5).to(dtype).float().to(dev()).contiguous()
  b = (torch.randn(lead + (cout,), generator=g) * 0.1).to(dev())
  return x, gy, w, b


def _edge_wgrad_oracle(x, gy, k, pad):
  """oracle/np_ops.py conv2d_bwd_weight; its one-BLAS-product-per-tap form (the same float64 sums, held to it by
  tests/test_oracle.py) where the einsum form would take minutes."""
  if x.size * gy.shape[3] * k * k <= 1 << 28:
    return N.conv2d_bwd_weight(x, gy, (k, k), pad)
  return N.conv2d_bwd_weight_gemm(x, gy, (k, k), pad)


def _edge_partials(st, y, what):
  """sum over chunks of the conv's statistics partials == (sum y, sum y^2) per image and channel of the tensor it wrote."""
  n, h, w, c = y.shape
  part = st.part.view(n, st.chunks, 2, c).double().sum(dim=1)
  yd = y.double().view(n, h * w, c)
  s1, s2 = yd.sum(dim=1), (yd * yd).sum(dim=1)
  e1 = float(((part[:, 0] - s1).abs() / (s2 * h * w).sqrt().clamp_min(1e-30)).max())
  e2 = float((part[:, 1] / s2.clamp_min(1e-30) - 1).abs().max())
  assert e1 < 2e-6 and e2 < 2e-6, ('statistics partials', what, e1, e2)


def _edge_symbols_check(case_id, dname, rec):
  """rec {entry point: {n: kernel symbol}} of one (case, dtype) against the recorded table (or into it)."""
  dst = os.environ.get('TG_RECORD_EDGE_KERNELS')
  if dst:
    table = {}
    if os.path.exists(dst):
      with open(dst) as fh:
        table = json.load(fh)
    table.setdefault(case_id, {})[dname] = rec
    with open(dst, 'w') as fh:
      json.dump(table, fh, indent=1, sort_keys=True)
    return
  assert os.path.exists(EDGE_KERNELS_PATH), 'record with TG_RECORD_EDGE_KERNELS=tests/golden/dispatch_edge_kernels.json'
  with open(EDGE_KERNELS_PATH) as fh:
    want = json.load(fh).get(case_id, {}).get(dname)
  assert want == rec, ('dispatch moved', case_id, dname, rec, want)


def _edge_straddles(cid, rec, flips, n_lo, n_hi):
  for ep in flips:
    lo, hi = rec[ep][str(n_lo)], rec[ep][str(n_hi)]
    assert lo != hi, '%s %s: n = %d and n = %d no longer straddle a dispatch threshold, both ran %s' % (cid, ep, n_lo, n_hi, lo)


def _edge_single(O, spec, pad, x, gy, w, b, dtype, rec, what):
  """Every conv entry point on one batch: first and last image against the float64 oracle on the same rounded operands, the
  whole tensor against the direct kernel, fp32 gradients against the oracle over the whole batch."""
  from twingan_amd._lib import TG_EPI_BIAS, TG_EPI_LRELU
  otol, dtol = EDGE_TOL[dtype]
  rnd = bf16_round if dtype == torch.bfloat16 else f16_round
  n, hin, _, cin = x.shape
  ho, cout, k = gy.shape[1], gy.shape[3], spec.kh
  sel = sorted({0, n - 1})
  wn, bn, xs, gs = host(w), host(b), host(x[sel]), host(gy[sel])
  epi = TG_EPI_BIAS | TG_EPI_LRELU
  # element-wise (tests/elementwise.py): first, last and one seeded middle image against the oracle, whole batch against the
  # direct kernel on the device.  sel3 holds sel's images at positions pos.
  sel3 = _with_middle(sel, '%s:%d' % (what, n), 0, n)
  pos = [sel3.index(i) for i in sel]
  dn = _ew_dname(dtype)
  KF, KB = k * k * cin, k * k * cout
  x3, g3 = host(x[sel3]), host(gy[sel3])
  fmag = lambda i0, i1: E.conv_mag_device(x[i0:i1], w, pad)
  bmag = lambda i0, i1: E.conv_mag_device(gy[i0:i1], w, pad, transpose=True)

  def each(got, ref, bound, name):
    _ew_note('conv edge ' + name, dn, E.assert_elementwise(got, ref, bound, '%s n%d %s images %s' % (what, n, name, sel3)))

  def pair(a, bb, mag, K, name, roundings=2):
    _ew_note('conv edge ' + name, dn, E.assert_pair_device(a, bb, mag, K, '%s n%d %s' % (what, n, name), roundings=roundings))

  def note(ep):
    rec.setdefault(ep, {})[str(n)] = _last_kernel()

  def close(got, ref, tol, name):
    e = rel_l2(got, ref)
    print('[edge %s n%d] %s %.3e (bound %.1e)' % (what, n, name, e, tol))
    assert e < tol, (what, n, name, e, tol)

  # ---- forward: plain, bias + LeakyReLU, with the mask epilogue, with the statistics epilogue
  lin3, lmag3 = N.conv2d_gemm(x3, wn, pad), N.conv2d_gemm(np.abs(x3), np.abs(wn), pad)
  lin = lin3[pos]
  y0 = O.conv_fwd_raw(x, w, None, spec, 0)
  note('fwd')
  close(host(y0[sel]), lin, otol, 'fwd')
  each(host(y0[sel3]), lin3, E.conv_bound(lin3, lmag3, KF, dtype), 'fwd')
  with _Direct():
    yd = O.conv_fwd_raw(x, w, None, spec, 0)
  close(host(y0), host(yd), dtol, 'fwd vs direct')      # linear part: LeakyReLU would amplify a 1-ulp flip across zero
  pair(y0, yd, fmag, KF, 'fwd vs direct')
  y1 = O.conv_fwd_raw(x, w, b, spec, epi)
  close(host(y1[sel]), N.leaky_relu(lin + bn), otol, 'fwd bias lrelu')
  # bias add and slope multiply: two more fp32 operations (K + 2, |bias| joins the magnitudes); LeakyReLU is 1-Lipschitz
  act3 = N.leaky_relu(lin3 + bn)
  act_bound = E.conv_bound(act3, lmag3 + np.abs(bn), KF + 2, dtype)
  each(host(y1[sel3]), act3, act_bound, 'fwd bias lrelu')
  ym = O.conv_fwd_masked_raw(x, w, gy, spec)             # gy has the output's shape: any tensor serves as the mask source
  note('fwd_masked')
  close(host(ym[sel]), lin * np.where(gs > 0, 1.0, 0.2), otol, 'fwd_masked')
  slope3 = np.where(g3 > 0, 1.0, 0.2)                    # from an input: exact
  # where the mask is not fusable (capi.hip: "the plain conv, then the mask in place") the stored value is masked and stored
  # again: a second rounding, u |ref|, of the elements whose slope is not 1
  twice = lambda ref, slope: _twice(ref, slope, dtype)
  each(host(ym[sel3]), lin3 * slope3, E.conv_bound(lin3 * slope3, lmag3 * slope3, KF + 1, dtype, twice(lin3 * slope3, slope3)),
       'fwd_masked')
  with _Direct():
    ymd = O.conv_fwd_masked_raw(x, w, gy, spec)
  close(host(ym), host(ymd), 2 * dtol, 'fwd_masked vs direct')      # the direct path rounds once more before the mask
  pair(ym, ymd, fmag, KF + 1, 'fwd_masked vs direct', roundings=4)      # two storage roundings on either side at most
  if k == 3:
    ys, st = O.conv_fwd_stats_raw(x, w, spec)
    note('fwd_stats')
    close(host(ys[sel]), lin, otol, 'fwd_stats')
    each(host(ys[sel3]), lin3, E.conv_bound(lin3, lmag3, KF, dtype), 'fwd_stats')
    close(host(ys), host(yd), dtol, 'fwd_stats vs direct')
    pair(ys, yd, fmag, KF, 'fwd_stats vs direct')
    if st is not None:
      _edge_partials(st, ys, what)
    del ys
  del ym, ymd

  # ---- block ends (3x3 SAME shapes of the tile kernels): pooled output, sign bytes, the backward-data that unpools
  if k == 3 and pad == 'SAME' and hin >= 16:
    z, zp = O.conv_fwd_pool_raw(x, w, b, spec, epi)
    note('fwd_pool')
    close(host(z[sel]), N.leaky_relu(lin + bn), otol, 'fwd_pool z')
    each(host(z[sel3]), act3, act_bound, 'fwd_pool z')
    close(host(z), host(y1), dtol, 'fwd_pool z vs plain forward')
    close(host(zp), host(z.float().view(n, ho // 2, 2, ho // 2, 2, cout).mean(dim=(2, 4))), dtol, 'fwd_pool pooled')
    # the pooled tensor: the mean of four STORED z (each within its own bound), rounded once more
    pool4 = lambda a: a.reshape(len(sel3), ho // 2, 2, ho // 2, 2, cout).mean(axis=(2, 4))
    u_st = E.unit_roundoff(dtype)
    each(host(zp[sel3]), pool4(act3), u_st * np.abs(pool4(act3)) + (1 + u_st) * pool4(act_bound) + E.tiny(dtype), 'fwd_pool pooled')
    assert O.conv_fwd_pool_signs_supported(x, w, spec, epi), ('no sign-bit variant', what, n)
    sg, zp2 = O.conv_fwd_pool_signs_raw(x, w, b, spec, epi)
    note('fwd_pool_signs')
    assert torch.equal(zp2, zp), ('fwd_pool_signs pooled', what, n)
    bits = (z > 0).view(n, ho, ho, cout // 8, 8).to(torch.int32)
    want_bytes = (bits << torch.arange(8, device=z.device, dtype=torch.int32)).sum(dim=-1).to(torch.uint8)
    assert torch.equal(sg, want_bytes), ('fwd_pool_signs bits', what, n, int((sg != want_bytes).sum()))
    if cout % 32 == 0:      # the unpooling kernels stage 32-channel chunks of the incoming gradient
      gzp = gy[:, ::2, ::2, :].contiguous()
      out = O.conv_bwd_data_unpool_raw(gzp, sg, w, x, tuple(x.shape), spec, True)
      assert out is not None, ('unpool refused', what, n)
      note('bwd_data_unpool')
      g2, _ = O.lrelu_pool_bwd_signs(gzp, sg, spec.alpha, None, False)
      assert torch.equal(out[1], g2), ('unpool kept gradient', what, n)
      two = O.conv_bwd_data_masked_raw(g2, w, x, spec)
      close(host(out[0]), host(two), dtol, 'unpool vs two launches')
      pair(out[0], two, lambda i0, i1: E.conv_mag_device(g2[i0:i1], w, pad, transpose=True), KB + 1, 'unpool vs two launches',
           roundings=4)
      # the oracle on sel3: the unpooled gradient is an MFMA operand, so it IS rounded to the storage type (rnd(up), which the
      # kept tensor equals bit for bit, asserted above); then backward-data (K = k k cout) and the producer's mask (+ 1)
      up3 = rnd(host(gzp[sel3]).repeat(2, axis=1).repeat(2, axis=2) * 0.25 * np.where(host(z[sel3]) > 0, 1.0, 0.2))
      xsl = np.where(x3 > 0, 1.0, 0.2)
      ref3u = N.conv2d_bwd_data_gemm(up3, wn, (hin, hin), pad) * xsl
      mag3u = N.conv2d_bwd_data_gemm(np.abs(up3), np.abs(wn), (hin, hin), pad) * xsl
      close(host(out[0][sel]), ref3u[pos], otol, 'unpool')
      each(host(out[0][sel3]), ref3u, E.conv_bound(ref3u, mag3u, KB + 1, dtype, twice(ref3u, xsl)), 'unpool')
      del out, g2, two
    del z, zp, sg, zp2
  del y0, y1, yd

  # ---- backward-data, plain and with the producer's LeakyReLU mask in the epilogue
  ref3 = N.conv2d_bwd_data_gemm(g3, wn, (hin, hin), pad)
  rmag3 = N.conv2d_bwd_data_gemm(np.abs(g3), np.abs(wn), (hin, hin), pad)
  ref = ref3[pos]
  gx = O.conv_bwd_data_raw(gy, w, tuple(x.shape), spec)
  note('bwd_data')
  close(host(gx[sel]), ref, otol, 'bwd_data')
  each(host(gx[sel3]), ref3, E.conv_bound(ref3, rmag3, KB, dtype), 'bwd_data')
  with _Direct():
    gd = O.conv_bwd_data_raw(gy, w, tuple(x.shape), spec)
  close(host(gx), host(gd), dtol, 'bwd_data vs direct')
  pair(gx, gd, bmag, KB, 'bwd_data vs direct')
  gm = O.conv_bwd_data_masked_raw(gy, w, x, spec)
  note('bwd_data_masked')
  close(host(gm[sel]), ref * np.where(xs > 0, 1.0, 0.2), otol, 'bwd_data_masked')
  xslope3 = np.where(x3 > 0, 1.0, 0.2)
  each(host(gm[sel3]), ref3 * xslope3, E.conv_bound(ref3 * xslope3, rmag3 * xslope3, KB + 1, dtype, twice(ref3 * xslope3, xslope3)),
       'bwd_data_masked')
  gdm = O.lrelu_bwd_raw(gd, x, 0.2)
  close(host(gm), host(gdm), 2 * dtol, 'bwd_data_masked vs direct')      # two roundings apart
  pair(gm, gdm, bmag, KB + 1, 'bwd_data_masked vs direct', roundings=4)
  del gdm
  del gx, gd, gm

  # ---- filter gradient (fp32), alone and with the bias gradient riding along
  want_gw = _edge_wgrad_oracle(host(x), host(gy), k, pad)
  gw = O.conv_bwd_weight_raw(x, gy, spec)
  note('bwd_weight')
  close(host(gw), want_gw, EDGE_F32_TOL, 'bwd_weight')
  gw_alone = gw
  gb = torch.zeros(cout, dtype=torch.float32, device=x.device)
  gw = O.conv_bwd_weight_raw(x, gy, spec, gbias=gb)
  note('bwd_weight_bias')
  close(host(gw), want_gw, EDGE_F32_TOL, 'bwd_weight_bias')
  close(host(gb), host(gy).sum(axis=(0, 1, 2)), EDGE_F32_TOL, 'bwd_weight_bias bias')
  # fp32 sums over P = n ho wo pixels, any order: both launches' filter gradients, and the bias gradient
  P = n * ho * ho
  wbound = E.wgrad_bound(want_gw, _edge_wgrad_oracle(np.abs(host(x)), np.abs(host(gy)), k, pad), P)
  r = E.assert_elementwise(host(gw), want_gw, wbound, '%s n%d bwd_weight_bias' % (what, n))
  r = max(r, E.assert_elementwise(host(gw_alone), want_gw, wbound, '%s n%d bwd_weight' % (what, n)))
  gsum = host(gy).sum(axis=(0, 1, 2))
  r = max(r, E.assert_elementwise(host(gb), gsum, E.wgrad_bound(gsum, np.abs(host(gy)).sum(axis=(0, 1, 2)), P),
                                  '%s n%d bias gradient' % (what, n)))
  _ew_note('conv edge bwd_weight', dn, r)


@pytest.mark.parametrize('dname', sorted(EDGE_DTYPES))
@pytest.mark.parametrize('case', EDGE_CASES, ids=[c[0] for c in EDGE_CASES])
def test_conv_entry_points_on_both_sides_of_a_dispatch_threshold(ops, case, dname):
  """One layer at two batches that straddle one batch threshold of the conv dispatch: every entry point is right on both
  sides (oracle, direct kernel), the two sides DID run different kernels (a pair that no longer straddles its threshold
  fails here and says so), and every symbol is the recorded one."""
  import twingan_amd.ops as O
  cid, k, pad, hw, cin, cout, n_lo, n_hi, flips = case
  dtype = EDGE_DTYPES[dname]
  spec = O.ConvSpec(k, pad)
  ho = hw if pad == 'SAME' else hw - k + 1
  x, gy, w, b = _edge_operands(900 + EDGE_CASES.index(case), n_hi, k, hw, ho, cin, cout, dtype)
  rec = {}
  for n in (n_lo, n_hi):
    _edge_single(O, spec, pad, x[:n], gy[:n], w, b, dtype, rec, cid)
  _edge_straddles(cid, rec, flips, n_lo, n_hi)
  _edge_symbols_check(cid, dname, rec)


UPCAT_EDGE_CASES = [
    # id, hw (output), c0, c1, cout, n below, n above, entry points whose kernel must differ
    ('upcat_32_32_mt_wres', 64, 32, 32, 32, 31, 32, ('upcat_fwd', 'upcat_bwd_data')),      # forward: sub-tiles; backward: weight-resident
    ('upcat_64_64_bn', 64, 64, 64, 64, 15, 16, ('upcat_bwd_data',)),                        # backward: 64-channel blocks
    ('upcat_64_64_mt', 64, 64, 64, 64, 31, 32, ('upcat_fwd',)),
    ('upcat_32_32_thin16', 128, 32, 32, 16, 15, 16, ('upcat_fwd',)),                        # forward: thin-output kernel
    ('upcat_32_32_upboth', 128, 32, 32, 16, 7, 8, ('upcat_fwd', 'upcat_bwd_data')),         # backward: both halves in one block
    ('upcat_64_64_wres', 128, 64, 64, 32, 7, 8, ('upcat_fwd', 'upcat_bwd_data')),
]


@pytest.mark.parametrize('dname', sorted(EDGE_DTYPES))
@pytest.mark.parametrize('case', UPCAT_EDGE_CASES, ids=[c[0] for c in UPCAT_EDGE_CASES])
def test_upcat_conv_on_both_sides_of_a_dispatch_threshold(ops, case, dname):
  """conv3x3(concat(up2(x0), skip)) read from its two sources, its backward-data with the concat adjoint in the epilogue and
  its filter gradient, at two batches that straddle a threshold of dispatch_tile_upcat / dispatch_tile_upbwd."""
  import twingan_amd.ops as O
  cid, hw, c0, c1, cout, n_lo, n_hi, flips = case
  dtype = EDGE_DTYPES[dname]
  otol, dtol = EDGE_TOL[dtype]
  spec = O.ConvSpec(3, 'SAME')
  g = torch.Generator().manual_seed(950 + UPCAT_EDGE_CASES.index(case))
  x0a = torch.randn(n_hi, hw // 2, hw // 2, c0, generator=g).to(dtype).to(dev())
  x1a = torch.randn(n_hi, hw, hw, c1, generator=g).to(dtype).to(dev())
  gya = torch.randn(n_hi, hw, hw, cout, generator=g).to(dtype).to(dev())
  w = (torch.randn(3, 3, c0 + c1, cout, generator=g) / (9 * (c0 + c1)) ** 0.5).to(dtype).float().to(dev()).contiguous()
  wn = host(w)
  rec = {}

  def close(got, ref, tol, name, n):
    e = rel_l2(got, ref)
    print('[edge %s n%d] %s %.3e (bound %.1e)' % (cid, n, name, e, tol))
    assert e < tol, (cid, n, name, e, tol)

  def cat_of(i):      # the materialised input of image i
    return np.concatenate([host(x0a[i:i + 1]).repeat(2, axis=1).repeat(2, axis=2), host(x1a[i:i + 1])], axis=3)

  for n in (n_lo, n_hi):
    x0, x1, gy = x0a[:n].contiguous(), x1a[:n].contiguous(), gya[:n].contiguous()
    assert O.upcat_conv_supported(x0, x1, w)
    sel = sorted({0, n - 1})
    # element-wise: first, last and one seeded middle image against the oracle, the whole batch against the direct kernel
    sel3 = _with_middle(sel, '%s:%d' % (cid, n), 0, n)
    pos = [sel3.index(i) for i in sel]
    KF, KB, u_st = 9 * (c0 + c1), 9 * cout, E.unit_roundoff(dtype)
    cat3 = np.concatenate([cat_of(i) for i in sel3])
    lin3, lmag3 = N.conv2d_gemm(cat3, wn), N.conv2d_gemm(np.abs(cat3), np.abs(wn))
    fbound = E.conv_bound(lin3, lmag3, KF, dtype)

    def each(got, ref, bound, name):
      _ew_note('upcat edge ' + name, dname, E.assert_elementwise(got, ref, bound, '%s n%d %s images %s' % (cid, n, name, sel3)))

    def pair(a, b, mag, K, name, roundings=2, extra=None):
      _ew_note('upcat edge ' + name, dname, E.assert_pair_device(a, b, mag, K, '%s n%d %s' % (cid, n, name), roundings=roundings,
                                                                 extra=extra))
    y = O.upcat_conv(x0, x1, w, 0, ())
    rec.setdefault('upcat_fwd', {})[str(n)] = _last_kernel()
    close(host(y[sel]), lin3[pos], otol, 'upcat fwd', n)
    each(host(y[sel3]), lin3, fbound, 'fwd')
    xcat = O.upsample2x_concat(x0, x1, 0, ())
    fmag = lambda i0, i1: E.conv_mag_device(xcat[i0:i1], w, 'SAME')
    with _Direct():
      yd = O.conv_fwd_raw(xcat, w, None, spec, 0)
    close(host(y), host(yd), dtol, 'upcat fwd vs direct', n)
    pair(y, yd, fmag, KF, 'fwd vs direct')
    ys, st = O.upcat_conv_stats(x0, x1, w, 0, ())
    rec.setdefault('upcat_fwd_stats', {})[str(n)] = _last_kernel()
    close(host(ys), host(yd), dtol, 'upcat fwd_stats vs direct', n)
    each(host(ys[sel3]), lin3, fbound, 'fwd_stats')
    pair(ys, yd, fmag, KF, 'fwd_stats vs direct')
    if st is not None:
      _edge_partials(st, ys, cid)
    del y, ys, yd, xcat
    # backward-data: 2x2 sums of the first c0 channels into g0, the rest into g1
    d = O._desc((n, hw, hw, c0 + c1), cout, spec, dtype, 0)
    g0, g1 = torch.empty_like(x0), torch.empty_like(x1)
    wpack = O.PackCache.get(w, d, 1)      # held in a local: an uncached pack must outlive the launch
    O.call('tg_conv2d_upcat_bwd_data', gy.data_ptr(), wpack.data_ptr(), g0.data_ptr(), g1.data_ptr(), n, hw, hw, c0, c1, cout, 0,
           O._pack_perm(()), O._dt(gy), O._stream())
    rec.setdefault('upcat_bwd_data', {})[str(n)] = _last_kernel()
    gc3 = N.conv2d_bwd_data_gemm(host(gy[sel3]), wn, (hw, hw))
    gm3 = N.conv2d_bwd_data_gemm(np.abs(host(gy[sel3])), np.abs(wn), (hw, hw))
    gc = gc3[pos]
    close(host(g0[sel]), gc[..., :c0].reshape(len(sel), hw // 2, 2, hw // 2, 2, c0).sum(axis=(2, 4)), otol, 'upcat g0', n)
    close(host(g1[sel]), gc[..., c0:], otol, 'upcat g1', n)
    # the fused kernel sums the 2x2 block in its fp32 accumulators and rounds once: 4 x 9 cout summands for g0, 9 cout for g1
    quad = lambda a: a[..., :c0].reshape(len(sel3), hw // 2, 2, hw // 2, 2, c0).sum(axis=(2, 4))
    each(host(g0[sel3]), quad(gc3), E.conv_bound(quad(gc3), quad(gm3), 4 * KB, dtype), 'bwd_data g0')
    each(host(g1[sel3]), gc3[..., c0:], E.conv_bound(gc3[..., c0:], gm3[..., c0:], KB, dtype), 'bwd_data g1')
    with _Direct():
      gcat = O.conv_bwd_data_raw(gy, w, (n, hw, hw, c0 + c1), spec)
    r0, r1 = torch.empty_like(g0), torch.empty_like(g1)
    O.call('tg_upsample2x_concat_bwd', gcat.data_ptr(), r0.data_ptr(), r1.data_ptr(), n, hw // 2, hw // 2, c0, c1, 0,
           O._pack_perm(()), O._dt(gcat), O._stream())
    close(host(g0), host(r0), 2 * dtol, 'upcat g0 vs direct', n)      # the composed path rounds the concat-layout gradient first
    close(host(g1), host(r1), dtol, 'upcat g1 vs direct', n)
    # whole batch on the device.  g0: the composed route adds four STORED concat-layout values -- u sum4 |gcat| of its own
    qd = lambda t: t[..., :c0].reshape(t.shape[0], hw // 2, 2, hw // 2, 2, c0).sum(dim=(2, 4))
    bmag = lambda i0, i1: E.conv_mag_device(gy[i0:i1], w, 'SAME', transpose=True)
    pair(g0, r0, lambda i0, i1: qd(bmag(i0, i1)), 4 * KB, 'bwd_data g0 vs direct',
         extra=lambda i0, i1: (1 + u_st) * (u_st * qd(gcat[i0:i1].float().abs()) + 4 * E.tiny(dtype)))
    pair(g1, r1, lambda i0, i1: bmag(i0, i1)[..., c0:], KB, 'bwd_data g1 vs direct')
    del g0, g1, r0, r1, gcat
    # filter gradient
    wl = w.clone().requires_grad_(True)
    O.upcat_conv(x0, x1, wl, 0, ()).backward(gy)
    rec.setdefault('upcat_bwd_weight', {})[str(n)] = _last_kernel()
    want = sum(N.conv2d_bwd_weight_gemm(cat_of(i), host(gy[i:i + 1]), (3, 3)) for i in range(n))
    close(host(wl.grad), want, EDGE_F32_TOL, 'upcat bwd_weight', n)
    wmag = sum(N.conv2d_bwd_weight_gemm(np.abs(cat_of(i)), np.abs(host(gy[i:i + 1])), (3, 3)) for i in range(n))
    _ew_note('upcat edge bwd_weight', dname, E.assert_elementwise(host(wl.grad), want, E.wgrad_bound(want, wmag, n * hw * hw),
                                                                  '%s n%d upcat bwd_weight' % (cid, n)))
  _edge_straddles(cid, rec, flips, n_lo, n_hi)
  _edge_symbols_check(cid, dname, rec)


GROUPED_EDGE_CASES = [
    # id, G, k, padding, hw, cin, cout, n (all groups), forward taken whole, backward-data taken whole, PackCache.refresh check
    # whole batch and one group both under conv_small's limit: ONE launch that picks the weight set per image
    ('g2_k1_hw8_under', 2, 1, 'SAME', 8, 32, 32, 64, True, True, False),
    ('g3_k1_hw8_under', 3, 1, 'SAME', 8, 32, 32, 48, True, True, False),
    ('g2_k3_hw4_under', 2, 3, 'SAME', 4, 32, 32, 256, True, True, False),
    ('g3_k3_hw4_under', 3, 3, 'SAME', 4, 32, 32, 240, True, True, False),
    ('g2_dense_under', 2, 4, 'VALID', 4, 8, 8, 384, True, True, False),
    # whole batch over, one group under: one launch per group, each on conv_small
    ('g2_k1_hw8_n96', 2, 1, 'SAME', 8, 32, 32, 96, False, False, True),
    ('g3_k1_hw8_n96', 3, 1, 'SAME', 8, 32, 32, 96, False, False, False),
    ('g2_k3_hw4_n264', 2, 3, 'SAME', 4, 32, 32, 264, False, False, False),
    ('g2_k3_hw4_n384', 2, 3, 'SAME', 4, 32, 32, 384, False, False, True),      # the discriminators' 4x4 layer as a pair at batch 64
    ('g3_k3_hw4_n600', 3, 3, 'SAME', 4, 32, 32, 600, False, False, False),
    ('g2_mbstd_c264_n264', 2, 3, 'SAME', 4, 264, 256, 264, False, False, False),      # the minibatch-stddev layer
    ('g2_dense_n8192', 2, 4, 'VALID', 4, 8, 8, 8192, False, False, True),      # the dense layer: n pixels, forward and backward-data
    ('g3_dense_n6144', 3, 4, 'VALID', 4, 8, 8, 6144, False, False, False),
    # whole batch and one group both over: one launch per group on the first-generation kernel
    ('g2_k1_hw8_over', 2, 1, 'SAME', 8, 32, 32, 130, False, False, False),
    ('g3_k1_hw8_over', 3, 1, 'SAME', 8, 32, 32, 195, False, False, False),
    ('g2_k3_hw4_over', 2, 3, 'SAME', 4, 32, 32, 514, False, False, False),
    ('g2_dense_over', 2, 4, 'VALID', 4, 8, 8, 8194, False, False, False),
    # tile family: the whole batch reaches the weight-resident kernel's 2048 tiles, one group does not / does / neither
    ('g2_tile_under', 2, 3, 'SAME', 128, 16, 32, 8, True, True, False),
    ('g2_tile_n16', 2, 3, 'SAME', 128, 16, 32, 16, False, False, True),
    ('g3_tile_n24', 3, 3, 'SAME', 128, 16, 32, 24, False, False, False),
    ('g2_tile_over', 2, 3, 'SAME', 128, 16, 32, 32, False, False, False),
]


@pytest.mark.parametrize('dname', sorted(EDGE_DTYPES))
@pytest.mark.parametrize('case', GROUPED_EDGE_CASES, ids=[c[0] for c in GROUPED_EDGE_CASES])
def test_grouped_conv_across_the_dispatch_thresholds(ops, case, dname):
  """test_grouped_conv_equals_one_call_per_weight_set where the grouped call and its groups sit on different sides of a batch
  threshold: a grouped call no kernel takes whole is launched once per group on n / G images, and that launch may pick another
  kernel -- and read another pack layout -- than the whole batch would.  Every entry point equals one call per weight set (bit
  for bit in the forward / backward-data forms), the forward and the backward-data also match the float64 oracle on the first
  and last image of every group (so that "grouped == per set" cannot hold by both being wrong), and a registered stacked
  weight survives PackCache.refresh."""
  import twingan_amd.ops as O
  cid, G, k, pad, hw, cin, cout, n, fwd_whole, bwd_whole, refresh = case
  dtype = EDGE_DTYPES[dname]
  otol, _ = EDGE_TOL[dtype]
  spec = O.ConvSpec(k, pad)
  ho = hw if pad == 'SAME' else hw - k + 1
  h = n // G
  x, gy, w2, b2 = _edge_operands(980 + GROUPED_EDGE_CASES.index(case), n, k, hw, ho, cin, cout, dtype, G)
  epi = O.TG_EPI_BIAS | O.TG_EPI_LRELU
  rec = {}

  def per_set(fn):
    return [fn(i, slice(i * h, (i + 1) * h)) for i in range(G)]

  def same(got, parts, name):
    want = torch.cat(parts)
    assert got.shape == want.shape, (cid, name)
    assert torch.equal(got, want), (cid, name, float((got.float() - want.float()).abs().max()), float(want.float().abs().max()))

  def close(got, ref, tol, name):
    e = rel_l2(got, ref)
    print('[edge %s] %s %.3e (bound %.1e)' % (cid, name, e, tol))
    assert e < tol, (cid, name, e, tol)

  def whole(ep, sym, expected):
    rec[ep] = sym
    assert sym.endswith(',sets>') == expected, \
        '%s %s: expected %s, ran %s' % (cid, ep, 'one launch over all weight sets' if expected else 'one launch per group', sym)

  # ---- forward (bias + LeakyReLU) and the forward with the mask epilogue
  y = O.conv_fwd_raw(x, w2, b2, spec, epi)
  whole('fwd', _last_kernel(), fwd_whole)
  same(y, per_set(lambda i, r: O.conv_fwd_raw(x[r].contiguous(), w2[i], b2[i], spec, epi)), 'fwd')
  ym = O.conv_fwd_masked_raw(x, w2, y, spec)
  rec['fwd_masked'] = _last_kernel()
  same(ym, per_set(lambda i, r: O.conv_fwd_masked_raw(x[r].contiguous(), w2[i], y[r].contiguous(), spec)), 'fwd_masked')
  # ---- backward-data, plain and masked
  gx = O.conv_bwd_data_raw(gy, w2, tuple(x.shape), spec)
  whole('bwd_data', _last_kernel(), bwd_whole)
  same(gx, per_set(lambda i, r: O.conv_bwd_data_raw(gy[r].contiguous(), w2[i], (h,) + tuple(x.shape[1:]), spec)), 'bwd_data')
  gm = O.conv_bwd_data_masked_raw(gy, w2, x, spec)
  rec['bwd_data_masked'] = _last_kernel()
  same(gm, per_set(lambda i, r: O.conv_bwd_data_masked_raw(gy[r].contiguous(), w2[i], x[r].contiguous(), spec)), 'bwd_data_masked')
  # ---- the oracle on the first and last image of every group
  KF, KB = k * k * cin, k * k * cout

  def each(got, ref, bound, name, i, s3):
    _ew_note('grouped edge ' + name, dname, E.assert_elementwise(got, ref, bound, '%s %s group %d images %s' % (cid, name, i, s3)))
  for i in range(G):
    sel = sorted({i * h, (i + 1) * h - 1})
    # element-wise: first, last and one seeded middle image of EVERY group
    sel3 = _with_middle(sel, '%s:%d' % (cid, i), i * h, (i + 1) * h)
    pos = [sel3.index(j) for j in sel]
    wn, bn = host(w2[i]), host(b2[i])
    x3, g3 = host(x[sel3]), host(gy[sel3])
    lin3, lmag3 = N.conv2d_gemm(x3, wn, pad), N.conv2d_gemm(np.abs(x3), np.abs(wn), pad)
    lin = lin3[pos]
    close(host(y[sel]), N.leaky_relu(lin + bn), otol, 'fwd vs oracle, group %d' % i)
    act3 = N.leaky_relu(lin3 + bn)
    each(host(y[sel3]), act3, E.conv_bound(act3, lmag3 + np.abs(bn), KF + 2, dtype), 'fwd', i, sel3)
    close(host(ym[sel]), lin * np.where(host(y[sel]) > 0, 1.0, 0.2), otol, 'fwd_masked vs oracle, group %d' % i)
    ysl = np.where(host(y[sel3]) > 0, 1.0, 0.2)      # y is the mask SOURCE of this launch, an input to it: exact
    each(host(ym[sel3]), lin3 * ysl, E.conv_bound(lin3 * ysl, lmag3 * ysl, KF + 1, dtype, _twice(lin3 * ysl, ysl, dtype)),
         'fwd_masked', i, sel3)
    ref3 = N.conv2d_bwd_data_gemm(g3, wn, (hw, hw), pad)
    rmag3 = N.conv2d_bwd_data_gemm(np.abs(g3), np.abs(wn), (hw, hw), pad)
    ref = ref3[pos]
    close(host(gx[sel]), ref, otol, 'bwd_data vs oracle, group %d' % i)
    each(host(gx[sel3]), ref3, E.conv_bound(ref3, rmag3, KB, dtype), 'bwd_data', i, sel3)
    close(host(gm[sel]), ref * np.where(host(x[sel]) > 0, 1.0, 0.2), otol, 'bwd_data_masked vs oracle, group %d' % i)
    xsl = np.where(x3 > 0, 1.0, 0.2)
    each(host(gm[sel3]), ref3 * xsl, E.conv_bound(ref3 * xsl, rmag3 * xsl, KB + 1, dtype, _twice(ref3 * xsl, xsl, dtype)),
         'bwd_data_masked', i, sel3)
  del ym, gm
  # ---- block ends: pooled output (+ sign bytes), and the backward-data that unpools
  if k == 3 and pad == 'SAME' and hw >= 16:
    z, zp = O.conv_fwd_pool_raw(x, w2, b2, spec, epi)
    rec['fwd_pool'] = _last_kernel()
    ref = per_set(lambda i, r: O.conv_fwd_pool_raw(x[r].contiguous(), w2[i], b2[i], spec, epi))
    same(z, [p[0] for p in ref], 'fwd_pool z')
    same(zp, [p[1] for p in ref], 'fwd_pool pooled')
    assert O.conv_fwd_pool_signs_supported(x, w2, spec, epi)
    sg, zp2 = O.conv_fwd_pool_signs_raw(x, w2, b2, spec, epi)
    rec['fwd_pool_signs'] = _last_kernel()
    ref = per_set(lambda i, r: O.conv_fwd_pool_signs_raw(x[r].contiguous(), w2[i], b2[i], spec, epi))
    same(sg, [p[0] for p in ref], 'fwd_pool_signs bits')
    same(zp2, [p[1] for p in ref], 'fwd_pool_signs pooled')
    gzp = gy[:, ::2, ::2, :].contiguous()
    out = O.conv_bwd_data_unpool_raw(gzp, sg, w2, x, tuple(x.shape), spec, True)
    assert out is not None
    rec['bwd_data_unpool'] = _last_kernel()
    ref = per_set(lambda i, r: O.conv_bwd_data_unpool_raw(gzp[r].contiguous(), sg[r].contiguous(), w2[i], x[r].contiguous(),
                                                          (h,) + tuple(x.shape[1:]), spec, True))
    same(out[0], [p[0] for p in ref], 'unpool gx')
    same(out[1], [p[1] for p in ref], 'unpool kept gradient')
    del z, zp, sg, zp2, out, ref
  # ---- filter (+ bias) gradients into zeroed stacked sinks: the bound of test_grouped_conv_equals_one_call_per_weight_set
  tol = 2e-5
  gw = O.conv_bwd_weight_raw(x, gy, spec, groups=G)
  ref = torch.stack(per_set(lambda i, r: O.conv_bwd_weight_raw(x[r].contiguous(), gy[r].contiguous(), spec)))
  assert gw.shape == ref.shape
  close(host(gw), host(ref), tol, 'bwd_weight')
  sink, bsink = torch.zeros_like(w2), torch.zeros_like(b2)
  O.conv_bwd_weight_raw(x, gy, spec, out=sink, gbias=bsink)
  close(host(sink), host(ref), tol, 'bwd_weight_bias')
  close(host(bsink), host(gy.float().reshape(G, -1, cout).sum(1)), 1e-3, 'bwd_weight_bias bias')
  # fp32 filter and bias gradients of every group against the float64 oracle: sums over P = (n / G) ho wo pixels, any order
  P = h * ho * ho
  for i in range(G):
    xi, gi = host(x[i * h:(i + 1) * h]), host(gy[i * h:(i + 1) * h])
    want_w = _edge_wgrad_oracle(xi, gi, k, pad)
    wb = E.wgrad_bound(want_w, _edge_wgrad_oracle(np.abs(xi), np.abs(gi), k, pad), P)
    r = E.assert_elementwise(host(gw[i]), want_w, wb, '%s bwd_weight group %d' % (cid, i))
    r = max(r, E.assert_elementwise(host(sink[i]), want_w, wb, '%s bwd_weight_bias group %d' % (cid, i)))
    gsum = gi.sum(axis=(0, 1, 2))
    r = max(r, E.assert_elementwise(host(bsink[i]), gsum, E.wgrad_bound(gsum, np.abs(gi).sum(axis=(0, 1, 2)), P),
                                    '%s bias gradient group %d' % (cid, i)))
    _ew_note('grouped edge bwd_weight', dname, r)
  if O.conv_bwd_weight2_raw(x, gy, x, gy, spec, sink, bsink, 3):      # two segments, both grouped
    close(host(sink), 3.0 * host(ref), tol, 'bwd_weight2')
  del gw, ref, sink, bsink
  # ---- a registered stacked weight: packs made by get(), re-made in place by refresh() after the weights moved
  if refresh:
    O.PackCache.register(w2)
    try:
      O.conv_fwd_raw(x, w2, b2, spec, epi)
      O.conv_bwd_data_raw(gy, w2, tuple(x.shape), spec)
      with torch.no_grad():
        w2.mul_(1.5)
      O.PackCache.version += 1
      assert O.PackCache.refresh([w2]) >= 2
      same(O.conv_fwd_raw(x, w2, b2, spec, epi),
           per_set(lambda i, r: O.conv_fwd_raw(x[r].contiguous(), w2[i].clone(), b2[i], spec, epi)), 'fwd after refresh')
      same(O.conv_bwd_data_raw(gy, w2, tuple(x.shape), spec),
           per_set(lambda i, r: O.conv_bwd_data_raw(gy[r].contiguous(), w2[i].clone(), (h,) + tuple(x.shape[1:]), spec)),
           'bwd_data after refresh')
    finally:
      O.PackCache.unregister(w2)
  _edge_symbols_check(cid, dname, rec)


def _lockstep_cases():
  out = []
  for cid, k, pad, hw, cin, cout, n_lo, n_hi, _ in EDGE_CASES:
    out += [('%s_n%d' % (cid, n), 1, k, pad, hw, hw, cin, cout, n) for n in (n_lo, n_hi)]
  for cid, G, k, pad, hw, cin, cout, n, _, _, _ in GROUPED_EDGE_CASES:
    out.append((cid, G, k, pad, hw, hw, cin, cout, n))
  for n, h, w, cin, cout, k, pad in MFMA_CASES:
    out.append(('mfma_n%d_%dx%d_c%d_%d_k%d' % (n, h, w, cin, cout, k), 1, k, pad, h, w, cin, cout, n))
  return out


LOCKSTEP_CASES = _lockstep_cases()


@pytest.mark.parametrize('case', LOCKSTEP_CASES, ids=[c[0] for c in LOCKSTEP_CASES])
def test_pack_layout_follows_the_kernel_that_runs(ops, case):
  """tg_conv2d_pack_layout(desc, mode) re-derives where tg_conv2d_fwd (mode 0) / tg_conv2d_bwd_data (mode 1) will end: it
  must say "fragment order" exactly when the kernel that then runs is conv_img_kernel or conv_small_kernel, the two that
  read such packs -- for a grouped descriptor launched once per group, the kernel of the per-group launch."""
  import twingan_amd.ops as O
  from twingan_amd import _lib
  cid, G, k, pad, h, w, cin, cout, n = case
  spec = O.ConvSpec(k, pad)
  ho, wo = spec.out_hw(h, w)
  d = O._desc((n, h, w, cin), cout, spec, torch.bfloat16, 0, G)
  assert d.algo == _lib.TG_ALGO_MFMA
  x = torch.zeros(n, h, w, cin, dtype=torch.bfloat16, device=dev())
  gy = torch.zeros(n, ho, wo, cout, dtype=torch.bfloat16, device=dev())
  wt = torch.zeros(((G,) if G > 1 else ()) + (k, k, cin, cout), device=dev())
  for mode in (0, 1):
    if mode == 0:
      O.conv_fwd_raw(x, wt, None, spec, 0)
    else:
      O.conv_bwd_data_raw(gy, wt, tuple(x.shape), spec)
    sym = _last_kernel()
    frag = int(sym.startswith(('conv_img_kernel', 'conv_small_kernel')))
    assert _lib.load().tg_conv2d_pack_layout(ctypes.byref(d), mode) == frag, \
        '%s mode %d: pack layout %d, but the pack is read by %s' % (cid, mode, 1 - frag, sym)


# =====================================================================================================================
# Element-wise parity of the streaming kernels (norm.hip, reduce.hip, pointwise.hip) at the sizes and edges that reach
# the branches of their host code.  Every output element against its own bound (tests/elementwise.py: the formulas and
# their derivation); the references are float64 autograd of the literal formulas, E32 their float32 restatement.
# =====================================================================================================================
def _round_to(a, dtype):
  """numpy / tensor values rounded to the storage type -> float64 torch tensor on the CPU."""
  t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
  return t.float().to(dtype).double().cpu()


def _norm_chunking(n, hw, pool=False):
  """The host's own arithmetic (norm.hip: norm_chunks, and the streaming pass' ~2048 blocks), restated to NAME the branch a
  case is for: -> ((chunks, ppb, tail) of pass 1, the same of pass 2)."""
  floor = 16 if hw <= 64 else 32 if hw <= 256 else 64
  ch = (1024 + n - 1) // n
  pp = max((hw + ch - 1) // ch, floor)
  units = hw // 4 if pool else hw
  c2 = (2048 + n - 1) // n
  pp2 = max((units + c2 - 1) // c2, 16 if pool else floor)
  return ((hw + pp - 1) // pp, pp, hw % pp), ((units + pp2 - 1) // pp2, pp2, units % pp2)


NORM_EDGE_CASES = [
    # id (the branch it is for), n, h, w, c, lrelu, pixel norm, pool, split (None: one domain), mode
    #   mode 'ret': gradients returned (the separate parameter-gradient kernel); 'sink': added into registered buffers that
    #   already hold values (16-bit: atomics; fp32: ordered); 'det': the same in deterministic mode (ordered in every type)
    ('p1_15x64_p2_15x64_pool_15x16', 3, 40, 24, 16, True, True, True, 1, 'ret'),
    ('hw221_floor32_tail29_split0', 5, 17, 13, 8, True, True, False, 0, 'sink'),
    ('p1_ppb128_p2_ppb66_tail4_pool_ppb17_tail4_split_n-1', 33, 64, 64, 8, True, True, True, 32, 'ret'),
    ('p1_ppb128_tail112_p2_ppb65_tail50_split_n', 33, 60, 68, 16, True, True, False, 33, 'sink'),
    ('n2_255_chunks_pool', 2, 136, 120, 16, True, True, True, 1, 'det'),
    ('n1_1024_chunks', 1, 256, 256, 16, True, True, False, None, 'ret'),
    ('n130_hw64_4_chunks_c48_scalar', 130, 8, 8, 48, True, False, False, 65, 'sink'),
    ('hw64_floor16_c24_scalar', 3, 8, 8, 24, True, False, False, None, 'ret'),
    ('hw65_floor32_tail1_c24_scalar', 3, 5, 13, 24, True, False, False, 1, 'ret'),
    ('hw256_floor32_c5_scalar_pool', 3, 16, 16, 5, True, False, True, None, 'ret'),
    ('hw257_floor64_tail1_c5_scalar', 3, 1, 257, 5, False, False, False, 2, 'sink'),
    ('hw258_floor64_tail2_c3_scalar', 3, 3, 86, 3, True, False, False, 1, 'det'),
    ('tail60_pool_tail15_c256', 2, 34, 30, 256, True, True, True, 1, 'ret'),
    ('tail12_pool_tail3_c512_widest_vector', 3, 18, 22, 512, True, True, True, 2, 'sink'),
]


def _norm_inputs(n, h, w, c, pool, dtype, seed):
  rng = np.random.RandomState(seed)
  y = _round_to(rng.randn(n, h, w, c) * 1.5 + 0.7 + 0.5 * rng.randn(1, 1, 1, c), dtype)
  gz = _round_to(rng.randn(n, h, w, c), dtype)
  gzp = _round_to(rng.randn(n, h // 2, w // 2, c), dtype) if pool else None
  par = [torch.from_numpy((o + s * rng.randn(c)).astype(np.float32)).double() for o, s in ((1.0, 0.2), (0.0, 0.1)) * 2]
  return y, gz, gzp, par


def _near_zero(r64, r32):
  """Where the float64 pre-activation u is inside its own bound, 2^-24 |u| + 16 E32(u): the kernels hold u in fp32 whatever
  the storage type.  E32(u) is taken over the elements the bound is applied to, |u| < 2^-6, when there are at least 256 of
  them (the maximum over the whole tensor belongs to the largest |u| and is ten times theirs)."""
  u, u32 = r64['u'].numpy(), r32['u'].numpy()
  small = np.abs(u) < 2.0 ** -6
  e_u = E.e32(u32[small], u[small]) if small.sum() >= 256 else E.e32(u32, u)
  return np.abs(u) < E.e32_bound(u, e_u, torch.float32)


def _seeded(make, refs, lrelu, seed):
  """The first of seeds seed, seed + 1, ... whose float64 reference ALONE has fewer than 1e-5 of its pre-activations inside
  their bound (a condition on the inputs, decided before any kernel runs) -> (inputs, r64, r32, near)."""
  for s in range(seed, seed + 8):
    inp = make(s)
    r64, r32 = refs(inp, torch.float64), refs(inp, torch.float32)
    near = _near_zero(r64, r32) if lrelu else None
    if near is None or near.mean() < 1e-5:
      return inp, r64, r32, near
  raise AssertionError('no seed in [%d, %d) meets the LeakyReLU condition' % (seed, seed + 8))


def _check_norm_outputs(what, dname, got, r64, r32, dtype, family, near=None, flip_ref=None, gy_extra=None):
  """z, zp, gy of a fused normaliser against the float64 reference: u |ref| + 16 E32 per element.
  zp: the kernels pool the STORED z (norm.hip: "the pool reads the stored (rounded) z", so that the pooled tensor is the pool
  of the skip tensor whichever kernel wrote it): the mean of four roundings, u mean4 |z|, is that path's own further term.
  gy takes its LeakyReLU mask from a computed sign: where `near` holds (_near_zero) the other slope is accepted, for at most
  1e-5 of the elements."""
  u_st = E.unit_roundoff(dtype)
  ref = r64['z'].numpy()
  r = E.assert_elementwise(host(got['z']), ref, E.e32_bound(ref, E.e32(r32['z'].numpy(), ref), dtype), what + ' z')
  _ew_note(family + ' z', dname, r)
  if r64['zp'] is not None:
    n, h, w, c = ref.shape
    ref = r64['zp'].numpy()
    zmag = np.abs(r64['z'].numpy()).reshape(n, h // 2, 2, w // 2, 2, c).mean(axis=(2, 4))
    bound = E.e32_bound(ref, E.e32(r32['zp'].numpy(), ref), dtype) + (1 + u_st) * u_st * zmag
    _ew_note(family + ' zp', dname, E.assert_elementwise(host(got['zp']), ref, bound, what + ' zp'))
  ref = r64['gy'].numpy()
  bound = E.e32_bound(ref, E.e32(r32['gy'].numpy(), ref), dtype)
  if gy_extra is not None:
    bound = bound + gy_extra
  alt = None
  if near is not None and near.any():
    alt = flip_ref(torch.from_numpy(near))['gy'].numpy()
  r = E.assert_elementwise(host(got['gy']), ref, bound, what + ' gy', alt_ref=alt, alt_where=near)
  _ew_note(family + ' gy', dname, r)


@pytest.mark.parametrize('dname', sorted(EW_DTYPES))
@pytest.mark.parametrize('case', NORM_EDGE_CASES, ids=[c[0] for c in NORM_EDGE_CASES])
def test_norm_act_elementwise_at_chunk_edges(ops, case, dname):
  """ops.norm_act (tg_instance_norm_partials + tg_norm_act_fwd_partials, tg_norm_act_bwd) forward and backward, every element
  of z, the pooled z, gy and the parameter gradients against float64, at shapes that reach: a tail chunk in pass 1 and in pass
  2, different chunk counts in the two passes, both sides of the min_ppb steps at hw 64 and 256, the scalar path (c = 3, 5;
  24 and 48 by the power-of-two rule), the widest vector path (c = 512: 16-bit only, fp32 must refuse it), split at 0, 1,
  n-1 and n, and the three ways the parameter gradients leave the kernel."""
  import twingan_amd.ops as O
  from twingan_amd import _lib
  name, n, h, w, c, lrelu, pn, pool, split, mode = case
  dtype = EW_DTYPES[dname]
  p1, p2 = _norm_chunking(n, h * w, pool)
  print('[norm chunks] %s: pass 1 (chunks, ppb, tail) %s, pass 2 %s' % (name, p1, p2))
  assert _lib.load().tg_norm_chunks(n, h, w) == p1[0], 'norm_chunks moved: the case ids of NORM_EDGE_CASES name stale branches'
  two = split is not None

  def refs(inp, dt, flip=None):
    y, gz, gzp, par = inp
    return E.norm_act_reference(y.to(dt), par[0], par[1], gz, par[2] if two else None, par[3] if two else None, split=split,
                                lrelu=lrelu, pixel_norm=pn, pool=pool, gzp=gzp, flip=flip)
  inp, r64, r32, near = _seeded(lambda s: _norm_inputs(n, h, w, c, pool, dtype, s), refs, lrelu, 70 + len(name))
  y, gz, gzp, par = inp
  yd = y.to(dev()).to(dtype).contiguous().requires_grad_(True)
  pd = [p.float().to(dev()).requires_grad_(True) for p in (par if two else par[:2])]
  kw = dict(lrelu=lrelu, pixel_norm=pn, pool=pool)
  if two:
    kw.update(gamma2=pd[2], beta2=pd[3], split=split)
  if c == 512 and dtype == torch.float32:
    with pytest.raises(_lib.TgError, match='pixel norm needs c'):      # loud, not a fall-back
      O.norm_act(yd, pd[0], pd[1], **kw)
    return
  lib = _lib.load()
  was = lib.tg_set_deterministic(1) if mode == 'det' else None
  pre = [torch.from_numpy(np.random.RandomState(5 + i).randn(c).astype(np.float32)).to(dev()) for i in range(len(pd))]
  sinks = [t.clone() for t in pre]
  try:
    if mode != 'ret':
      for p, s in zip(pd, sinks):
        O.GradSink.register(p, s)
    out = O.norm_act(yd, pd[0], pd[1], **kw)
    z, zp = out if pool else (out, None)
    gzd = gz.to(dev()).to(dtype)
    if pool:
      torch.autograd.backward([z, zp], [gzd, gzp.to(dev()).to(dtype)])
    else:
      z.backward(gzd)
    torch.cuda.synchronize()
  finally:
    for p in pd:
      O.GradSink.unregister(p)
    if was is not None:
      lib.tg_set_deterministic(was)

  _check_norm_outputs('norm_act[%s,%s]' % (name, dname), dname, dict(z=z, zp=zp, gy=yd.grad), r64, r32, dtype, 'norm_act',
                      near, lambda f: refs(inp, torch.float64, f))
  for i, nm in enumerate(('gamma', 'beta', 'gamma2', 'beta2')[:len(pd)]):
    ref = r64['grads'][i].numpy()
    bound = E.e32_bound(ref, E.e32(r32['grads'][i].numpy(), ref), torch.float32)
    if mode == 'ret':
      got = host(pd[i].grad)
    else:      # added into what the buffer held: one more fp32 addition, its rounding named here
      assert pd[i].grad is None
      got = host(sinks[i]) - host(pre[i])
      bound = bound + 2.0 ** -24 * (np.abs(host(pre[i])) + np.abs(ref))
    r = E.assert_elementwise(got, ref, bound, 'norm_act[%s,%s] %s gradient (%s)' % (name, dname, nm, mode))
    _ew_note('norm_act parameter grads', dname, r)


@pytest.mark.parametrize('dname', sorted(EW_DTYPES))
@pytest.mark.parametrize('c,pn', [(24, True), (48, True), (520, True), (520, False), (3, True)])
def test_norm_act_refuses_what_it_cannot_run(ops, c, pn, dname):
  """Pixel norm needs c = VN * 2^k <= 64 VN (VN = 8 in 16-bit storage, 4 in fp32); without it c <= 256 on the scalar path,
  and 520 = 8 * 65 fits neither.  The refusal is an error with the reason in it, never another code path."""
  import twingan_amd.ops as O
  from twingan_amd import _lib
  dtype = EW_DTYPES[dname]
  y = torch.ones((2, 6, 6, c), dtype=dtype, device=dev())
  ga, be = torch.ones(c, device=dev()), torch.zeros(c, device=dev())
  with pytest.raises(_lib.TgError, match='pixel norm needs c|scalar path needs c'):
    O.norm_act(y, ga, be, lrelu=True, pixel_norm=pn)


ROWS_CASES = [('tail12_c32', 4, 18, 22, 32, True, True), ('hw65_c8_pool_unfused', 3, 10, 26, 8, True, True),
              ('c5_scalar', 3, 5, 13, 5, False, False)]


@pytest.mark.parametrize('dname', sorted(EW_DTYPES))
@pytest.mark.parametrize('case', ROWS_CASES, ids=[c[0] for c in ROWS_CASES])
def test_norm_act_per_image_parameters_elementwise(ops, case, dname):
  """The non-partials route: tg_instance_norm_stats + tg_norm_act_fwd with one parameter row per image (batch renorm's
  form), its backward writing [n, c] row gradients; the pool is then the stand-alone kernel."""
  import twingan_amd.ops as O
  name, n, h, w, c, pn, pool = case
  dtype = EW_DTYPES[dname]

  def make(seed):
    rng = np.random.RandomState(seed + 1000)
    return _norm_inputs(n, h, w, c, pool, dtype, seed)[:3] + (
        [torch.from_numpy((o + s * rng.randn(n, c)).astype(np.float32)).double() for o, s in ((1.0, 0.2), (0.0, 0.1))],)

  def refs(inp, dt, flip=None):
    y, gz, gzp, rows = inp
    return E.norm_act_reference(y.to(dt), rows[0], rows[1], gz, lrelu=True, pixel_norm=pn, pool=pool, gzp=gzp, flip=flip)
  inp, r64, r32, near = _seeded(make, refs, True, 91)
  y, gz, gzp, rows = inp
  yd = y.to(dev()).to(dtype).contiguous().requires_grad_(True)
  rd = [r.float().to(dev()).requires_grad_(True) for r in rows]
  stats = O.instance_stats(yd.detach(), 1e-6)
  # the statistics kernel on its own: mean and rstd per (image, channel), fp32
  yn = y.numpy().reshape(n, h * w, c)
  m64, v64 = yn.mean(axis=1), yn.var(axis=1)
  y32 = y.float()
  m32 = y32.mean(dim=(1, 2))
  v32 = ((y32 - m32.view(n, 1, 1, c)) ** 2).mean(dim=(1, 2))
  r64s, r32s = 1.0 / np.sqrt(v64 + 1e-6), torch.rsqrt(v32 + 1e-6).numpy()
  r = E.assert_elementwise(host(stats[0]).reshape(n, c), m64, E.e32_bound(m64, E.e32(m32.numpy(), m64), torch.float32),
                           'instance_stats[%s,%s] mean' % (name, dname))
  _ew_note('instance_norm_stats', dname, r)
  r = E.assert_elementwise(host(stats[1]).reshape(n, c), r64s, E.e32_bound(r64s, E.e32(r32s, r64s), torch.float32),
                           'instance_stats[%s,%s] rstd' % (name, dname))
  _ew_note('instance_norm_stats', dname, r)
  out = O.norm_act(yd, rd[0], rd[1], lrelu=True, pixel_norm=pn, pool=pool, stats=stats)
  z, zp = out if pool else (out, None)
  if pool:
    torch.autograd.backward([z, zp], [gz.to(dev()).to(dtype), gzp.to(dev()).to(dtype)])
  else:
    z.backward(gz.to(dev()).to(dtype))

  _check_norm_outputs('rows[%s,%s]' % (name, dname), dname, dict(z=z, zp=zp, gy=yd.grad), r64, r32, dtype, 'norm_act rows',
                      near, lambda f: refs(inp, torch.float64, f))
  for i, nm in enumerate(('gamma rows', 'beta rows')):
    ref = r64['grads'][i].numpy()
    r = E.assert_elementwise(host(rd[i].grad), ref, E.e32_bound(ref, E.e32(r32['grads'][i].numpy(), ref), torch.float32),
                             'rows[%s,%s] %s gradient' % (name, dname, nm))
    _ew_note('norm_act rows parameter grads', dname, r)


# ------------------------------------------------------------------------------------------------ streaming ops, element by element
def _f32_ops_bound(ref, mag, ops_, dtype):
  """A value computed by `ops_` fp32 operations on terms of magnitude `mag`, stored once: u |ref| + (1 + u) ops 2^-24 mag."""
  return E.conv_bound(ref, mag, ops_, dtype)


def _sum4_bound(ref, mag, dtype):
  """A sum of four stored values (pool, upsample adjoint).  16-bit storage: the fp32 sum of four 16-bit values of one scale is
  exact, the output is one rounding of it -- u |ref| and nothing else.  fp32 storage: the three additions round, so
  2^-24 |ref| + 3 2^-24 sum|x| (the one place where this file needs more than the plain rounding for these ops)."""
  return E.rounded_bound(ref, dtype) if dtype != torch.float32 else _f32_ops_bound(ref, mag, 3, dtype)


STREAM_SHAPES = [
    # id, n, h, w, c
    ('bench_past_2p24_elements', 17, 256, 256, 16),      # 17.8 M elements: an index held in a float, or 24 bits, would show
    ('odd_non_square_c5', 3, 10, 14, 5),                 # scalar path, nothing a multiple of anything
    ('one_past_a_vector_c9', 2, 6, 4, 9),                # 16-bit vectors hold 8, fp32 vectors 4: one channel past both
    ('c24_three_vectors', 2, 4, 6, 24),
]


def _stream_inputs(shape, dtype, seed, k=1):
  rng = np.random.RandomState(seed)
  return [_round_to(torch.from_numpy(rng.standard_normal(shape).astype(np.float32)), dtype) for _ in range(k)]


def _up2(a):
  return a.repeat(2, axis=1).repeat(2, axis=2)


def _sum4(a):
  n, h, w, c = a.shape
  return a.reshape(n, h // 2, 2, w // 2, 2, c).sum(axis=(2, 4))


@pytest.mark.parametrize('dname', sorted(EW_DTYPES))
@pytest.mark.parametrize('case', STREAM_SHAPES, ids=[c[0] for c in STREAM_SHAPES])
def test_pool_and_upsample_elementwise(ops, case, dname):
  """tg_pool2x2_fwd / _bwd (and the pool of the backward's backward), tg_upsample2x_concat_fwd / _bwd without groups.
  Copies are exact (array_equal), a multiplication by 0.25 is exact down to the type's smallest numbers, a sum of four stored
  values is bounded by _sum4_bound: u |ref| alone in 16-bit storage."""
  name, n, h, w, c = case
  dtype = EW_DTYPES[dname]
  x, gyp, v = _stream_inputs((n, h, w, c), dtype, 300, 1) + _stream_inputs((n, h // 2, w // 2, c), dtype, 301, 1) + \
      _stream_inputs((n, h, w, c), dtype, 302, 1)
  xd = x.to(dev()).to(dtype).requires_grad_(True)
  y = ops.avg_pool2(xd)
  xn = x.numpy()
  ref = 0.25 * _sum4(xn)
  _ew_note('pool2x2 fwd', dname, E.assert_elementwise(host(y), ref, _sum4_bound(ref, 0.25 * _sum4(np.abs(xn)), dtype),
                                                      'avg_pool2 fwd %s %s' % (name, dname)))
  gyd = gyp.to(dev()).to(dtype).requires_grad_(True)
  gx, = torch.autograd.grad(y, xd, grad_outputs=gyd, create_graph=True)
  # an exact scaled copy (a power of two) -- down to the storage type's smallest numbers: bound tiny(dtype) and nothing else
  _ew_note('pool2x2 bwd', dname, E.assert_elementwise(host(gx), 0.25 * _up2(gyp.numpy()), E.tiny(dtype), 'avg_pool2 bwd %s %s' % (name, dname)))
  ggy, = torch.autograd.grad(gx, gyd, grad_outputs=v.to(dev()).to(dtype))
  vn = v.numpy()
  ref = 0.25 * _sum4(vn)
  _ew_note('pool2x2 bwd-bwd', dname, E.assert_elementwise(host(ggy), ref, _sum4_bound(ref, 0.25 * _sum4(np.abs(vn)), dtype),
                                                          'avg_pool2 bwd-bwd %s %s' % (name, dname)))
  del y, gx, ggy, xd, gyd
  # upsample + concat: x0 at half resolution, x1 (c + 3 channels: the two halves differ) at full resolution
  c1 = c + 3
  x0, = _stream_inputs((n, h // 2, w // 2, c), dtype, 303)
  x1, go = _stream_inputs((n, h, w, c1), dtype, 304)[0], _stream_inputs((n, h, w, c + c1), dtype, 305)[0]
  a, b = x0.to(dev()).to(dtype).requires_grad_(True), x1.to(dev()).to(dtype).requires_grad_(True)
  out = ops.upsample2x_concat(a, b)
  assert np.array_equal(host(out), np.concatenate([_up2(x0.numpy()), x1.numpy()], axis=3)), ('upsample2x_concat fwd', name, dname)
  out.backward(go.to(dev()).to(dtype))
  gon = go.numpy()
  ref = _sum4(gon[..., :c])
  _ew_note('upsample2x_concat bwd', dname, E.assert_elementwise(
      host(a.grad), ref, _sum4_bound(ref, _sum4(np.abs(gon[..., :c])), dtype), 'upsample2x_concat bwd g0 %s %s' % (name, dname)))
  assert np.array_equal(host(b.grad), gon[..., c:]), ('upsample2x_concat bwd g1 is a copy', name, dname)


@pytest.mark.parametrize('dname', sorted(EW_DTYPES))
@pytest.mark.parametrize('n,h,w,c0,c1,gsz,perm', [(8, 6, 10, 5, 9, 2, (1, 0, 0, 1)), (12, 4, 4, 16, 8, 4, (0, 1, 1)),
                                                  (64, 64, 64, 16, 16, 16, (1, 0, 0, 1))])
def test_upsample_concat_group_permutation_elementwise(ops, dname, n, h, w, c0, c1, gsz, perm):
  """The skip source shared between passes: output group g reads skip images [perm[g] gsz, (perm[g] + 1) gsz); the backward
  adds the gradients of every group that read an image in fp32 and stores once."""
  dtype = EW_DTYPES[dname]
  n1 = (max(perm) + 1) * gsz
  x0, = _stream_inputs((n, h, w, c0), dtype, 310)
  x1, = _stream_inputs((n1, 2 * h, 2 * w, c1), dtype, 311)
  go, = _stream_inputs((n, 2 * h, 2 * w, c0 + c1), dtype, 312)
  a, b = x0.to(dev()).to(dtype).requires_grad_(True), x1.to(dev()).to(dtype).requires_grad_(True)
  out = ops.upsample2x_concat(a, b, gsz, perm)
  src = [perm[i // gsz] * gsz + i % gsz for i in range(n)]
  assert np.array_equal(host(out), np.concatenate([_up2(x0.numpy()), x1.numpy()[src]], axis=3))
  out.backward(go.to(dev()).to(dtype))
  gon = go.numpy()
  ref = _sum4(gon[..., :c0])
  _ew_note('upsample2x_concat bwd', dname, E.assert_elementwise(
      host(a.grad), ref, _sum4_bound(ref, _sum4(np.abs(gon[..., :c0])), dtype), 'grouped upsample2x_concat g0'))
  ref1, mag1, cnt = np.zeros(x1.shape), np.zeros(x1.shape), np.zeros(n1, int)
  for i, s_ in enumerate(src):
    ref1[s_] += gon[i, ..., c0:]
    mag1[s_] += np.abs(gon[i, ..., c0:])
    cnt[s_] += 1
  _ew_note('upsample2x_concat bwd', dname, E.assert_elementwise(
      host(b.grad), ref1, _f32_ops_bound(ref1, mag1, int(cnt.max()) - 1 if cnt.max() > 1 else 1, dtype), 'grouped upsample2x_concat g1'))


@pytest.mark.parametrize('dname', sorted(EW_DTYPES))
@pytest.mark.parametrize('case', STREAM_SHAPES, ids=[c[0] for c in STREAM_SHAPES])
def test_lrelu_backward_family_elementwise(ops, case, dname):
  """tg_lrelu_bwd, tg_lrelu_pool_bwd (with and without either gradient, with the bias gradient), tg_lrelu_bwd_bias (the same
  launcher without a pooled gradient), tg_lrelu_pool_bwd_signs, tg_channel_sum and its ordered form, tg_bias_lrelu_fwd.
  The masks come from an INPUT tensor (exact).  g * slope is one fp32 multiplication by float32(0.2), gz + 0.25 up(gzp) one
  fused multiply-add before it: 1 / 2 fp32 operations, then the storage rounding.  The bias gradient is the fp32 sum of the
  values the kernel STORED (norm.hip: `a[j] += rnd(g)`): the float64 sum of the reference, with the sum of the elements' own
  bounds added to the summation bound."""
  import twingan_amd.ops as O
  from twingan_amd import _lib
  name, n, h, w, c = case
  dtype = EW_DTYPES[dname]
  al = float(np.float32(0.2))
  gz, z = _stream_inputs((n, h, w, c), dtype, 320, 2)
  gzp, = _stream_inputs((n, h // 2, w // 2, c), dtype, 321)
  bias = torch.zeros(c, device=dev())
  gzd, zd, gzpd = (t.to(dev()).to(dtype).contiguous() for t in (gz, z, gzp))
  slope = np.where(z.numpy() > 0, 1.0, al)
  ref = gz.numpy() * slope
  _ew_note('lrelu_bwd', dname, E.assert_elementwise(host(O.lrelu_bwd_raw(gzd, zd, 0.2)), ref,
                                                    _f32_ops_bound(ref, np.abs(ref), 1, dtype), 'lrelu_bwd %s %s' % (name, dname)))
  P = n * h * w
  for use_gz, use_gzp in ((True, True), (False, True), (True, False)):
    pre = (gz.numpy() if use_gz else 0.0) + (0.25 * _up2(gzp.numpy()) if use_gzp else 0.0)
    mag = ((np.abs(gz.numpy()) if use_gz else 0.0) + (0.25 * _up2(np.abs(gzp.numpy())) if use_gzp else 0.0)) * slope
    ref = pre * slope
    g, gb = O.lrelu_pool_bwd(gzd if use_gz else None, gzpd if use_gzp else None, zd, 0.2, bias, True)
    what = 'lrelu_pool_bwd gz=%d gzp=%d %s %s' % (use_gz, use_gzp, name, dname)
    gbound = _f32_ops_bound(ref, mag, 2, dtype)
    _ew_note('lrelu_pool_bwd', dname, E.assert_elementwise(host(g), ref, gbound, what))
    # the bias gradient is the fp32 sum of the STORED g: against the float64 sum of the reference, every summand within its
    # own element bound (their sum), plus the fp32 summation over P pixels
    bsum, bmag_ = ref.reshape(-1, c).sum(axis=0), np.abs(ref).reshape(-1, c).sum(axis=0)
    bbound = E.wgrad_bound(bsum, bmag_, P) + gbound.reshape(-1, c).sum(axis=0)
    _ew_note('lrelu_pool_bwd bias', dname, E.assert_elementwise(host(gb), bsum, bbound, what + ' bias'))
    if use_gzp and not use_gz and c % 8 == 0 and dtype != torch.float32:      # the sign-byte form of the same backward
      bits = (zd > 0).view(n, h, w, c // 8, 8).to(torch.int32)
      signs = (bits << torch.arange(8, device=zd.device, dtype=torch.int32)).sum(dim=-1).to(torch.uint8).contiguous()
      g2, gb2 = O.lrelu_pool_bwd_signs(gzpd, signs, 0.2, bias, True)
      assert torch.equal(g2, g), what + ': sign-byte form differs'
      _ew_note('lrelu_pool_bwd bias', dname, E.assert_elementwise(host(gb2), bsum, bbound, what + ' signs bias'))
    del g
  # tg_lrelu_bwd_bias: the launcher's form without a pooled gradient, written (accumulate = 0) and added (1)
  for acc in (0, 1):
    g = torch.empty_like(zd)
    gb = torch.full((c,), 3.0 if acc else float('nan'), dtype=torch.float32, device=dev())
    O.call('tg_lrelu_bwd_bias', gzd.data_ptr(), zd.data_ptr(), g.data_ptr(), gb.data_ptr(), P, c, 0.2, acc, O._dt(zd), O._stream())
    ref = gz.numpy() * slope
    gbound = _f32_ops_bound(ref, np.abs(ref), 1, dtype)
    _ew_note('lrelu_bwd_bias', dname, E.assert_elementwise(host(g), ref, gbound, 'lrelu_bwd_bias %s %s' % (name, dname)))
    bsum = ref.reshape(-1, c).sum(axis=0)
    bound = E.wgrad_bound(bsum, np.abs(ref).reshape(-1, c).sum(axis=0), P) + gbound.reshape(-1, c).sum(axis=0) + \
        (2.0 ** -24 * (3.0 + np.abs(bsum)) if acc else 0.0)
    _ew_note('lrelu_bwd_bias bias', dname, E.assert_elementwise(host(gb) - (3.0 if acc else 0.0), bsum, bound,
                                                                'lrelu_bwd_bias bias acc=%d %s %s' % (acc, name, dname)))
  # channel sums: atomic and ordered
  lib = _lib.load()
  gs = gz.numpy().reshape(-1, c)
  for det in (0, 1):
    was = lib.tg_set_deterministic(det)
    try:
      got = O.channel_sum_raw(gzd)
    finally:
      lib.tg_set_deterministic(was)
    _ew_note('channel_sum' + ('_ordered' if det else ''), dname, E.assert_elementwise(
        host(got), gs.sum(axis=0), E.wgrad_bound(gs.sum(axis=0), np.abs(gs).sum(axis=0), P), 'channel_sum det=%d %s %s' % (det, name, dname)))
  # bias + LeakyReLU forward (rows of [npix, c])
  b = torch.from_numpy(np.random.RandomState(322).randn(c).astype(np.float32))
  out = torch.empty_like(zd)
  O.call('tg_bias_lrelu_fwd', zd.data_ptr(), b.to(dev()).data_ptr(), out.data_ptr(), P, c, 0.2, O._dt(zd), O._stream())
  pre = z.numpy() + b.double().numpy()
  ref = np.where(pre > 0, pre, al * pre)      # continuous in pre: no alternates
  _ew_note('bias_lrelu_fwd', dname, E.assert_elementwise(
      host(out), ref, _f32_ops_bound(ref, np.abs(z.numpy()) + np.abs(b.double().numpy()), 2, dtype), 'bias_lrelu_fwd %s %s' % (name, dname)))


@pytest.mark.parametrize('dname', sorted(EW_DTYPES))
@pytest.mark.parametrize('case', STREAM_SHAPES, ids=[c[0] for c in STREAM_SHAPES])
def test_axpby_sample_lerp_gdrop_elementwise(ops, case, dname):
  """tg_axpby (a x + b y: two multiplications and an addition in fp32), tg_sample_lerp (x + alpha[n] (y - x): a subtraction and
  a fused multiply-add), tg_gdrop (x (noise[n, c] s sqrt(C) + 1): the factor in fp32, one multiplication)."""
  import twingan_amd.ops as O
  name, n, h, w, c = case
  dtype = EW_DTYPES[dname]
  x, y = _stream_inputs((n, h, w, c), dtype, 330, 2)
  xd, yd = (t.to(dev()).to(dtype).contiguous() for t in (x, y))
  xn, yn = x.numpy(), y.numpy()
  a, b = float(np.float32(0.3)), float(np.float32(-1.7))
  out = torch.empty_like(xd)
  O.call('tg_axpby', xd.data_ptr(), yd.data_ptr(), out.data_ptr(), xd.numel(), a, b, O._dt(xd), O._stream())
  ref = a * xn + b * yn
  _ew_note('axpby', dname, E.assert_elementwise(host(out), ref, _f32_ops_bound(ref, np.abs(a * xn) + np.abs(b * yn), 3, dtype),
                                                'axpby %s %s' % (name, dname)))
  alpha = torch.from_numpy(np.random.RandomState(331).rand(n).astype(np.float32))
  got = O.sample_lerp(xd, yd, alpha.to(dev()))
  an = alpha.double().numpy().reshape(n, 1, 1, 1)
  ref = xn + an * (yn - xn)
  _ew_note('sample_lerp', dname, E.assert_elementwise(
      host(got), ref, _f32_ops_bound(ref, np.abs(xn) + an * (np.abs(yn) + np.abs(xn)), 3, dtype), 'sample_lerp %s %s' % (name, dname)))
  noise = torch.from_numpy(np.random.RandomState(332).randn(n, c).astype(np.float32))
  cl = c - 1 if c > 4 else c
  f = noise.double().numpy() * (float(np.float32(0.37)) * float(np.sqrt(np.float32(cl)))) + 1.0
  got = O.gdrop(xd, 0.37, noise=noise.to(dev()), c_logical=cl)
  ref = xn * f[:, None, None, :]
  fmag = np.abs(noise.double().numpy()) * 0.37 * np.sqrt(cl) + 1.0
  _ew_note('gdrop', dname, E.assert_elementwise(host(got), ref, _f32_ops_bound(ref, np.abs(xn) * fmag[:, None, None, :], 4, dtype),
                                                'gdrop %s %s' % (name, dname)))


# ------------------------------------------------------------------------------------------------ minibatch stddev, element by element
MBSTD_CASES = [(2, 1, 8), (16, 1, 256), (48, 3, 256), (64, 4, 256), (64, 1, 8), (48, 2, 5), (5, 1, 32)]


@pytest.mark.parametrize('dname', sorted(EW_DTYPES))
@pytest.mark.parametrize('n,groups,c', MBSTD_CASES)
def test_mbstd_elementwise_at_the_discriminator_shapes(ops, n, groups, c, dname):
  """tg_mbstd_fwd / _bwd / _bwd_bwd at the 4 x 4 maps the growing discriminator feeds them (n = 2 ... 64; 1 to 4 batched
  discriminator calls as groups; c = 256 padded to 264), every element against float64 autograd: u |ref| + 16 E32, first AND
  second order, in every storage type -- the second-order output of the 16-bit types included (a rel-L2 of 0.1 was all that
  stood there).  fp32 adds the derived conditioning term of elementwise.mbstd_conditioning (first needed by n = 2 over the
  emulated kernels: ratio 1.09 of u |ref| + 16 E32 at the one position whose two samples nearly coincide).  The copied
  channels are exact, the padding is zero.
  What this does NOT give at n = 2: E32 is one number per tensor, and the second-order gradient there spans orders of
  magnitude between positions (1 / sigma^3), so 16 E32 exceeds half of |ref| for most elements of gx2 at n = 2 -- that case
  guards against garbage, not against a wrong term; n >= 5 is where the second-order check bites.  A per-position E32
  (e32_bound takes an array) would close it and needs a restatement with more than two samples per position to be a bound."""
  from twingan_amd.params import mbstd_cpad
  from twingan_amd import _lib
  dtype = EW_DTYPES[dname]
  cpad = mbstd_cpad(c)
  eps = 1e-8 if dtype == torch.float32 else 1e-6
  rng = np.random.RandomState(400 + n + c)
  x, v = _round_to(rng.randn(n, 4, 4, c), dtype), _round_to(rng.randn(n, 4, 4, c), dtype)
  go = _round_to(rng.randn(n, 4, 4, cpad), dtype)
  xd = x.to(dev()).to(dtype).requires_grad_(True)
  god = go.to(dev()).to(dtype).requires_grad_(True)
  out = ops.minibatch_state_concat(xd, cpad, groups)
  gx, = torch.autograd.grad(out, xd, grad_outputs=god, create_graph=True)
  ggo, gx2 = torch.autograd.grad(gx, [god, xd], grad_outputs=v.to(dev()).to(dtype))
  r64 = E.mbstd_reference(x, go[..., :c + 1], v, groups, eps, torch.float64)
  r32 = E.mbstd_reference(x, go[..., :c + 1], v, groups, eps, torch.float32)
  o = host(out)
  assert np.array_equal(o[..., :c], x.numpy()) and np.all(o[..., c + 1:] == 0), 'mbstd copies x and pads with zeros'
  what = 'mbstd n%d g%d c%d %s ' % (n, groups, c, dname)
  gg = host(ggo)
  assert np.all(gg[..., c + 1:] == 0), what + 'second-order gradient of the padding'
  extra = {}
  if dtype == torch.float32:      # the derived term replaces nothing in 16-bit storage, where u |ref| + 16 E32 holds as it is
    ex_gx, ex_T, ex_gx2 = E.mbstd_conditioning(x, go, v, groups, eps)
    ex_ggo = np.zeros((n, 4, 4, c + 1))
    ex_ggo[..., c] = np.repeat(ex_T, n // groups).reshape(n, 1, 1)
    extra = {1: ex_gx, 2: ex_ggo, 3: ex_gx2}
  for nm, got, i in (('statistic', o[..., c:c + 1], 0), ('gx', host(gx), 1), ('ggo', gg[..., :c + 1], 2), ('gx2', host(gx2), 3)):
    ref = r64[i][..., c:c + 1] if i == 0 else r64[i]
    r32i = r32[i][..., c:c + 1] if i == 0 else r32[i]
    r = E.assert_elementwise(got, ref, E.e32_bound(ref, E.e32(r32i, ref), dtype) + extra.get(i, 0.0), what + nm)
    _ew_note('mbstd ' + nm, dname, r)
  if n % 3:
    with pytest.raises(_lib.TgError, match='not divisible by groups'):
      ops.minibatch_state_concat(xd.detach(), cpad, 3)


# ------------------------------------------------------------------------------------------------ fromRGB / toRGB, element by element
@pytest.mark.parametrize('dname', sorted(EW_DTYPES))
@pytest.mark.parametrize('cin,cout', [(3, 16), (3, 256), (16, 3), (256, 3), (3, 12), (20, 3)])
@pytest.mark.parametrize('n,h,w', [(3, 7, 5), (2, 33, 31)])      # 105 and 2046 pixels: no multiple of a block's pixel count
def test_pointwise_conv_elementwise(ops, n, h, w, cin, cout, dname):
  """tg_pointwise_conv_fwd (bias + LeakyReLU), its masked form, tg_pointwise_conv_bwd_weight(_bias) and the ordered form, with
  a pixel count that no block size divides.  Bounds as for the convs with K = cin: the weights hold values of the storage
  type, so 16-bit products are exact in fp32 (K + 2 operations with the epilogue); fp32 products round once each (2 K + 2).
  The masked form stores `rnd(x @ W) * mask`: the second rounding of the masked elements is named."""
  import twingan_amd.ops as O
  from twingan_amd._lib import TG_EPI_BIAS, TG_EPI_LRELU
  dtype = EW_DTYPES[dname]
  u_st = E.unit_roundoff(dtype)
  rng = np.random.RandomState(500 + cin + cout)
  x, gy = _round_to(rng.randn(n, h, w, cin), dtype), _round_to(rng.randn(n, h, w, cout), dtype)
  wt = _round_to(rng.randn(cin, cout) / np.sqrt(cin), dtype)
  b = torch.from_numpy((rng.randn(cout) * 0.1).astype(np.float32))
  xd, gyd = x.to(dev()).to(dtype).contiguous(), gy.to(dev()).to(dtype).contiguous()
  wd, bd = wt.float().to(dev()).contiguous(), b.to(dev())
  xn, wn, gn, bn = x.numpy(), wt.numpy(), gy.numpy(), b.double().numpy()
  K = cin if dtype != torch.float32 else 2 * cin
  lin, mag = xn @ wn, np.abs(xn) @ np.abs(wn)
  what = 'pointwise %d>%d n%d %dx%d %s ' % (cin, cout, n, h, w, dname)
  y = O._pw_fwd_raw(xd, wd, bd, False, TG_EPI_BIAS | TG_EPI_LRELU, 0.2)
  pre = lin + bn
  ref = np.where(pre > 0, pre, float(np.float32(0.2)) * pre)
  _ew_note('pointwise fwd', dname, E.assert_elementwise(host(y), ref, E.conv_bound(ref, mag + np.abs(bn), K + 2, dtype), what + 'fwd'))
  y0 = O._pw_fwd_raw(xd, wd, None, False, 0, 0.2)
  _ew_note('pointwise fwd', dname, E.assert_elementwise(host(y0), lin, E.conv_bound(lin, mag, K, dtype), what + 'fwd plain'))
  if cin <= 4:
    ym = O._pw_fwd_masked_raw(xd, wd, False, gyd, 0.2)
    slope = np.where(gn > 0, 1.0, float(np.float32(0.2)))
    ref = lin * slope
    extra = (1 + u_st) * u_st * np.abs(ref) * (slope != 1.0)
    _ew_note('pointwise fwd_masked', dname, E.assert_elementwise(host(ym), ref, E.conv_bound(ref, mag * slope, K + 1, dtype, extra),
                                                                 what + 'fwd_masked'))
  # filter (+ bias) gradient: fp32 sums over the pixels
  P = n * h * w
  ref_w = xn.reshape(-1, cin).T @ gn.reshape(-1, cout)
  mag_w = np.abs(xn).reshape(-1, cin).T @ np.abs(gn).reshape(-1, cout)
  ref_b, mag_b = gn.reshape(-1, cout).sum(axis=0), np.abs(gn).reshape(-1, cout).sum(axis=0)
  Pw = P if dtype != torch.float32 else 2 * P      # fp32 products round once each
  for acc in (0, 1):
    base = 3.0 if acc else 0.0
    addb = 2.0 ** -24 * (3.0 + np.abs(ref_w)) if acc else 0.0      # the addition into what the buffer held
    gw = torch.full((cin, cout), 3.0 if acc else float('nan'), device=dev())
    O.call('tg_pointwise_conv_bwd_weight', xd.data_ptr(), gyd.data_ptr(), gw.data_ptr(), P, cin, cout, acc, O._dt(xd), O._stream())
    _ew_note('pointwise bwd_weight', dname, E.assert_elementwise(host(gw) - base, ref_w, E.wgrad_bound(ref_w, mag_w, Pw) + addb,
                                                                 what + 'bwd_weight acc=%d' % acc))
    if cin <= 4:
      gw = torch.full((cin, cout), 3.0 if acc else float('nan'), device=dev())
      gb = torch.full((cout,), 3.0 if acc else float('nan'), device=dev())
      O.call('tg_pointwise_conv_bwd_weight_bias', xd.data_ptr(), gyd.data_ptr(), gw.data_ptr(), gb.data_ptr(), P, cin, cout, acc,
             O._dt(xd), O._stream())
      _ew_note('pointwise bwd_weight', dname, E.assert_elementwise(host(gw) - base, ref_w, E.wgrad_bound(ref_w, mag_w, Pw) + addb,
                                                                   what + 'bwd_weight_bias acc=%d' % acc))
      addbb = 2.0 ** -24 * (3.0 + np.abs(ref_b)) if acc else 0.0
      _ew_note('pointwise bias gradient', dname, E.assert_elementwise(host(gb) - base, ref_b, E.wgrad_bound(ref_b, mag_b, P) + addbb,
                                                                      what + 'bias gradient acc=%d' % acc))
    ws = torch.empty(256 * cin * cout, dtype=torch.float32, device=dev())
    gw = torch.full((cin, cout), 3.0 if acc else float('nan'), device=dev())
    O.call('tg_pointwise_conv_bwd_weight_ordered', xd.data_ptr(), gyd.data_ptr(), gw.data_ptr(), P, cin, cout, acc, ws.data_ptr(),
           ws.numel(), O._dt(xd), O._stream())
    _ew_note('pointwise bwd_weight_ordered', dname, E.assert_elementwise(
        host(gw) - base, ref_w, E.wgrad_bound(ref_w, mag_w, Pw) + addb, what + 'bwd_weight_ordered acc=%d' % acc))


# ------------------------------------------------------------------------------------------------ layer norm, conv statistics route
@pytest.mark.parametrize('dname', sorted(EW_DTYPES))
@pytest.mark.parametrize('n,h,w,c,pool,split', [(5, 17, 13, 8, False, None), (3, 34, 30, 16, True, 1), (4, 18, 22, 32, True, 4),
                                                (130, 8, 8, 16, False, 0)])
def test_layer_norm_act_elementwise(ops, n, h, w, c, pool, split, dname):
  """ops.layer_norm_act (statistics kernel + row arithmetic + the fused per-image-row kernel, and their backwards) at the tail
  shapes, every element against float64 autograd of the literal formula (moments of each image over (H, W, C), eps 1e-12)."""
  dtype = EW_DTYPES[dname]
  two = split is not None

  def refs(inp, dt, flip=None):
    y, gz, gzp, par = inp
    return E.norm_act_reference(y.to(dt), par[0], par[1], gz, par[2] if two else None, par[3] if two else None, split=split,
                                pool=pool, gzp=gzp, eps=1e-12, flip=flip, layer=True)
  inp, r64, r32, near = _seeded(lambda s: _norm_inputs(n, h, w, c, pool, dtype, s), refs, True, 600 + n)
  y, gz, gzp, par = inp
  yd = y.to(dev()).to(dtype).contiguous().requires_grad_(True)
  pd = [p.float().to(dev()).requires_grad_(True) for p in (par if two else par[:2])]
  out = ops.layer_norm_act(yd, pd[0], pd[1], pool=pool, gamma2=pd[2] if two else None, beta2=pd[3] if two else None, split=split)
  z, zp = out if pool else (out, None)
  if pool:
    torch.autograd.backward([z, zp], [gz.to(dev()).to(dtype), gzp.to(dev()).to(dtype)])
  else:
    z.backward(gz.to(dev()).to(dtype))
  what = 'layer_norm_act n%d %dx%d c%d %s' % (n, h, w, c, dname)
  # gy leaves this composition as the SUM of two stored tensors (the fused kernel's gy with the statistics held constant, and
  # the moments' backward), added by autograd in the storage type: three roundings, u (|direct| + |through the statistics|)
  # more than the one of a dedicated kernel
  direct = E.norm_act_reference(y.double(), par[0], par[1], gz, par[2] if two else None, par[3] if two else None, split=split,
                                pool=pool, gzp=gzp, eps=1e-12, layer=True, detach_stats=True)['gy'].numpy()
  u_st = E.unit_roundoff(dtype)
  extra = (1 + u_st) * (u_st * (np.abs(direct) + np.abs(r64['gy'].numpy() - direct)) + 2 * E.tiny(dtype))
  _check_norm_outputs(what, dname, dict(z=z, zp=zp, gy=yd.grad), r64, r32, dtype, 'layer_norm_act', near,
                      lambda f: refs(inp, torch.float64, f), gy_extra=extra)
  for i, nm in enumerate(('gamma', 'beta', 'gamma2', 'beta2')[:len(pd)]):
    ref = r64['grads'][i].numpy()
    if pd[i].grad is None:      # a domain without images (split 0 or n) receives no gradient at all
      assert not ref.any(), (what, nm)
      continue
    r = E.assert_elementwise(host(pd[i].grad), ref, E.e32_bound(ref, E.e32(r32['grads'][i].numpy(), ref), torch.float32),
                             '%s %s gradient' % (what, nm))
    _ew_note('layer_norm_act parameter grads', dname, r)


CONV_STATS_CASES = [
    # producer, n, hw (of the normalised tensor), cin (upcat: c0 = c1 = cin / 2), cout, pool
    ('conv', 5, 8, 256, 256, True),        # conv_img: ONE chunk per 8 x 8 image; norm_chunks cuts it in 4
    ('conv', 3, 16, 256, 256, False),      # tile kernel: 2 tiles per image against 8 chunks
    ('conv', 2, 16, 40, 24, True),         # ragged channel blocks, the scalar normaliser (no pixel norm at c = 24)
    ('conv', 3, 64, 64, 64, True),
    ('upcat', 4, 64, 64, 16, True),        # tg_conv2d_upcat_fwd_stats as the producer
    ('upcat', 3, 32, 128, 64, False),
]


@pytest.mark.parametrize('dname', ['bf16', 'f16'])
@pytest.mark.parametrize('producer,n,hw,cin,cout,pool', CONV_STATS_CASES)
def test_norm_act_fed_by_conv_statistics_elementwise(ops, producer, n, hw, cin, cout, pool, dname):
  """tg_norm_act_fwd_conv_stats: the normaliser's statistics come from the partial sums the conv's epilogue wrote -- the plain
  conv's (tg_conv2d_fwd_stats) and the upsample-concat conv's (tg_conv2d_upcat_fwd_stats) -- in the PRODUCER's chunking, which
  for every case here differs from norm_chunks' (asserted): z and the pooled z element by element against float64 on the
  tensor the conv stored.  A shape that loses its statistics epilogue fails here; it does not skip."""
  from twingan_amd import _lib
  dtype = EW_DTYPES[dname]
  g = torch.Generator().manual_seed(7)
  w = (torch.randn(3, 3, cin, cout, generator=g) * (2.0 / (9 * cin)) ** 0.5).to(dev())
  if producer == 'conv':
    x = (torch.randn(n, hw, hw, cin, generator=g) + 0.3).to(dtype).to(dev())
    y, st = ops.conv_fwd_stats_raw(x, w, ops.ConvSpec(3, 'SAME'))
  else:
    x0 = (torch.randn(n, hw // 2, hw // 2, cin // 2, generator=g) + 0.3).to(dtype).to(dev())
    x1 = torch.randn(n, hw, hw, cin // 2, generator=g).to(dtype).to(dev())
    assert ops.upcat_conv_supported(x0, x1, w)
    y, st = ops.upcat_conv_stats(x0, x1, w, 0, ())
  assert st is not None, 'no statistics epilogue for %s n%d hw%d c%d>%d %s' % (producer, n, hw, cin, cout, dname)
  own = _lib.load().tg_norm_chunks(n, hw, hw)
  assert own == _norm_chunking(n, hw * hw)[0][0]
  print('[conv stats] producer chunks %d, norm_chunks %d' % (st.chunks, own))
  assert st.chunks != own, ('the producer chunks this shape as norm_chunks does: the case no longer tests part_chunks', st.chunks, own)
  pn = cout % 8 == 0 and (cout // 8) & (cout // 8 - 1) == 0
  par = [torch.from_numpy((o + s * np.random.RandomState(8 + i).randn(cout)).astype(np.float32)) for i, (o, s) in
         enumerate(((1.0, 0.2), (0.0, 0.1)))]
  out = ops.norm_act(y, par[0].to(dev()), par[1].to(dev()), pixel_norm=pn, pool=pool, conv_stats=st)
  z, zp = out if pool else (out, None)
  yc = y.double().cpu()
  zero = torch.zeros(tuple(y.shape), dtype=torch.float64)
  zerop = torch.zeros((n, hw // 2, hw // 2, cout), dtype=torch.float64)
  r64, r32 = (E.norm_act_reference(yc.to(dt), par[0].double(), par[1].double(), zero, pixel_norm=pn, pool=pool, gzp=zerop)
              for dt in (torch.float64, torch.float32))
  what = 'norm_act conv_stats n%d hw%d c%d %s' % (n, hw, cout, dname)
  u_st = E.unit_roundoff(dtype)
  ref = r64['z'].numpy()
  _ew_note('norm_act conv_stats z', dname, E.assert_elementwise(host(z), ref, E.e32_bound(ref, E.e32(r32['z'].numpy(), ref), dtype),
                                                                what + ' z'))
  if pool:
    refp = r64['zp'].numpy()
    zmag = np.abs(ref).reshape(n, hw // 2, 2, hw // 2, 2, cout).mean(axis=(2, 4))
    bound = E.e32_bound(refp, E.e32(r32['zp'].numpy(), refp), dtype) + (1 + u_st) * u_st * zmag
    _ew_note('norm_act conv_stats zp', dname, E.assert_elementwise(host(zp), refp, bound, what + ' zp'))


# ===================================================================== attention, softmax, GEMM, losses, Adam: element-wise
# The derivations are in tests/elementwise.py (each count names the kernel operation it stands for); one line each:
#   flash forward    u |ref| + (1 + u) [((u + eps + len 2^-24) (mag + |ref|) + tiny16 (sum|v| + len |ref|)) / (1 - rho) + 2 2^-24 |ref|]
#                    eps = ((d_qk + 9) A + 2 + 3 len / 32) 2^-24, A = max_j |q_i| . |k_j|, mag = softmax(s) |v|
#   flash lse        -log(1 - rho) + 3 2^-24 (lse - max s + 6 + rho) + 2^-24 |lse|,   rho = u + eps + len 2^-24 + len tiny16
#   flash dQ dK dV   u |ref| + R u mag + A 2^-24 mag + 2^-25 S: P / dS packed, the forward's lse and O bounds carried in, A = len + d_v + 3
#   flash 2nd order  the same form over the four packed maps (P, gS, T, U); magnitudes: the closed form on |operands|, differences as sums
#   batched GEMM     conv_bound with K = k + 1 (alpha) + 1 (accumulate), mag = |alpha| |a| |b| + |C0|
#   softmax kernels  u |ref| + 16 E32, each kernel on the operands it reads
#   scalar sums      L 2^-24 |scale| sum|terms|, L from the launch geometry (trips, tail, tree, one add per workgroup)
#   Adam             one step in float64 from the fp32 state it reads, every fp32 operation counted once
FLASH_DTYPES = {'bf16': torch.bfloat16, 'f16': torch.float16}
FLASH_FWD_SHAPES = [(1, 128, 8, 64), (3, 256, 16, 64), (2, 384, 8, 128), (1, 256, 16, 128), (2, 128, 16, 256), (1, 384, 8, 256)]
FLASH_BWD_SHAPES = [(1, 128, 8, 64), (3, 256, 16, 64), (2, 384, 8, 128), (1, 256, 16, 128)]
FLASH_BB_SHAPES = [(1, 128, 8, 64), (2, 256, 16, 64), (1, 256, 8, 128), (2, 128, 16, 128)]
FLASH_FWD_CASES = [(f,) + s for s in FLASH_FWD_SHAPES for f in E.ATTENTION_FAMILIES] + \
    [(f, 1, 1024, 16, 128) for f in ('benign', 'ramp_up')]
FLASH_BWD_CASES = [(f,) + s for s in FLASH_BWD_SHAPES for f in E.ATTENTION_FAMILIES]
FLASH_BB_CASES = [(f,) + s for s in FLASH_BB_SHAPES for f in E.ATTENTION_FAMILIES]


def _r16(a, dtype):
  return bf16_round(a) if dtype == torch.bfloat16 else f16_round(a)


@functools.lru_cache(maxsize=None)
def _flash_inputs(family, n, ln, dk, dv, dname):
  """Operands of one case (float64 values of the storage type) and their float64 attention, computed once and shared by the
  forward, first-order and second-order tests; nobody writes to them."""
  dtype = FLASH_DTYPES[dname]
  rng = np.random.RandomState(zlib.crc32(('%s%d%d%d%d' % (family, n, ln, dk, dv)).encode()) % (2 ** 31))
  rnd = lambda a: _r16(a, dtype)
  q, k = E.attention_family(family, n, ln, dk, rng, rnd)
  v, go = rnd(rng.randn(n, ln, dv)), rnd(rng.randn(n, ln, dv))
  adj = tuple(rnd(rng.randn(n, ln, d)) for d in (dk, dk, dv))
  t = E.attention_terms(q, k, v)
  for a in (q, k, v, go) + adj + tuple(x for x in t.values()):
    a.setflags(write=False)
  return dict(q=q, k=k, v=v, go=go, adj=adj, t=t)


@pytest.mark.parametrize('dname', sorted(FLASH_DTYPES))
@pytest.mark.parametrize('family,n,ln,dk,dv', FLASH_FWD_CASES)
def test_flash_attention_forward_elementwise(ops, family, n, ln, dk, dv, dname):
  """tg_flash_attention_fwd on the eight score families (elementwise.attention_family: real rescales every block, a stale
  maximum with p > 1, lanes of one wave that disagree on `raise`, probabilities under the 16-bit pack's range, one rescale by
  e^80, saturated and uniform rows), every template instance, one / several loop trips and an odd number of 128-query
  workgroups: EVERY element of O and of lse inside its derived bound against float64 on the rounded operands; and each image
  of a batch bit-identical to the same image run alone (the img * d_v * len offsets of the packed V workspace)."""
  dtype = FLASH_DTYPES[dname]
  c = _flash_inputs(family, n, ln, dk, dv, dname)
  qd, kd, vd = (to_dev(c[x], dtype) for x in 'qkv')
  assert ops.flash_attention_supported(qd, vd)
  o, lse = ops.flash_attention_fwd_raw(qd, kd, vd)
  t = c['t']
  wo = E.assert_elementwise(host(o), t['o'], E.attention_fwd_bound(t, dk, dtype), 'flash O %s' % family)
  wl = E.assert_elementwise(host(lse), t['lse'], E.attention_lse_bound(t, dk, dtype), 'flash lse %s' % family)
  _ew_note('flash fwd O %s' % family, dname, wo)
  _ew_note('flash fwd lse %s' % family, dname, wl)
  for i in range(n if n > 1 else 0):
    o1, l1 = ops.flash_attention_fwd_raw(qd[i:i + 1].contiguous(), kd[i:i + 1].contiguous(), vd[i:i + 1].contiguous())
    assert torch.equal(o1[0], o[i]) and torch.equal(l1[0], lse[i]), 'image %d of %d differs from the same image alone' % (i, n)


@pytest.mark.parametrize('dname', sorted(FLASH_DTYPES))
@pytest.mark.parametrize('family,n,ln,dk,dv', FLASH_BWD_CASES)
def test_flash_attention_backward_elementwise(ops, family, n, ln, dk, dv, dname):
  """tg_flash_attention_bwd fed by the forward kernel's own O and lse (as in the product): every element of dQ, dK, dV inside
  elementwise.attention_bwd_bounds -- u_out |ref| + R u mag + A 2^-24 mag + 2^-25 S, the forward's lse and O bounds carried in
  as this kernel's input errors; rel-L2 says nothing here (a saturated row's gradient is 1e-29, an ill-conditioned row's
  cancels).  Batch independence as in the forward."""
  dtype = FLASH_DTYPES[dname]
  c = _flash_inputs(family, n, ln, dk, dv, dname)
  qd, kd, vd, gd = (to_dev(c[x], dtype) for x in ('q', 'k', 'v', 'go'))
  assert ops.flash_attention_trainable(qd, vd)
  o, lse = ops.flash_attention_fwd_raw(qd, kd, vd)
  got = ops._flash_bwd_raw(qd, kd, vd, o, lse, gd)
  r = E.attention_grads_reference(c['q'], c['k'], c['v'], c['go'], c['t'])
  bounds = E.attention_bwd_bounds(c['q'], c['k'], c['v'], c['go'], c['t'], r, dk, dtype)
  for g, nm, b in zip(got, ('dq', 'dk', 'dv'), bounds):
    _ew_note('flash bwd %s %s' % (nm, family), dname, E.assert_elementwise(host(g), r[nm], b, 'flash %s %s' % (nm, family)))
  for i in range(n if n > 1 else 0):
    sl = lambda x: x[i:i + 1].contiguous()
    o1, l1 = ops.flash_attention_fwd_raw(sl(qd), sl(kd), sl(vd))
    for g, g1 in zip(got, ops._flash_bwd_raw(sl(qd), sl(kd), sl(vd), o1, l1, sl(gd))):
      assert torch.equal(g1[0], g[i]), 'image %d of %d differs from the same image alone' % (i, n)


def _flash_second_order(ops, calls, dtype, q, k, v, go, aq, ak, av):
  """The four adjoints through the product's autograd path; the second-order pass must be the flash kernel's launch, not the
  batched-GEMM / softmax composition a cleared USE_FLASH_BWD_BWD would select."""
  qd, kd, vd, gd = (to_dev(x, dtype).requires_grad_(True) for x in (q, k, v, go))
  assert ops.USE_FLASH_BWD_BWD is True
  with ops.second_order():
    assert ops.flash_attention_trainable(qd, vd)
  o = ops.flash_attention(qd, kd, vd)
  gq, gk, gv = torch.autograd.grad(o, (qd, kd, vd), gd, create_graph=True)
  calls.clear()
  out = torch.autograd.grad((gq, gk, gv), (qd, kd, vd, gd), tuple(to_dev(x, dtype) for x in (aq, ak, av)))
  names = [c[0] for c in calls]
  assert names.count('tg_flash_attention_bwd_bwd') == 1, names
  assert not [x for x in names if x.startswith(('tg_batched_gemm', 'tg_softmax_rows'))], names
  return out


@pytest.mark.parametrize('dname', sorted(FLASH_DTYPES))
@pytest.mark.parametrize('family,n,ln,dk,dv', FLASH_BB_CASES)
def test_flash_attention_second_order_elementwise(ops, record_calls, family, n, ln, dk, dv, dname):
  """tg_flash_attention_bwd_bwd through the product's autograd path (create_graph backward, then its backward): every element of
  the four adjoints inside elementwise.attention_bwd_bwd_bounds against float64 autograd on the rounded operands, on every
  score family -- the saturated rows included, where the truth is 1e-29 and the kernel returns the fp32 noise of D against
  gP times |k| (the bound's (d_v + 3) 2^-24 dsa |K| term, derived there).  And each image of a batch bit-identical to the same
  image run alone (the per-image offsets of the packed workspaces and of the E / F statistics)."""
  dtype = FLASH_DTYPES[dname]
  c = _flash_inputs(family, n, ln, dk, dv, dname)
  ops_ = (c['q'], c['k'], c['v'], c['go']) + c['adj']
  got = _flash_second_order(ops, record_calls, dtype, *ops_)
  r = E.attention_grads_reference(c['q'], c['k'], c['v'], c['go'], c['t'])
  r['bb'] = _attention_second_order_ref(*ops_)
  bounds = E.attention_bwd_bwd_bounds(*ops_, c['t'], r, dk, dtype)
  for g, ref, b, nm in zip(got, r['bb'], bounds, ('adj q', 'adj k', 'adj v', 'adj dO')):
    _ew_note('flash bwd_bwd %s %s' % (nm, family), dname, E.assert_elementwise(host(g), ref, b, 'flash %s %s' % (nm, family)))
  for i in range(n if n > 1 else 0):
    alone = _flash_second_order(ops, record_calls, dtype, *(x[i:i + 1] for x in ops_))
    for g, g1, nm in zip(got, alone, ('adj q', 'adj k', 'adj v', 'adj dO')):
      assert torch.equal(g1[0], g[i]), '%s: image %d of %d differs from the same image alone' % (nm, i, n)


# ------------------------------------------------------------------------------------------------ batched GEMM
BGEMM_EW_CASES = BGEMM_CASES + [(2, 136, 72, 40), (2, 264, 200, 72), (1, 8, 8, 8)]      # 16-byte staging with ragged m, n, k tiles


def _round_dt(a, dtype):
  return a.astype(np.float32).astype(np.float64) if dtype == torch.float32 else _r16(a, dtype)


@pytest.mark.parametrize('dname', sorted(EW_DTYPES))
@pytest.mark.parametrize('batch,m,n,k', BGEMM_EW_CASES)
def test_batched_gemm_elementwise(ops, batch, m, n, k, dname):
  """tg_batched_gemm, all four layouts: every element inside conv_bound with K = k + 1 (the alpha multiply).  The last three
  cases are eligible for the 16-byte vector staging (every extent a multiple of 8) AND ragged in m, n and k."""
  dtype = EW_DTYPES[dname]
  rng = np.random.RandomState(zlib.crc32(('bg%d%d%d%d' % (batch, m, n, k)).encode()) % (2 ** 31))
  for ta in (False, True):
    for tb in (False, True):
      a = _round_dt(rng.randn(batch, k, m) if ta else rng.randn(batch, m, k), dtype)
      b = _round_dt(rng.randn(batch, n, k) if tb else rng.randn(batch, k, n), dtype)
      oa, ob = (a.transpose(0, 2, 1) if ta else a), (b.transpose(0, 2, 1) if tb else b)
      ref, mag = 0.5 * np.matmul(oa, ob), 0.5 * np.matmul(np.abs(oa), np.abs(ob))
      c = ops.bgemm(to_dev(a, dtype), to_dev(b, dtype), ta, tb, 0.5)
      w = E.assert_elementwise(host(c), ref, E.gemm_bound(ref, mag, k, dtype), 'bgemm ta=%d tb=%d' % (ta, tb))
      _ew_note('batched gemm', dname, w)


@pytest.mark.parametrize('dname,c_f32', [('f32', 0), ('bf16', 0), ('bf16', 1), ('f16', 0), ('f16', 1)])
@pytest.mark.parametrize('pad', [8, 3])
@pytest.mark.parametrize('batch,m,n,k', [(2, 136, 72, 40), (1, 8, 8, 8)])
def test_batched_gemm_c_abi_strides_accumulate_and_f32_output(ops, batch, m, n, k, pad, dname, c_f32):
  """What include/twingan_hip.h declares and ops.bgemm never passes: accumulate = 1 onto a non-zero C, c_is_f32 = 1 from 16-bit
  operands, lda / ldb / ldc and batch strides larger than dense (pad 8 keeps the 16-byte staging, pad 3 forces the scalar one).
  The padding of A and B holds NaN (a kernel that reads it shows), the padding columns, rows and the spare batch slot of C a
  sentinel that must come back bit-identical."""
  import twingan_amd.ops as O
  dtype = EW_DTYPES[dname]
  cdt = torch.float32 if c_f32 else dtype
  rng = np.random.RandomState(zlib.crc32(('abi%d%d%d%d%d' % (batch, m, n, k, pad)).encode()) % (2 ** 31))
  st = torch.cuda.current_stream().cuda_stream
  for ta in (0, 1):
    for tb in (0, 1):
      (ra, ca), (rb, cb) = ((k, m) if ta else (m, k)), ((n, k) if tb else (k, n))
      a, b = _round_dt(rng.randn(batch, ra, ca), dtype), _round_dt(rng.randn(batch, rb, cb), dtype)
      c0 = _round_dt(rng.randn(batch, m, n), cdt)
      A = torch.full((batch, ra + 2, ca + pad), float('nan'), dtype=dtype, device=dev())
      B = torch.full((batch, rb + 2, cb + pad), float('nan'), dtype=dtype, device=dev())
      C = torch.full((batch + 1, m + 1, n + pad), -7.25, dtype=cdt, device=dev())
      A[:, :ra, :ca], B[:, :rb, :cb], C[:batch, :m, :n] = to_dev(a, dtype), to_dev(b, dtype), to_dev(c0, cdt)
      before = C.clone()
      O.call('tg_batched_gemm', A.data_ptr(), B.data_ptr(), C.data_ptr(), batch, m, n, k, ta, tb, ca + pad, cb + pad, n + pad,
             (ra + 2) * (ca + pad), (rb + 2) * (cb + pad), (m + 1) * (n + pad), -0.75, 1, O._dt(A), c_f32, st)
      oa, ob = (a.transpose(0, 2, 1) if ta else a), (b.transpose(0, 2, 1) if tb else b)
      ref = -0.75 * np.matmul(oa, ob) + c0
      bound = E.gemm_bound(ref, 0.75 * np.matmul(np.abs(oa), np.abs(ob)), k, dtype, c0=c0, c_f32=bool(c_f32))
      w = E.assert_elementwise(host(C[:batch, :m, :n]), ref, bound, 'bgemm C ABI ta=%d tb=%d pad=%d' % (ta, tb, pad))
      _ew_note('batched gemm C ABI', dname + ('>f32' if c_f32 else ''), w)
      keep = torch.ones_like(C, dtype=torch.bool)
      keep[:batch, :m, :n] = False
      bits = torch.int32 if cdt == torch.float32 else torch.int16
      assert torch.equal(C.view(bits)[keep], before.view(bits)[keep]), 'the padding of C changed (ta=%d tb=%d)' % (ta, tb)


# ------------------------------------------------------------------------------------------------ row softmax
@pytest.mark.parametrize('dname', sorted(EW_DTYPES))
@pytest.mark.parametrize('cols', [1, 63, 64, 100, 255, 256, 257, 4096, 4100])
def test_softmax_kernels_elementwise(ops, cols, dname):
  """tg_softmax_rows_fwd / _bwd / _bwd_bwd, five rows: scores scaled to a row range of about 4, 40 and 160 (the last under both
  16-bit types' range), one all-equal row, one row of values about -1e4 (fp32; a plain row in 16 bit) -- one thread's worth of
  columns, a partial wave, exactly / one more than a block, many trips with a tail.  Each kernel on the operands it reads
  (the backwards take the stored p), every element inside u |ref| + 16 E32, E32 taken PER ROW: the absolute term of a row is
  set by that row's own largest element, not by the largest of the five, so the small probabilities of the range-40 and
  range-160 rows are not judged against the uniform row's scale."""
  import twingan_amd.ops as O
  dtype = EW_DTYPES[dname]
  rng = np.random.RandomState(500 + cols)
  s = rng.randn(5, cols)
  for r, rg in enumerate((4.0, 40.0, 160.0)):
    s[r] *= rg / max(np.ptp(s[r]), 1e-30) if cols > 1 else 1.0
  s[3] = s[3, 0]
  if dtype == torch.float32:
    s[4] = -1e4 + s[4]
  s = _round_dt(s, dtype)
  dp, v = _round_dt(rng.randn(5, cols), dtype), _round_dt(rng.randn(5, cols), dtype)
  p_in = _round_dt(E.softmax_kernels_reference(s, s, dp, v, np.float64)[0], dtype)      # the stored p the backwards read
  r64 = E.softmax_kernels_reference(s, p_in, dp, v, np.float64)
  r32 = E.softmax_kernels_reference(s, p_in, dp, v, np.float32)
  sd, pd, dpd, vd = (to_dev(x, dtype) for x in (s, p_in, dp, v))
  out = [torch.empty_like(sd) for _ in range(3)]
  st, dt = torch.cuda.current_stream().cuda_stream, O._dt(sd)
  O.call('tg_softmax_rows_fwd', sd.data_ptr(), out[0].data_ptr(), 5, cols, dt, st)
  O.call('tg_softmax_rows_bwd', pd.data_ptr(), dpd.data_ptr(), out[1].data_ptr(), 5, cols, dt, st)
  O.call('tg_softmax_rows_bwd_bwd', pd.data_ptr(), dpd.data_ptr(), vd.data_ptr(), out[2].data_ptr(), 5, cols, dt, st)
  for got, a64, a32, nm in zip(out, r64, r32, ('fwd', 'bwd', 'bwd_bwd')):
    e32_row = np.abs(a32.astype(np.float64) - a64).max(-1, keepdims=True)
    w = E.assert_elementwise(host(got), a64, E.e32_bound(a64, e32_row, dtype), 'softmax %s cols %d' % (nm, cols))
    _ew_note('softmax ' + nm, dname, w)


# ------------------------------------------------------------------------------------------------ losses
LOSS_SHAPES = [(1, 1, 1, 1), (2, 5, 5, 3), (3, 5, 5, 3), (1, 4099, 1, 1), (16, 256, 256, 3)]
LOSS_BIG = 16 * 256 * 256 * 3


def _spike_positions(numel, dtype):
  """The elements a broken index would drop or double: the first and last element, the vector tail, and the first and last
  element of every workgroup's 256 vectors in every grid-stride trip (a trip is a whole number of workgroups, so these are the
  same positions at every workgroup cap) -- of its 256 ELEMENTS where the length is no multiple of the vector width, the case
  in which a per-sample sum takes the scalar loop."""
  V = 4 if dtype == torch.float32 else 8
  nvec = numel // V
  first, efirst = np.arange(0, nvec, 256), np.arange(0, numel if numel % V else 0, 256)
  idx = np.unique(np.concatenate([np.array([0, numel - 1]), np.arange(nvec * V, numel), first * V,
                                  np.minimum(first + 255, max(nvec - 1, 0)) * V + V - 1, efirst, efirst + 255]))
  return idx[(idx >= 0) & (idx < numel)]


def _spiked(rng, shape, dtype, per_sample=False, scale=1.0):
  """Values in +-[0.5, 1) * scale with the elements of _spike_positions 1e3 times that (per sample for the per-sample sums)."""
  x = (0.5 + 0.5 * rng.rand(*shape)) * np.where(rng.rand(*shape) < 0.5, -1.0, 1.0) * scale
  flat = x.reshape(shape[0], -1) if per_sample else x.reshape(1, -1)
  flat[:, _spike_positions(flat.shape[1], dtype)] *= 1e3
  return _round_dt(x, dtype)


@pytest.mark.parametrize('ordered', [False, True], ids=['plain', 'ordered'])
@pytest.mark.parametrize('dname', sorted(EW_DTYPES))
@pytest.mark.parametrize('shape', LOSS_SHAPES, ids=['x'.join(map(str, s)) for s in LOSS_SHAPES])
def test_loss_reductions_elementwise(ops, shape, dname, ordered):
  """abs_diff_mean, mean and gradient_penalty at 1, 150, 225 (per = 75 with batch 3: samples that do not start on a 16-byte
  boundary), 4099 (a vector tail) and 16 x 256 x 256 x 3 elements (more than one grid-stride trip at every workgroup cap: 1024
  plain, 512 ordered, 64 per sample), in the plain route and the deterministic() ordered one.  The data is spiked where an
  index fault would bite (_spike_positions).  Forward: |got - ref| <= L 2^-24 |scale| sum|terms| with L from the launch geometry;
  gradients element by element; the ordered route twice, bit-identical."""
  from twingan_amd import _lib
  lib = _lib.load()
  dtype = EW_DTYPES[dname]
  numel = int(np.prod(shape))
  rng = np.random.RandomState(numel % 9973 + 17 * ordered)
  u = E.unit_roundoff(dtype)
  # the geometry each route launches (csrc/reduce.hip, ops._scalar_sum_into): tg_sum / tg_abs_diff_sum cap 1024 and ONE workgroup
  # for fp32; tg_sum_ordered cap 512 for every type; tg_sample_sumsq cap 64, one workgroup for fp32 and in deterministic mode
  geo = (512, False) if ordered else (1024, None)
  a = _spiked(rng, shape, dtype)
  b = _round_dt(0.5 + 0.5 * rng.rand(*shape), dtype)
  per = numel // shape[0]
  g = _spiked(rng, shape, dtype, per_sample=True, scale=1.0 / np.sqrt(per))
  was = lib.tg_set_deterministic(1 if ordered else 0)
  try:
    assert ops.deterministic() == ordered
    runs = []
    for _ in range(2 if ordered else 1):
      ad, bd, gd = (to_dev(x, dtype).requires_grad_(True) for x in (a, b, g))
      l1, l2, l3 = ops.abs_diff_mean(ad, bd, 0.1), ops.mean(ad, -1.0), ops.gradient_penalty(gd, 10.0)
      (l1 * 3.0 + l2 * 0.5 + l3 * 2.0).backward()
      runs.append((l1.clone(), l2.clone(), l3.clone(), ad.grad.clone(), bd.grad.clone(), gd.grad.clone()))
    if ordered:
      for x, y in zip(*runs):
        assert torch.equal(x, y), 'the ordered route differs between two runs'
  finally:
    lib.tg_set_deterministic(was)
  l1, l2, l3, ga, gb, gg = runs[0]
  L, _ = E.reduction_chain(numel, dtype, geo[0], one_block=geo[1])
  # abs_diff_mean: terms |a - b| (one fp32 subtraction each)
  terms = np.abs(a - b)
  bnd = E.reduction_bound(terms.sum(), L, 0.1 / numel, term_ops=1)
  r1 = abs(l1.item() - 0.1 * terms.sum() / numel) / bnd
  bnd2 = E.reduction_bound(np.abs(a).sum(), L, 1.0 / numel)
  r2 = abs(l2.item() + a.sum() / numel) / bnd2
  print('[loss sums] %s %s numel %d: L %d, ratios abs_diff %.3f mean %.3f' % (dname, 'ordered' if ordered else 'plain', numel, L, r1, r2))
  assert r1 <= 1.0 and r2 <= 1.0, (r1, r2)
  _ew_note('loss sums ' + ('ordered' if ordered else 'plain'), dname, max(r1, r2))
  if numel > 1:
    # the test's own power: ONE spiked element dropped or doubled moves either sum by more than its bound (the exception: the
    # fp32 plain route sums 3 M elements in ONE workgroup, a chain of 12 K additions whose worst case exceeds one spike)
    # -- there a single-element index fault of the fp32 plain route is NOT detectable by the sum; the 16-bit types and the ordered
    # route, which run the same sum_kernel template over the same indices, are what pins its indexing at that size).  The
    # same for |a - b|, whose spiked terms are at least |a| - 1
    spike = np.abs(a).max() / 2.0 / numel
    spike1 = 0.1 * (np.abs(a).max() - 1.0) / 2.0 / numel
    assert (spike > bnd2 and spike1 > bnd) or (dname == 'f32' and not ordered and numel == LOSS_BIG), (spike, bnd2, spike1, bnd)
  # gradients: 3 k sign(a - b) and 0.5 k': the weight as a C float, its product with the incoming gradient, then the store
  # (3 2^-24 + u of each term); a's gradient is the stored sum of its two stored terms (u of the sum)
  sgn, t1, t2 = np.sign(a - b), 0.3 / numel, 0.5 / numel
  one = lambda m: (u + 3 * E.U32) * m + E.tiny(dtype)
  ra = t1 * sgn - t2
  _ew_note('loss gradients', dname, E.assert_elementwise(host(ga).reshape(shape), ra, one(t1) + one(t2) + u * np.abs(ra) + E.tiny(dtype),
                                                         'abs_diff_mean + mean, d a'))
  _ew_note('loss gradients', dname, E.assert_elementwise(host(gb).reshape(shape), -t1 * sgn, one(t1), 'abs_diff_mean, d b'))
  # gradient penalty: per-sample sums of squares (an fmaf per term), the scalar tail, coef[b] x g
  Ls, _ = E.reduction_chain(per, dtype, 64, vec=(shape[0] == 1 or per % (4 if dtype == torch.float32 else 8) == 0),
                            one_block=True if ordered else None)
  ss = (g.reshape(shape[0], -1) ** 2).sum(1)
  (loss, coef), (b_loss, b_coef) = E.gp_penalty_bounds(ss, Ls, 10.0)
  r3 = abs(l3.item() - loss) / b_loss
  print('[loss sums] gradient penalty: L %d ratio %.3f' % (Ls, r3))
  assert r3 <= 1.0, (l3.item(), loss, b_loss)
  _ew_note('gradient penalty', dname, r3)
  cb = (1,) * (len(shape) - 1)
  ref = 2.0 * coef.reshape((-1,) + cb) * g
  bound = 2.0 * b_coef.reshape((-1,) + cb) * np.abs(g) + (u + 3 * E.U32) * np.abs(ref) + E.tiny(dtype)
  _ew_note('gradient penalty grad', dname, E.assert_elementwise(host(gg).reshape(shape), ref, bound, 'gradient penalty d g'))


@pytest.mark.parametrize('ordered', [False, True], ids=['plain', 'ordered'])
@pytest.mark.parametrize('dname', sorted(EW_DTYPES))
@pytest.mark.parametrize('numel', [1, 4099, 300001])
def test_loss_sums_of_a_view_off_the_16_byte_boundary(ops, numel, dname, ordered):
  """mean and abs_diff_mean of contiguous views that start ONE element into their buffers (_chk asks for contiguity only): the
  base pointers of tg_sum, tg_abs_diff_sum and tg_sum_ordered are then 2 or 4 bytes off a 16-byte boundary, and the entry
  points must send every element through the scalar loop (sum_kernel's vec = 0) -- reduction_chain(vec=False) is the chain
  that launch has.  One element, several workgroups, and 300001 elements (several grid-stride trips of the scalar loop).
  Also a alone off the boundary with b on it: the condition is on BOTH operands.  abs_diff_mean's gradients element-wise."""
  from twingan_amd import _lib
  lib = _lib.load()
  dtype = EW_DTYPES[dname]
  rng = np.random.RandomState(numel % 9973 + 31 * ordered)
  u = E.unit_roundoff(dtype)
  a = _spiked(rng, (numel,), dtype)
  b = _round_dt(0.5 + 0.5 * rng.rand(numel), dtype)
  abuf, bbuf = (torch.full((numel + 1,), float('nan'), dtype=dtype, device=dev()) for _ in range(2))
  abuf[1:], bbuf[1:] = to_dev(a, dtype), to_dev(b, dtype)
  av, bv, b0 = abuf[1:].requires_grad_(True), bbuf[1:].requires_grad_(True), to_dev(b, dtype)
  assert av.is_contiguous() and av.data_ptr() % 16 != 0 and bv.data_ptr() % 16 != 0 and b0.data_ptr() % 16 == 0
  was = lib.tg_set_deterministic(1 if ordered else 0)
  try:
    runs = []
    for _ in range(2 if ordered else 1):
      l1, l2, l4 = ops.abs_diff_mean(av, bv, 0.1), ops.mean(av, -1.0), ops.abs_diff_mean(av, b0, 0.1)
      ga, gb = torch.autograd.grad(l1 * 3.0, (av, bv))
      runs.append((l1.clone(), l2.clone(), l4.clone(), ga, gb))
    if ordered:
      for x, y in zip(*runs):
        assert torch.equal(x, y), 'the ordered route differs between two runs'
  finally:
    lib.tg_set_deterministic(was)
  l1, l2, l4, ga, gb = runs[0]
  L, _ = E.reduction_chain(numel, dtype, 512 if ordered else 1024, vec=False, one_block=False if ordered else None)
  terms = np.abs(a - b)
  bnd1 = E.reduction_bound(terms.sum(), L, 0.1 / numel, term_ops=1)
  bnd2 = E.reduction_bound(np.abs(a).sum(), L, 1.0 / numel)
  r1 = abs(l1.item() - 0.1 * terms.sum() / numel) / bnd1
  r4 = abs(l4.item() - 0.1 * terms.sum() / numel) / bnd1
  r2 = abs(l2.item() + a.sum() / numel) / bnd2
  print('[loss sums] unaligned %s %s numel %d: L %d, ratios abs_diff %.3f (a alone off: %.3f) mean %.3f'
        % (dname, 'ordered' if ordered else 'plain', numel, L, r1, r4, r2))
  assert r1 <= 1.0 and r2 <= 1.0 and r4 <= 1.0, (r1, r2, r4)
  _ew_note('loss sums unaligned ' + ('ordered' if ordered else 'plain'), dname, max(r1, r2, r4))
  if numel > 1:      # one spiked element dropped or doubled moves either sum by more than its bound
    spike = np.abs(a).max() / 2.0
    assert spike / numel > bnd2 and 0.1 * spike / numel > bnd1, (spike, bnd1, bnd2)
  sgn, t1 = np.sign(a - b), 0.3 / numel
  one = (u + 3 * E.U32) * t1 + E.tiny(dtype)
  E.assert_elementwise(host(ga), t1 * sgn, one, 'abs_diff_mean of views, d a')
  E.assert_elementwise(host(gb), -t1 * sgn, one, 'abs_diff_mean of views, d b')
  assert bool(torch.isnan(abuf[0])) and bool(torch.isnan(bbuf[0]))


@pytest.mark.parametrize('dname', sorted(EW_DTYPES))
def test_gradient_penalty_of_an_all_zero_sample(ops, dname):
  """One all-zero sample in the batch: slope = 0, where the literal formula's gradient 2 lambda (slope - 1) g / (slope batch)
  is 0 / 0.  The kernel's `slope > 0` guard makes that sample's coefficient -- and gradient -- 0: loss
  and gradient finite, the loss counts (0 - 1)^2 for the sample, its gradient is exactly 0, the others' are right."""
  dtype = EW_DTYPES[dname]
  rng = np.random.RandomState(77)
  g = _round_dt(rng.randn(3, 5, 5, 3) * 0.1, dtype)
  g[1] = 0.0
  gd = to_dev(g, dtype).requires_grad_(True)
  l = ops.gradient_penalty(gd, 10.0)
  l.backward()
  gr = host(gd.grad)
  assert np.isfinite(l.item()) and np.all(np.isfinite(gr)) and np.all(gr[1] == 0.0)
  L, _ = E.reduction_chain(75, dtype, 64, vec=False)
  (loss, coef), (b_loss, b_coef) = E.gp_penalty_bounds((g.reshape(3, -1) ** 2).sum(1), L, 10.0)
  assert coef[1] == 0.0 and abs(l.item() - loss) <= b_loss
  ref = coef.reshape(3, 1, 1, 1) * g
  bound = b_coef.reshape(3, 1, 1, 1) * np.abs(g) + (E.unit_roundoff(dtype) + 3 * E.U32) * np.abs(ref) + E.tiny(dtype)
  E.assert_elementwise(gr, ref, bound, 'gradient penalty with a zero sample')


# ------------------------------------------------------------------------------------------------ Adam
@pytest.mark.parametrize('numel', [1, 255, 257, 5000000])
def test_adam_step_elementwise(numel):
  """tg_adam_tick + tg_adam_step, ten steps: grad_scale = 1 / 1024 on gradients multiplied by 1024, the rate read from the device
  pointer, a shadow buffer; elements with g = 0 throughout, |g| = 1e4, |g| = 1e-20 (v is subnormal in fp32), theta = 0 (where
  nothing hides the update behind theta's own rounding).  After EVERY step theta, m and v are inside the bounds of
  elementwise.adam_step_bounds -- one step in float64 from the fp32 state the launch read -- and the shadow equals the
  round-to-nearest-even bfloat16 of the theta the kernel stored, bit for bit.  One element, a partial / just over one
  workgroup, and 5 M elements (more than the 4096-workgroup cap: the grid-stride loop)."""
  from twingan_amd._lib import call
  gen = torch.Generator().manual_seed(numel % 1000)
  ar = torch.arange(numel)
  kind = ar % 4
  scale = torch.where(kind == 1, 1e4, torch.where(kind == 2, 1e-20, torch.where(kind == 3, 0.0, 1.0))).double()
  th0 = torch.randn(numel, generator=gen)
  th0[ar % 8 == 0] = 0.0
  thd, md, vd = th0.to(dev()), torch.zeros(numel, device=dev()), torch.zeros(numel, device=dev())
  shadow = torch.full((numel,), 7.0, dtype=torch.bfloat16, device=dev())
  step = torch.zeros(1, dtype=torch.int64, device=dev())
  lr_t = torch.zeros(1, dtype=torch.float32, device=dev())
  st = torch.cuda.current_stream().cuda_stream
  worst = [0.0, 0.0, 0.0]
  for t in range(1, 11):
    gdev = (torch.randn(numel, generator=gen).double() * scale * 1024.0).float().to(dev())
    prev = [x.double().cpu().numpy() for x in (thd, gdev, md, vd)]
    call('tg_adam_tick', step.data_ptr(), lr_t.data_ptr(), 1e-4, 0.5, 0.99, st)
    call('tg_adam_step', thd.data_ptr(), gdev.data_ptr(), md.data_ptr(), vd.data_ptr(), shadow.data_ptr(), numel, 0.0,
         lr_t.data_ptr(), 0.5, 0.99, 1e-8, 1.0 / 1024.0, st)
    assert int(step.item()) == t
    want_lr = 1e-4 * np.sqrt(1 - float(np.float32(0.99)) ** t) / (1 - 0.5 ** t)
    assert abs(lr_t.item() - want_lr) <= 2 * E.U32 * want_lr
    refs, bounds = E.adam_step_bounds(*prev, lr_t.item(), 0.5, 0.99, 1e-8, 1.0 / 1024.0)
    for i, (got, nm) in enumerate(((thd, 'theta'), (md, 'm'), (vd, 'v'))):
      worst[i] = max(worst[i], E.assert_elementwise(got.double().cpu().numpy(), refs[i], bounds[i], 'adam %s step %d' % (nm, t)))
    assert torch.equal(shadow.view(torch.int16), thd.to(torch.bfloat16).view(torch.int16)), 'shadow != bf16(theta) at step %d' % t
  if numel >= 255:
    assert bool((md[kind.to(dev()) == 3] == 0).all()) and bool((thd[kind.to(dev()) == 3] == th0.to(dev())[kind.to(dev()) == 3]).all())
  for w, nm in zip(worst, ('theta', 'm', 'v')):
    _ew_note('adam ' + nm, 'f32', w)


# ------------------------------------------------------------------------------------------------ spectral norm
SN_OLD_SHAPES = [(3, 3, 16, 32), (1, 1, 3, 16), (4, 4, 64, 64), (3, 3, 264, 256), (3, 3, 5, 7)]
SN_SHAPES = [(1, 1, 1, 1), (1, 1, 1, 5), (1, 1, 5, 1), (1, 1, 2, 64), (1, 1, 15, 65), (1, 1, 17, 63), (4, 4, 16, 1), (1, 1, 4096, 1),
             (3, 3, 7, 129), (3, 3, 8, 257), (1, 1, 64, 300), (3, 3, 16, 512), (1, 1, 16, 1023), (1, 1, 33, 1024), (1, 1, 1025, 3)] + SN_OLD_SHAPES
SN_STATES = [(1e-4, 'random'), (0.1, 'random'), (30.0, 'random'), (1e-4, 'converged'), (0.1, 'converged'), (30.0, 'converged'),
             (0.1, 'rank1')]
_SN_ID = lambda sh: 'x'.join(map(str, sh))


def _sn_power(w2, u, iters):
  l2n = lambda x: x / x.pow(2).sum().clamp_min(1e-12).sqrt()
  for _ in range(iters):
    u = l2n(l2n(u @ w2.t()) @ w2)
  return u


def _sn_inputs(shape, scale, kind, salt=0):
  """-> (w [kh, kw, cin, cout], u [1, cout], G like w) as float32 CPU tensors.  random: w ~ scale N(0, 1) (1e-4, 0.1, and 30 --
  the equalised-learning-rate kernels are N(0, 1)), u ~ N(0, 1); converged: u after 30 float64 power iterations (b ~ 0: the
  v (x) u' term carries the gradient); rank1: w = scale (p (x) q + 1e-3 N(0, 1)), nearly degenerate.  The seed of a case is the
  first for which the float64 norms |u W^T| and |v W| are at least 1e-5, ten times l2_normalize's clamp: the clamped branch is
  not what the backward's closed form differentiates (from the inputs alone, as _seeded does for the normalisers)."""
  cout = shape[3]
  k_rows = shape[0] * shape[1] * shape[2]
  base = zlib.crc32(('sn%s%g%s%d' % (shape, scale, kind, salt)).encode()) % (2 ** 31 - 64)
  for seed in range(base, base + 64):
    g = torch.Generator().manual_seed(seed)
    if kind == 'rank1':
      w2 = scale * (torch.randn(k_rows, 1, generator=g, dtype=torch.float64) * torch.randn(1, cout, generator=g, dtype=torch.float64)
                    + 1e-3 * torch.randn(k_rows, cout, generator=g, dtype=torch.float64))
    else:
      w2 = scale * torch.randn(k_rows, cout, generator=g, dtype=torch.float64)
    w2 = w2.float()
    u = torch.randn(1, cout, generator=g, dtype=torch.float64)
    if kind == 'converged':
      u = _sn_power(w2.double(), u, 30)
    u = u.float()
    G = torch.randn(k_rows, cout, generator=g, dtype=torch.float64).float()
    v_raw = u.double() @ w2.double().t()
    u_raw = (v_raw / v_raw.norm()) @ w2.double()
    if float(v_raw.norm()) >= 1e-5 and float(u_raw.norm()) >= 1e-5:
      return w2.reshape(shape), u, G.reshape(shape)
  raise AssertionError('no seed keeps %s %g %s off the clamp' % (shape, scale, kind))


def _sn_run(ops, w, u, G):
  """ops.spectral_norm forward + backward on the device -> dict(w_bar, u_new, v, stats, gw) as float64 numpy, plus u_new on the device."""
  wd = w.clone().to(dev()).requires_grad_(True)
  w_bar, u_new = ops.spectral_norm(wd, u.clone().to(dev()))
  _, _, _, v, stats = w_bar.grad_fn.saved_tensors
  (w_bar * G.to(dev())).sum().backward()
  k_rows = w.numel() // w.shape[-1]
  return dict(w_bar=host(w_bar).reshape(k_rows, -1), u_new=host(u_new).reshape(-1), v=host(v), stats=host(stats),
              gw=host(wd.grad).reshape(k_rows, -1)), u_new.detach()


def _sn_check(what, got, ref, bound):
  for key in ('w_bar', 'u_new', 'v', 'stats', 'gw'):
    if key in got:
      _ew_note('spectral norm ' + key, 'f32', E.assert_elementwise(got[key], ref[key], bound[key], '%s %s' % (what, key)))


@pytest.mark.parametrize('shape', SN_SHAPES, ids=_SN_ID)
def test_spectral_norm_elementwise(ops, shape):
  """tg_spectral_norm_fwd / _bwd, every element of w_bar, u', the saved v and stats = {sigma, |v_raw|}, and d L / d w inside
  elementwise.sn_bounds, against float64 autograd of the literal formulas.  Shapes: a 1 x 1 matrix, one row, one column
  (cout = 1: a prediction layer), k_rows on both sides of ROWS = KS = 16, K = 4096 and 1025 rows on a thin matrix, cout across
  64, 128, 256 (where sn_finish's ur[4] loop takes its second, third and fourth trip), 512 and the documented limit of 1024;
  the five shapes test_spectral_norm_matches_oracle has.  States: weight scales 1e-4 / 0.1 / 30, u random and converged
  (b ~ 0), one nearly rank-1 matrix."""
  k_rows, cout = shape[0] * shape[1] * shape[2], shape[3]
  for scale, kind in SN_STATES:
    w, u, G = _sn_inputs(shape, scale, kind)
    got, _ = _sn_run(ops, w, u, G)
    ref, bound = E.sn_bounds(w.reshape(k_rows, cout), u, G.reshape(k_rows, cout))
    _sn_check('sn %s %g %s' % (_SN_ID(shape), scale, kind), got, ref, bound)
  # one more state: w ~ 1e-8 N(0, 1) / sqrt(K cout) (|u W^T| ~ 1e-8), where BOTH l2_normalize clamps are active (|u W^T|^2 and |v W|^2 < 1e-12; v =
  # v_raw 1e6, stats[1] = 1e-6).  Forward outputs and the saved v / stats only: a stats[1] left unclamped shows nowhere else, and
  # the backward's closed form differentiates the unclamped normalisation, so its gradient is not asked here
  g = torch.Generator().manual_seed(k_rows * 7 + cout)
  w = (1e-8 / (k_rows * cout) ** 0.5 * torch.randn(shape, generator=g, dtype=torch.float64)).float()
  u, G = torch.randn(1, cout, generator=g), torch.randn(shape, generator=g)
  assert float((u.double() @ w.double().reshape(k_rows, cout).t()).norm()) < 1e-7
  got, _ = _sn_run(ops, w, u, G)
  ref, bound = E.sn_bounds(w.reshape(k_rows, cout), u, G.reshape(k_rows, cout))
  assert ref['stats'][1] == 1e-6
  del got['gw']
  _sn_check('sn %s clamped' % _SN_ID(shape), got, ref, bound)


@pytest.mark.parametrize('shape', [(1, 1, 1, 1), (1, 1, 17, 63), (3, 3, 8, 257), (1, 1, 33, 1024), (3, 3, 16, 32)], ids=_SN_ID)
def test_spectral_norm_gradient_into_a_sink_that_holds_values(ops, shape):
  """tg_spectral_norm_bwd with accumulate = 1 (ops.GradSink.register(w, sink): the trainer's route): forward + backward twice
  onto a sink pre-filled with seeded values -> sink0 + 2 gw, every element inside the sum of the two single-call bounds plus
  the two fp32 additions (2 2^-24 |ref|); w.grad stays None."""
  k_rows, cout = shape[0] * shape[1] * shape[2], shape[3]
  for scale, kind in ((0.1, 'random'), (30.0, 'converged')):
    w, u, G = _sn_inputs(shape, scale, kind, salt=1)
    gen = torch.Generator().manual_seed(k_rows * 1031 + cout)
    sink0 = torch.randn(shape, generator=gen) * float(G.abs().mean()) / scale      # of the gradient's own size: gw ~ G / sigma
    wd, sink = w.clone().to(dev()).requires_grad_(True), sink0.clone().to(dev())
    ops.GradSink.clear()
    ops.GradSink.register(wd, sink)
    try:
      for _ in range(2):
        w_bar, _ = ops.spectral_norm(wd, u.to(dev()))
        (w_bar * G.to(dev())).sum().backward()
    finally:
      ops.GradSink.clear()
    assert wd.grad is None
    ref, bound = E.sn_bounds(w.reshape(k_rows, cout), u, G.reshape(k_rows, cout))
    want = sink0.double().numpy().reshape(k_rows, cout) + 2.0 * ref['gw']
    _ew_note('spectral norm gw into sink', 'f32', E.assert_elementwise(host(sink).reshape(k_rows, cout), want,
                                                                      2.0 * bound['gw'] + 2.0 * E.U32 * np.abs(want),
                                                                      'sn sink %s %g %s' % (_SN_ID(shape), scale, kind)))


@pytest.mark.parametrize('shape', [(1, 1, 5, 1), (3, 3, 7, 129), (1, 1, 16, 1023), (3, 3, 16, 32)], ids=_SN_ID)
def test_spectral_norm_ten_chained_power_iterations(ops, shape):
  """Ten runs, each from the previous run's u' (what a training run does): every step's sigma, u', v and w_bar element-wise
  against the float64 step taken from the DEVICE's own u (as the Adam test hands the reference the state the launch read)."""
  k_rows, cout = shape[0] * shape[1] * shape[2], shape[3]
  w, u, G = _sn_inputs(shape, 0.1, 'random', salt=2)
  for step in range(10):
    got, u_dev = _sn_run(ops, w, u, G)
    ref, bound = E.sn_bounds(w.reshape(k_rows, cout), u, G.reshape(k_rows, cout))
    _sn_check('sn chained %s step %d' % (_SN_ID(shape), step), got, ref, bound)
    u = u_dev.cpu().reshape(1, cout)


SN_MULTI_SHAPES = [SN_SHAPES[i] for i in (11, 0, 13, 2, 19, 7, 12, 1, 9, 16, 3, 14, 8, 17, 4, 10, 5, 15, 6, 18,
                                           0, 12, 2, 13, 1, 11, 7, 9, 3, 14, 16, 4, 19)]      # 33 jobs: 1-block and many-block jobs adjacent


def test_spectral_norm_multi_of_33_jobs_and_assign_u(ops):
  """tg_spectral_norm_fwd_multi over a table of 33 jobs (config 4 lays 60 end to end; sn_job_of finds each block's job at every
  boundary: jobs of 1 and of hundreds of blocks next to each other, cout = 1, 1023 and 1024 among them) and over a table of ONE
  job: w_bar, u' and the gradients equal the one-kernel entry point's bit for bit.  SnTable.assign_u (tg_sn_assign_u): u
  equals u' for every job afterwards, bit for bit, and a second run from the assigned u again equals the single-kernel path."""
  assert len(SN_MULTI_SHAPES) == 33
  g = torch.Generator().manual_seed(41)
  ws = [(torch.randn(*sh, generator=g) * 0.1).to(dev()) for sh in SN_MULTI_SHAPES]
  us = [torch.randn(1, sh[3], generator=g).to(dev()) for sh in SN_MULTI_SHAPES]
  gq = [torch.randn(*sh, generator=g).to(dev()) for sh in SN_MULTI_SHAPES]
  outs = [torch.empty(w.numel(), dtype=torch.float32, device=w.device) for w in ws]
  wds = [w.clone().requires_grad_(True) for w in ws]

  def single(j):
    wd = ws[j].clone().requires_grad_(True)
    wb, un = ops.spectral_norm(wd, us[j].clone())
    (wb * gq[j]).sum().backward()
    return wb.detach().clone(), un.detach().clone(), wd.grad.clone()

  table = None
  for run in range(2):
    ones = [single(j) for j in range(33)]
    for wd in wds:
      wd.grad = None
    res, table2 = ops.spectral_norm_multi(list(zip(wds, us, outs)), table)
    assert run == 0 or table2 is table
    table = table2
    sum((wb * q).sum() for (wb, _), q in zip(res, gq)).backward()
    for j, ((wb, un), wd, (wb1, un1, g1)) in enumerate(zip(res, wds, ones)):
      assert torch.equal(wb.detach(), wb1) and torch.equal(un.detach().reshape(-1), un1.reshape(-1)), (run, j, SN_MULTI_SHAPES[j])
      assert torch.equal(wd.grad, g1), (run, j, SN_MULTI_SHAPES[j])
    before = [u.clone() for u in us]
    table.assign_u()
    for j, (u, (u_new, _, _, _)) in enumerate(zip(us, table.bufs)):
      assert torch.equal(u.reshape(-1), u_new), (run, j, SN_MULTI_SHAPES[j])
      assert u.numel() == 1 or not torch.equal(u, before[j]), j
  # a table of a single job (njobs = 1: sn_job_of's loop body never runs)
  j = SN_MULTI_SHAPES.index((1, 1, 16, 1023))
  wd1, out1 = ws[j].clone().requires_grad_(True), torch.empty(ws[j].numel(), dtype=torch.float32, device=dev())
  want = single(j)
  res1, t1 = ops.spectral_norm_multi([(wd1, us[j], out1)], None)
  assert t1.n == 1
  (res1[0][0] * gq[j]).sum().backward()
  assert torch.equal(res1[0][0].detach(), want[0]) and torch.equal(res1[0][1].detach().reshape(-1), want[1].reshape(-1))
  assert torch.equal(wd1.grad, want[2])
  t1.assign_u()
  assert torch.equal(us[j].reshape(-1), t1.bufs[0][0])


def test_spectral_norm_refuses_what_it_cannot_run(ops):
  """cout = 1025 (sn_finish holds u_raw in four registers per thread: 1024 columns) is refused with TG_EINVAL by
  tg_spectral_norm_fwd and by tg_sn_table_fill, a workspace one byte short by the forward and the backward; nothing is launched
  (every output keeps its sentinel, the host table and the running totals keep theirs).  tg_spectral_norm_bwd has no such
  limit -- sn_rowdot strides over the columns and sn_bwd_apply is element-wise -- and computes cout = 1025 from hand-made
  u' / v / stats: checked against the closed form in float64 on the operands it reads."""
  import ctypes
  from twingan_amd import _lib
  lib = _lib.load()
  st = torch.cuda.current_stream().cuda_stream
  rng = np.random.RandomState(1025)

  def run(k_rows, cout, short=0, which='fwd'):
    w, u, G = (to_dev(rng.randn(*s)) for s in ((k_rows, cout), (cout,), (k_rows, cout)))
    outs = [torch.full((n,), -7.25, device=dev()) for n in (k_rows * cout, cout, k_rows, 2)]
    nbytes = lib.tg_spectral_norm_workspace(k_rows, cout)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=dev())
    if which == 'fwd':
      rc = lib.tg_spectral_norm_fwd(w.data_ptr(), u.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(),
                                    outs[3].data_ptr(), k_rows, cout, ws.data_ptr(), nbytes - short, st)
    else:
      rc = lib.tg_spectral_norm_bwd(G.data_ptr(), w.data_ptr(), u.data_ptr(), u.data_ptr(), outs[2].data_ptr(), outs[3].data_ptr(),
                                    outs[0].data_ptr(), 0, k_rows, cout, ws.data_ptr(), nbytes - short, st)
    torch.cuda.synchronize()
    return rc, all(bool((o == -7.25).all()) for o in outs) and bool((ws == 0).all())

  TG_EINVAL = -1      # include/twingan_hip.h
  assert run(3, 1025) == (TG_EINVAL, True)
  assert run(5, 70, short=1) == (TG_EINVAL, True)
  assert run(5, 70, short=1, which='bwd') == (TG_EINVAL, True)
  assert run(5, 70)[0] == 0
  # tg_sn_table_fill
  host_table = ctypes.create_string_buffer(b'\x5a' * lib.tg_sn_table_bytes(2), lib.tg_sn_table_bytes(2))
  totals = (ctypes.c_int32 * 3)(11, 12, 13)
  buf = torch.zeros(1025 * 3 + 4096, device=dev())
  nbytes = lib.tg_spectral_norm_workspace(3, 1025)
  wsb = torch.zeros(nbytes, dtype=torch.uint8, device=dev())
  p = buf.data_ptr()
  rc = lib.tg_sn_table_fill(1, p, p, p, p, p, p, wsb.data_ptr(), nbytes, 3, 1025, ctypes.addressof(host_table), totals)
  assert rc == TG_EINVAL and tuple(totals) == (11, 12, 13) and host_table.raw == b'\x5a' * lib.tg_sn_table_bytes(2)
  rc = lib.tg_sn_table_fill(1, p, p, p, p, p, p, wsb.data_ptr(), lib.tg_spectral_norm_workspace(3, 1024) - 1, 3, 1024,
                            ctypes.addressof(host_table), totals)
  assert rc == TG_EINVAL and tuple(totals) == (11, 12, 13)
  # the backward at cout = 1025, from hand-made operands
  k_rows, cout = 3, 1025
  w, u, G = (torch.randn(*s, generator=torch.Generator().manual_seed(7 + i)) * sc
             for i, (s, sc) in enumerate((((k_rows, cout), 0.1), ((1, cout), 1.0), ((k_rows, cout), 1.0))))
  r = E.sn_formulas(w, u, G, torch.float64)
  f32 = lambda a: np.asarray(a, np.float32)
  u_new, v, stats = f32(r['u_new']), f32(r['v']), f32(r['stats'])
  ops_in = (G.numpy(), w.numpy(), u.numpy().reshape(-1), u_new, v, stats)
  ref = E.sn_bwd_closed_form(*ops_in)
  r32 = E.sn_bwd_closed_form(*ops_in, dt=np.float32)
  sig, s = float(stats[0]), float((G.double() * w.double()).sum())
  a = w.double().numpy() @ u_new.astype(np.float64)
  b = (a - v * (v.astype(np.float64) * a).sum()) / float(stats[1])
  mag = np.abs(G.numpy()) / sig + abs(s) / sig ** 2 * (np.abs(np.outer(v, u_new)) + np.abs(np.outer(b, u.numpy().reshape(-1))))
  bound = E.e32_bound(ref, max(E.e32(r32, ref), E.U32 * float(mag.max())), 'f32')
  gw = torch.full((k_rows, cout), float('nan'), device=dev())
  nbytes = lib.tg_spectral_norm_workspace(k_rows, cout)
  wsb = torch.empty(nbytes, dtype=torch.uint8, device=dev())
  dv = [to_dev(x) for x in ops_in]
  import twingan_amd.ops as O
  O.call('tg_spectral_norm_bwd', dv[0].data_ptr(), dv[1].data_ptr(), dv[2].data_ptr(), dv[3].data_ptr(), dv[4].data_ptr(),
         dv[5].data_ptr(), gw.data_ptr(), 0, k_rows, cout, wsb.data_ptr(), nbytes, st)
  _ew_note('spectral norm bwd cout 1025', 'f32', E.assert_elementwise(host(gw), ref, bound, 'sn bwd at cout 1025'))


# ------------------------------------------------------------------------------------------------ the loss tail
def _t32(a):
  return torch.from_numpy(np.ascontiguousarray(a, np.float32))


@pytest.mark.parametrize('family', ['random', 'parallel', 'opposite', 'clamped'])
@pytest.mark.parametrize('b,d', [(1, 1), (3, 5), (4, 256), (5, 257), (16, 600), (2, 1024)])
def test_cosine_distance_elementwise(ops, b, d, family):
  """tg_cosine_distance_fwd / _bwd (the encoder-distillation loss), weight 0.7, incoming gradient 2.5: one element, a partial
  workgroup, exactly one / one more than one trip of 256, several trips.  random; p = 3 e (distance 0, gradient ~ 0: the two
  summands cancel); p = -e / 2 (distance 2); p 1e-8 with one all-zero row (|p|^2 < 1e-12: the clamped branch of the backward,
  phat = p 1e6).  Against float64 autograd of the formula with the clamp written as the kernel documents it."""
  rng = np.random.RandomState(zlib.crc32(('cos%d%d%s' % (b, d, family)).encode()) % (2 ** 31))
  e = rng.randn(b, d)
  p = {'random': rng.randn(b, d), 'parallel': 3.0 * e, 'opposite': -0.5 * e, 'clamped': rng.randn(b, d) * 1e-8}[family]
  if family == 'clamped':
    p[b // 2] = 0.0
  e, p = _t32(e), _t32(p)
  assert family != 'clamped' or float((p.double() ** 2).sum(1).max()) < 0.5e-12
  ref, b_out, b_gp = E.cosine_bounds(e, p, 0.7, 2.5)
  pd = p.clone().to(dev()).requires_grad_(True)
  out = ops.cosine_distance(e.clone().to(dev()), pd, 0.7)
  (out * 2.5).backward()
  r = abs(out.item() - ref['out']) / b_out
  print('[cosine] %s (%d, %d): out %.9g ref %.9g ratio %.3f' % (family, b, d, out.item(), ref['out'], r))
  assert r <= 1.0, (out.item(), ref['out'], b_out)
  _ew_note('cosine distance', 'f32', r)
  _ew_note('cosine distance grad', 'f32', E.assert_elementwise(host(pd.grad), ref['gp'], b_gp, 'cosine %s d p' % family))


PRED_MODES = [('hinge_fake', 1, 1.0, 1.0), ('hinge_real', 1, 1.0, -1.0), ('xent_1', 2, 1.0, 0.0), ('xent_0', 2, 0.0, 0.0),
              ('square', 3, 0.0, 0.0)]


def _pred_values(n, seed):
  """4 N(0, 1) with +-88 planted (expf(-|x|) underflows, the sigmoid saturates), +-20 (sigmoid - 1 cancels in fp32) and +-1
  (a + b x = 0 exactly for the hinge with a = 1, b = -+1), as far as n has room."""
  x = np.random.RandomState(seed).randn(n) * 4.0
  for i, v in enumerate((88.0, -88.0, 1.0, -1.0, 20.0, -20.0)):
    if 1 + 41 * i < n or (n == 7 and i < 6):
      x[(1 + 41 * i) if n > 7 else i + 1] = v
  return x.astype(np.float32).astype(np.float64)


@pytest.mark.parametrize('name,mode,a,b', PRED_MODES, ids=[m[0] for m in PRED_MODES])
@pytest.mark.parametrize('n', [1, 7, 256, 257, 5000])
def test_pred_loss_elementwise(ops, n, name, mode, a, b):
  """hinge_mean / sigmoid_xent_mean / square_mean (tg_pred_loss_fwd / _bwd, modes 1-3) at 1, 7, 256, 257 and 5000 predictions,
  weight 0.3, incoming gradient 2.5.  Forward: reduction_bound with the chain of one 256-thread workgroup; backward: per
  element (elementwise.pred_loss_bwd_bound)."""
  x = _pred_values(n, 100 + n)
  if n == 1 and mode == 1:
    x[0] = -b      # a + b x = 0
  f, df, parts, term_ops, sig = E.pred_loss_reference(x, mode, a, b)
  xd = to_dev(x).requires_grad_(True)
  fn = {1: lambda t: ops.hinge_mean(t, a, b, 0.3), 2: lambda t: ops.sigmoid_xent_mean(t, a, 0.3), 3: lambda t: ops.square_mean(t, 0.3)}[mode]
  out = fn(xd)
  (out * 2.5).backward()
  want = 0.3 * f.sum() / n
  bound = E.pred_loss_fwd_bound(parts.sum(), n, 0.3 / n, term_ops)
  r = abs(out.item() - want) / bound
  print('[pred loss] %s n %d: got %.9g ref %.9g ratio %.3f' % (name, n, out.item(), want, r))
  assert r <= 1.0, (out.item(), want, bound)
  _ew_note('pred loss ' + name.split('_')[0], 'f32', r)
  g = 2.5 * 0.3 / n
  _ew_note('pred loss grad ' + name.split('_')[0], 'f32',
           E.assert_elementwise(host(xd.grad), g * df, E.pred_loss_bwd_bound(g * df, abs(g), sig), 'pred loss %s d x' % name))
  if mode == 1:
    assert np.all(host(xd.grad)[a + b * x == 0.0] == 0.0) and (a + b * x == 0.0).any()


PRED_JOBS = [      # (group, term, mode, a, b, coef): two jobs into term 0 from different groups, two jobs on group 1 into
    (0, 0, 1, 1.0, -1.0, 0.5), (2, 0, 1, 1.0, 1.0, 0.5),      # different terms, every mode, term 3 fed by nobody, term 4 fed but
    (1, 1, 2, 1.0, 0.0, 0.7), (1, 2, 2, 0.0, 0.0, 0.3),        # without a gradient
    (0, 2, 3, 0.0, 0.0, 1e-3), (2, 1, 0, 0.0, 0.0, -1.0),
    (1, 4, 1, 1.0, 1.0, 2.0), (0, 4, 0, 0.0, 0.0, 1.0)]


def _pred_losses_reference(x, gs, jobs, nterms, gterms):
  """-> (terms, their bounds, d pred, its bound) in float64: per job coef mean f over its group; acc_t += coef * tot / gs is a
  multiply, a division (2) and an addition per job: extra_ops 4; the backward adds, per job, g_t (coef / gs) df: the division
  (2), two multiplies, the addition: 6 2^-24 |summand| each (+ the sigmoid term of mode 2)."""
  terms, tb = np.zeros(nterms), np.zeros(nterms)
  gx, gb = np.zeros_like(x), np.full_like(x, E.TINY)
  for grp, t, mode, a, b, coef in jobs:
    xs = x[grp * gs:(grp + 1) * gs]
    f, df, parts, term_ops, sig = E.pred_loss_reference(xs, mode, a, b)
    terms[t] += coef * f.sum() / gs
    tb[t] += E.pred_loss_fwd_bound(parts.sum(), gs, coef / gs, term_ops, extra_ops=3)
    if gterms[t] is not None:
      k = gterms[t] * coef / gs
      gx[grp * gs:(grp + 1) * gs] += k * df
      gb[grp * gs:(grp + 1) * gs] += E.pred_loss_bwd_bound(k * df, abs(k), sig, ops=6)
  return terms, tb, gx, gb


@pytest.mark.parametrize('gs', [1, 3, 64, 255, 256, 257, 1000])
def test_pred_losses_elementwise(ops, gs):
  """tg_pred_losses_fwd / _bwd: three groups of gs predictions, eight jobs over four of five terms (PRED_JOBS), gradients for
  three terms only (term 4 is fed and gets None; term 3 is fed by no job and must read 0).  Against float64, and against the
  sum of single PredLossFn calls (each inside its own bound)."""
  x = _pred_values(3 * gs, 200 + gs)
  gts = [1.5, -0.5, 2.0, None, None]
  terms, tb, gx, gb = _pred_losses_reference(x, gs, PRED_JOBS, 5, gts)
  xd = to_dev(x).reshape(3 * gs, 1).requires_grad_(True)
  out = ops.pred_losses(xd, gs, PRED_JOBS, 5)
  torch.autograd.backward([out[t] for t in (0, 1, 2)], [torch.full((1,), gts[t], device=dev()) for t in (0, 1, 2)])
  got = np.array([o.item() for o in out])
  assert got[3] == 0.0
  ratios = np.abs(got - terms) / np.maximum(tb, E.TINY)
  print('[pred losses] gs %d: terms %s ratios %s' % (gs, got, np.round(ratios, 3)))
  assert np.all(ratios <= 1.0), (got, terms, tb)
  _ew_note('pred losses', 'f32', ratios.max())
  _ew_note('pred losses grad', 'f32', E.assert_elementwise(host(xd.grad).reshape(-1), gx, gb, 'pred_losses d pred'))
  # the sum of single calls
  one_t, one_tb = np.zeros(5), np.zeros(5)
  xs = to_dev(x).requires_grad_(True)
  loss = None
  for grp, t, mode, a, b, coef in PRED_JOBS:
    seg = xs[grp * gs:(grp + 1) * gs]
    o = ops.PredLossFn.apply(seg.contiguous(), mode, a, b, coef)
    f, df, parts, term_ops, sig = E.pred_loss_reference(x[grp * gs:(grp + 1) * gs], mode, a, b)
    one_t[t] += o.item()
    one_tb[t] += E.pred_loss_fwd_bound(parts.sum(), gs, coef / gs, term_ops)
    if gts[t] is not None:
      loss = o * gts[t] if loss is None else loss + o * gts[t]
  loss.backward()
  assert np.all(np.abs(got - one_t) <= tb + one_tb + 8 * E.U32 * np.abs(terms)), (got, one_t)
  E.assert_elementwise(host(xd.grad).reshape(-1), host(xs.grad), 2.0 * gb + 8 * E.U32 * np.abs(gx), 'pred_losses vs single calls')


def test_pred_losses_limits(ops):
  """12 jobs and 8 terms are taken (and right); 13 jobs, 9 terms, a group or a term index out of range are refused."""
  from twingan_amd._lib import TgError
  gs = 5
  x = _pred_values(3 * gs, 77)
  jobs = [(j % 3, j % 8, 1 + j % 3, 1.0 if j % 3 != 2 else 0.0, -1.0, 0.25 + j) for j in range(12)]
  gts = [0.5 + t for t in range(8)]
  terms, tb, gx, gb = _pred_losses_reference(x, gs, jobs, 8, gts)
  xd = to_dev(x).reshape(-1, 1).requires_grad_(True)
  out = ops.pred_losses(xd, gs, jobs, 8)
  torch.autograd.backward(list(out), [torch.full((1,), g, device=dev()) for g in gts])
  got = np.array([o.item() for o in out])
  assert np.all(np.abs(got - terms) <= tb), (got, terms, tb)
  E.assert_elementwise(host(xd.grad).reshape(-1), gx, gb, 'pred_losses at 12 jobs / 8 terms')
  for bad_jobs, nterms in ((jobs + [jobs[0]], 8), (jobs, 9), ([(3, 0, 1, 1.0, 1.0, 1.0)], 2), ([(0, 2, 1, 1.0, 1.0, 1.0)], 2),
                           ([(-1, 0, 1, 1.0, 1.0, 1.0)], 2), ([(0, -1, 1, 1.0, 1.0, 1.0)], 2)):
    with pytest.raises(TgError):
      ops.pred_losses(to_dev(x).reshape(-1, 1), gs, bad_jobs, nterms)


@pytest.mark.parametrize('n', [2, 5, 24])
def test_sum_scalars_elementwise(ops, n):
  """tg_sum_scalars (tf.add_n over the loss collection): magnitudes over six decades, both signs, summed in argument order:
  |got - ref| <= n 2^-24 sum|x|; every term's gradient IS the incoming one, bit for bit.  25 terms are refused."""
  import ctypes
  from twingan_amd import _lib
  rng = np.random.RandomState(300 + n)
  vals = (rng.randn(n) * 10.0 ** rng.uniform(-3, 3, n)).astype(np.float32)
  ts = [to_dev(vals[i:i + 1]).requires_grad_(True) for i in range(n)]
  out = ops.sum_scalars(ts)
  gin = torch.full((1,), 1.7, device=dev())
  out.backward(gin)
  ref, bound = vals.astype(np.float64).sum(), n * E.U32 * np.abs(vals.astype(np.float64)).sum() + E.TINY
  assert abs(out.item() - ref) <= bound, (out.item(), ref, bound)
  _ew_note('sum_scalars', 'f32', abs(out.item() - ref) / bound)
  for t in ts:
    assert torch.equal(t.grad, gin)
  if n == 24:
    keep = ts + [to_dev(vals[:1])]
    ptrs = (ctypes.c_void_p * 25)(*[t.data_ptr() for t in keep])
    res = torch.full((1,), -7.25, device=dev())
    rc = _lib.load().tg_sum_scalars(ctypes.addressof(ptrs), 25, res.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == -1 and res.item() == -7.25


VAR_SHAPES = [(1, 1, 1, 3), (2, 8, 8, 3), (3, 17, 19, 3), (4, 64, 64, 3), (16, 32, 32, 3)]


@pytest.mark.parametrize('dname', sorted(EW_DTYPES))
@pytest.mark.parametrize('shape', VAR_SHAPES, ids=['x'.join(map(str, s)) for s in VAR_SHAPES])
def test_batch_variance_and_dragan_interpolates_elementwise(ops, shape, dname):
  """ops.batch_variance (tg_sum, tg_sample_sumsq, tg_var_from_sums) and ops.dragan_interpolates on U[-1, 1], on 0.9 + 0.01 U (the
  cancellation case: the variance is 1e-5 of E[x^2]) and on the constant 0.7 (the result must be >= 0).  The reference is taken
  on the stored values; the variance's bound is relative to E[x^2] (elementwise.variance_bound), the interpolates' per element:
  u |ref| + the stored delta's own rounding u |delta| + 5 fp32 operations (noise coef var: 2; axpby: 3) + the variance's bound
  carried through 0.5 |alpha noise|."""
  dtype = EW_DTYPES[dname]
  u = E.unit_roundoff(dtype)
  rng = np.random.RandomState(zlib.crc32(('var%s' % (shape,)).encode()) % (2 ** 31))
  for fam in ('uniform', 'offset', 'constant'):
    base = rng.uniform(-1, 1, shape)
    x = _round_dt({'uniform': base, 'offset': 0.9 + 0.01 * base, 'constant': np.full(shape, 0.7)}[fam], dtype)
    noise, alpha = _round_dt(rng.randn(*shape), dtype), rng.rand(shape[0]).astype(np.float32).astype(np.float64)
    var, bvar, L = E.variance_bound(x, dtype, shape[0])
    xd = to_dev(x, dtype)
    got = ops.batch_variance(xd).item()
    r = abs(got - var) / bvar
    print('[variance] %s %s %s: got %.9g ref %.9g L %d ratio %.3f' % (dname, shape, fam, got, var, L, r))
    assert got >= 0.0 and r <= 1.0, (got, var, bvar)
    _ew_note('batch_variance', dname, r)
    out = ops.dragan_interpolates(xd, to_dev(noise, dtype), to_dev(alpha))
    an = 0.5 * np.abs(alpha.reshape(-1, 1, 1, 1) * noise)
    delta = 0.5 * alpha.reshape(-1, 1, 1, 1) * noise * var
    ref = x + delta
    bound = u * np.abs(ref) + (1 + u) * (u * np.abs(delta) + 5 * E.U32 * (np.abs(x) + np.abs(delta)) + bvar * an) + E.tiny(dtype)
    _ew_note('dragan_interpolates', dname, E.assert_elementwise(host(out), ref, bound, 'dragan_interpolates %s' % fam))


# ------------------------------------------------------------------------------------------------ small dense kernels
SMALL_GEMM_CASES = [(1, 1, 1), (3, 5, 31), (3, 5, 32), (3, 5, 33), (64, 64, 40), (64, 65, 40), (7, 1, 256), (2, 4096, 300),
                    (65, 63, 100), (4, 16, 512)]


def _small_gemm_wave(m, n, k):
  """tg_small_gemm's choice (csrc/reduce.hip): one wave per output element when k >= 32 and m n <= 4096, else one thread."""
  return k >= 32 and m * n <= 4096


@pytest.mark.parametrize('m,n,k', SMALL_GEMM_CASES)
def test_small_gemm_elementwise(ops, m, n, k):
  """GemmFn (tg_small_gemm), all four transposes, forward and both gradients (themselves GEMMs: K = n for d a, K = m for d b):
  every element inside conv_bound with K summands in fp32.  The shapes sit on both sides of both conditions of the kernel
  choice (k = 31 / 32 / 33 -- at 33 lanes 33..63 of the wave kernel have no term; m n = 4096 / 4160), and the gradients of one
  shape take the other kernel (k = 300, m n = 8192: the thread kernel forward; d b is [300, 4096] from K = 2: thread; d a is
  [2, 300] from K = 4096: wave).  Through the C ABI once each with a bias and with accumulate = 1 onto a non-zero C: K + 1.
  tg_last_kernel reports the conv kernels only, so the choice is pinned by its restatement here, not by a report."""
  import twingan_amd.ops as O
  assert [_small_gemm_wave(*c) for c in SMALL_GEMM_CASES] == [False, False, True, True, True, False, True, False, True, True]
  rng = np.random.RandomState(zlib.crc32(('sg%d%d%d' % (m, n, k)).encode()) % (2 ** 31))
  f32 = lambda a: a.astype(np.float32).astype(np.float64)
  for ta in (False, True):
    for tb in (False, True):
      a, b, g = f32(rng.randn(k, m) if ta else rng.randn(m, k)), f32(rng.randn(n, k) if tb else rng.randn(k, n)), f32(rng.randn(m, n))
      oa, ob = (a.T if ta else a), (b.T if tb else b)
      ad, bd = to_dev(a).requires_grad_(True), to_dev(b).requires_grad_(True)
      c = ops.GemmFn.apply(ad, bd, ta, tb)
      c.backward(to_dev(g))
      what = 'small gemm (%d, %d, %d) ta=%d tb=%d' % (m, n, k, ta, tb)
      w = E.assert_elementwise(host(c), oa @ ob, E.conv_bound(oa @ ob, np.abs(oa) @ np.abs(ob), k, 'f32'), what)
      ga, ma = g @ ob.T, np.abs(g) @ np.abs(ob).T
      gb, mb = oa.T @ g, np.abs(oa).T @ np.abs(g)
      w = max(w, E.assert_elementwise(host(ad.grad), ga.T if ta else ga, E.conv_bound(ga.T if ta else ga, ma.T if ta else ma, n, 'f32'),
                                      what + ' d a'))
      w = max(w, E.assert_elementwise(host(bd.grad), gb.T if tb else gb, E.conv_bound(gb.T if tb else gb, mb.T if tb else mb, m, 'f32'),
                                      what + ' d b'))
      _ew_note('small gemm', 'f32', w)
      # the C ABI: bias, and accumulate onto a non-zero C
      bias, c0 = f32(rng.randn(n)), f32(rng.randn(m, n))
      st = torch.cuda.current_stream().cuda_stream
      cb, cacc, biasd = torch.empty(m, n, device=dev()), to_dev(c0), to_dev(bias)
      O.call('tg_small_gemm', ad.data_ptr(), bd.data_ptr(), biasd.data_ptr(), cb.data_ptr(), m, n, k, int(ta), int(tb), 0, st)
      O.call('tg_small_gemm', ad.data_ptr(), bd.data_ptr(), None, cacc.data_ptr(), m, n, k, int(ta), int(tb), 1, st)
      mag = np.abs(oa) @ np.abs(ob)
      w = E.assert_elementwise(host(cb), oa @ ob + bias, E.conv_bound(oa @ ob + bias, mag + np.abs(bias), k + 1, 'f32'), what + ' bias')
      w = max(w, E.assert_elementwise(host(cacc), oa @ ob + c0, E.conv_bound(oa @ ob + c0, mag + np.abs(c0), k + 1, 'f32'), what + ' acc'))
      _ew_note('small gemm C ABI', 'f32', w)


FC_CASES = [(1, 1, 1), (6, 3, 40), (5, 7, 7), (33, 2, 65), (64, 1, 256), (64, 16, 256), (16, 1, 512), (2, 16, 1000), (4, 9, 5), (3, 70, 80)]


@pytest.mark.parametrize('dname', sorted(EW_DTYPES))
@pytest.mark.parametrize('m,n,k', FC_CASES)
def test_fully_connected_elementwise(ops, m, n, k, dname):
  """ops.fully_connected in first-order passes (FcFn: tg_fc_fwd / tg_fc_bwd, one launch each way; x in the activations' type):
      y   conv_bound(K = k + 1, 'f32')     k products and the bias       gx   conv_bound(K = n, dtype)
      gw, gb   wgrad_bound(P = m); through a gradient sink that holds values one more summand (P = m + 1, mag + |sink|)
  and gx alone in a no_param_grads pass (gw / gb not written).  n = k (5, 7, 7) is the last shape FcFn takes; (4, 9, 5) has
  n > k, which tg_fc_bwd's one-thread-per-k layout cannot serve: fully_connected must take the composition (asserted by the
  grad_fn's name) -- the same bounds hold (the cast is exact, the GEMM has the same k products).  (3, 70, 80) is the
  only shape with n > 64, where gb's columns pass the first 64-thread workgroup of tg_fc_bwd."""
  dtype = EW_DTYPES[dname]
  rng = np.random.RandomState(zlib.crc32(('fc%d%d%d' % (m, n, k)).encode()) % (2 ** 31))
  f32 = lambda a: a.astype(np.float32).astype(np.float64)
  x, w, b, g = _round_dt(rng.randn(m, k), dtype), f32(rng.randn(k, n)), f32(rng.randn(n)), f32(rng.randn(m, n))
  xd = to_dev(x, dtype).requires_grad_(True)
  wd, bd = to_dev(w).requires_grad_(True), to_dev(b).requires_grad_(True)
  y = ops.fully_connected(xd, wd, bd)
  assert type(y.grad_fn).__name__ == ('FcFnBackward' if n <= k else 'AddRowBiasFnBackward') and y.dtype == torch.float32
  y.backward(to_dev(g))
  what = 'fc (%d, %d, %d)' % (m, n, k)
  ry, rgx, rgw, rgb = x @ w + b, g @ w.T, x.T @ g, g.sum(0)
  mgw, mgb = np.abs(x).T @ np.abs(g), np.abs(g).sum(0)
  _ew_note('fc y', dname, E.assert_elementwise(host(y), ry, E.conv_bound(ry, np.abs(x) @ np.abs(w) + np.abs(b), k + 1, 'f32'), what + ' y'))
  _ew_note('fc gx', dname, E.assert_elementwise(host(xd.grad), rgx, E.conv_bound(rgx, np.abs(g) @ np.abs(w).T, n, dtype), what + ' gx'))
  _ew_note('fc gw', dname, E.assert_elementwise(host(wd.grad), rgw, E.wgrad_bound(rgw, mgw, m), what + ' gw'))
  _ew_note('fc gb', dname, E.assert_elementwise(host(bd.grad), rgb, E.wgrad_bound(rgb, mgb, m), what + ' gb'))
  # gradient sinks that hold seeded values (FcFn adds into them; the composition's GemmFn hands its gradients to autograd)
  sw0, sb0 = f32(rng.randn(k, n)), f32(rng.randn(n))
  sw, sb = to_dev(sw0), to_dev(sb0)
  ops.GradSink.clear()
  ops.GradSink.register(wd, sw)
  ops.GradSink.register(bd, sb)
  wd.grad = bd.grad = xd.grad = None
  try:
    ops.fully_connected(xd, wd, bd).backward(to_dev(g))
    if n <= k:
      assert wd.grad is None and bd.grad is None
      _ew_note('fc gw sink', dname, E.assert_elementwise(host(sw), sw0 + rgw, E.wgrad_bound(sw0 + rgw, mgw + np.abs(sw0), m + 1), what + ' gw sink'))
      _ew_note('fc gb sink', dname, E.assert_elementwise(host(sb), sb0 + rgb, E.wgrad_bound(sb0 + rgb, mgb + np.abs(sb0), m + 1), what + ' gb sink'))
    # gx alone: a no_param_grads pass (the gradient penalty's inner gradient) leaves the registered parameters' gradients alone
    keep = [t.clone() for t in (sw, sb)]
    wd.grad = bd.grad = xd.grad = None
    with ops.no_param_grads():
      ops.fully_connected(xd, wd, bd).backward(to_dev(g))
    assert wd.grad is None and bd.grad is None and torch.equal(sw, keep[0]) and torch.equal(sb, keep[1])
    E.assert_elementwise(host(xd.grad), rgx, E.conv_bound(rgx, np.abs(g) @ np.abs(w).T, n, dtype), what + ' gx alone')
  finally:
    ops.GradSink.clear()


POINT_SIZES = [1, 255, 257, 16384, 16385, 3 * 16384 + 5, 4 * 32 * 32 * 64]


@pytest.mark.parametrize('dname', sorted(EW_DTYPES))
@pytest.mark.parametrize('numel', POINT_SIZES)
def test_tanh_mul3_scale_dev_and_dot_elementwise(ops, numel, dname):
  """tg_tanh_fwd / _bwd, tg_mul3 (TanhBwdFn's backward), tg_scale_dev and tg_dot, each on the operands it reads, from one
  element to 4 x 32 x 32 x 64 (what the attention layer's gamma sees), across tg_dot's 16384 elements per partial.  tanh inputs
  include +-20, +-1e-4 and 0.  Pointwise: u |ref| + (1 + u) ops 2^-24 mag -- tanh_bwd g (1 - y^2): 3 operations on |g| (1 + y^2);
  mul3: 3; scale_dev: 1 -- tanh's own error is E of the float32 restatement (torch on the CPU) at m = 16.  tg_dot:
  reduction_bound with the chain of its two stages (elementwise.dot_chain)."""
  import twingan_amd.ops as O
  dtype = EW_DTYPES[dname]
  u = E.unit_roundoff(dtype)
  rng = np.random.RandomState(numel % 9973)
  x = rng.randn(numel) * 2.0
  for i, v in enumerate((20.0, -20.0, 1e-4, -1e-4, 0.0)):
    if i * 50 < numel:
      x[(i * 50) % numel] = v
  x, g, v = _round_dt(x, dtype), _round_dt(rng.randn(numel), dtype), _round_dt(rng.randn(numel), dtype)
  xt = torch.from_numpy(x)
  y64 = torch.tanh(xt).numpy()
  y32 = torch.tanh(xt.float()).double().numpy()
  yd = ops.tanh(to_dev(x, dtype))
  _ew_note('tanh fwd', dname, E.assert_elementwise(host(yd), y64, E.e32_bound(y64, E.e32(y32, y64), dtype), 'tanh %d' % numel))
  pw = lambda ref, mag, n_ops: u * np.abs(ref) + (1 + u) * n_ops * E.U32 * np.abs(mag) + E.tiny(dtype)
  y = _round_dt(y64, dtype)      # the stored y the backward reads
  gd, vd, ysd = to_dev(g, dtype), to_dev(v, dtype), to_dev(y, dtype)
  st, dt = torch.cuda.current_stream().cuda_stream, O._dt(gd)
  out = torch.empty_like(gd)
  O.call('tg_tanh_bwd', gd.data_ptr(), ysd.data_ptr(), out.data_ptr(), numel, dt, st)
  _ew_note('tanh bwd', dname, E.assert_elementwise(host(out), g * (1 - y * y), pw(g * (1 - y * y), np.abs(g) * (1 + y * y), 3), 'tanh_bwd'))
  O.call('tg_mul3', ysd.data_ptr(), gd.data_ptr(), vd.data_ptr(), out.data_ptr(), -2.0, numel, dt, st)
  _ew_note('mul3', dname, E.assert_elementwise(host(out), -2.0 * y * g * v, pw(-2.0 * y * g * v, y * g * v, 3), 'mul3'))
  gam = np.float32(0.7)
  sc = ops.scale_dev(gd, to_dev(np.array([gam])))
  _ew_note('scale_dev', dname, E.assert_elementwise(host(sc), g * float(gam), pw(g * float(gam), g * float(gam), 1), 'scale_dev'))
  d = ops.DotFn.apply(gd, vd)
  L, nparts, per = E.dot_chain(numel)
  bound = E.reduction_bound(np.abs(g * v).sum(), L, term_ops=1)
  r = abs(d.item() - (g * v).sum()) / bound
  print('[dot] %s numel %d: %d partials of %d, L %d, ratio %.3f' % (dname, numel, nparts, per, L, r))
  assert r <= 1.0, (d.item(), (g * v).sum(), bound)
  _ew_note('dot', dname, r)
  if nparts > 1:      # the test's own power: the last partial left out moves the sum by more than the bound
    assert abs((g * v)[(nparts - 1) * per:].sum()) > bound, (nparts, per, bound)


def test_tanh_and_scale_second_order_at_the_attention_shape_bf16(ops):
  """The pattern of test_tanh_and_scale_second_order -- y = gamma tanh(x), gx = d <y, w1> / d x with create_graph, then the
  gradients of <gx, w2> towards x and gamma -- at 4 x 32 x 32 x 64 in bf16, element-wise.  With t = tanh(x), Et = u |t| + 16 E32
  the error of the STORED tanh, and every stored intermediate one more u of its magnitude:
      y      = gamma t                          stored once:       u |y| + |gamma| Et + 1 op
      gx     = g1 (1 - t^2),  g1 = rnd(w1 gamma)   two stores:        2 u mag + 2 |t g1| Et + 4 ops,  mag = |g1| (1 + t^2)
      d x    = rnd(rnd(-2 t g1 w2) (1 - t^2))      three stores:      3 u mag + 2 |g1 w2| (1 + 3 t^2) Et + 7 ops,  mag = 2 |t g1 w2| (1 + t^2)
      d gamma = sum w1 rnd(w2 (1 - t^2))           fp32, tg_dot:      sum [u + 3 ops] |w1 w2| (1 + t^2) + 2 |t w1 w2| Et, + the dot's chain"""
  dtype, dname, numel = torch.bfloat16, 'bf16', 4 * 32 * 32 * 64
  u = E.unit_roundoff(dtype)
  rng = np.random.RandomState(131)
  x, w1, w2 = (_round_dt(rng.randn(4, 32 * 32, 64), dtype) for _ in range(3))
  gam = float(np.float32(0.7))
  xd, gd = to_dev(x, dtype).requires_grad_(True), to_dev(np.array([gam])).requires_grad_(True)
  y = ops.scale_dev(ops.tanh(xd), gd)
  gx, = torch.autograd.grad(y, xd, grad_outputs=to_dev(w1, dtype), create_graph=True)
  torch.autograd.backward(gx, to_dev(w2, dtype))
  t = np.tanh(x)
  Et = u * np.abs(t) + 16 * E.e32(torch.tanh(torch.from_numpy(x).float()).double().numpy(), t)
  ops32 = lambda n_ops, mag: n_ops * E.U32 * mag
  g1 = w1 * gam
  r_y = gam * t
  b_y = u * np.abs(r_y) + (1 + u) * (abs(gam) * Et + ops32(1, np.abs(r_y))) + E.tiny(dtype)
  r_gx, m_gx = g1 * (1 - t * t), np.abs(g1) * (1 + t * t)
  b_gx = (1 + u) ** 2 * (2 * u * m_gx + 2 * np.abs(t * g1) * Et + ops32(4, m_gx)) + E.tiny(dtype)
  r_dx, m_dx = -2 * t * g1 * w2 * (1 - t * t), 2 * np.abs(t * g1 * w2) * (1 + t * t)
  b_dx = (1 + u) ** 3 * (3 * u * m_dx + 2 * np.abs(g1 * w2) * (1 + 3 * t * t) * Et + ops32(7, m_dx)) + 3 * E.tiny(dtype)
  _ew_note('tanh scale 2nd order y', dname, E.assert_elementwise(host(y), r_y, b_y, 'y'))
  _ew_note('tanh scale 2nd order gx', dname, E.assert_elementwise(host(gx), r_gx, b_gx, 'gx'))
  _ew_note('tanh scale 2nd order d x', dname, E.assert_elementwise(host(xd.grad), r_dx, b_dx, 'd x'))
  m_dg = np.abs(w1 * w2) * (1 + t * t)
  L, _, _ = E.dot_chain(numel)
  r_dg = (w1 * w2 * (1 - t * t)).sum()
  b_dg = ((u + 3 * E.U32) * m_dg + 2 * np.abs(t * w1 * w2) * Et).sum() * (1 + u) + E.reduction_bound(m_dg.sum(), L, term_ops=1)
  r = abs(gd.grad.item() - r_dg) / b_dg
  print('[tanh scale 2nd order] d gamma got %.9g ref %.9g ratio %.3f' % (gd.grad.item(), r_dg, r))
  assert r <= 1.0
  _ew_note('tanh scale 2nd order d gamma', dname, r)


# ------------------------------------------------------------------------------------------------ preprocessing, through the C ABI
PRE_U = {'f32': 0.0, 'f16': 2.0 ** -11, 'bf16': 2.0 ** -8}
PRE_PRECISION = {'f32': 'fp32', 'f16': 'fp16', 'bf16': 'bf16'}


@functools.lru_cache(maxsize=None)
def _pre_sources():
  """Nine decoded images: 1 x 1, one row, one column (sources SMALLER than every target but hw = 1: up-sampling, where an
  unclamped bottom / right tap reads past the image), 2 x 3 all white, 5 x 5 all black, 31 x 33 grey (three equal channels:
  saturate's s = 0), 40 x 13, 64 x 64 and 3 x 200 (down-sampling in one axis, up-sampling in the other)."""
  rng = np.random.RandomState(90)
  out = []
  for h, w in ((1, 1), (1, 7), (7, 1), (2, 3), (5, 5), (31, 33), (40, 13), (64, 64), (3, 200)):
    im = rng.randint(0, 256, (h, w, 3), dtype=np.uint8)
    if (h, w) == (2, 3):
      im[:] = 255
    elif (h, w) == (5, 5):
      im[:] = 0
    elif (h, w) == (31, 33):
      im[:] = im[:, :, :1]
    out.append(im)
  return out


def _pre_aug(n):
  """Flips alternate over the batch (so a flip meets every planted crop rectangle); brightness delta at +-32/255 and the
  saturation factor at 1.4999 and 0.5 (the ends of their ranges) in both orderings, the remaining images random draws."""
  rng = np.random.RandomState(91)
  aug = np.zeros((n, 4), np.float32)
  aug[:, 0] = np.arange(n) % 2
  aug[:, 1] = (np.arange(n) // 2) % 2
  aug[:, 2] = rng.uniform(-32.0 / 255.0, 32.0 / 255.0, n)
  aug[:, 3] = rng.uniform(0.5, 1.5, n)
  aug[:4, 2] = np.float32([32.0 / 255.0, -32.0 / 255.0, -32.0 / 255.0, 32.0 / 255.0])
  aug[:4, 3] = np.float32([1.4999, 0.5, 1.4999, 0.5])
  return aug


def _pre_crops(n, mid, hw):
  """(cy, cx, ch, cw): the whole mid x mid image, its last pixel alone, its last column -- twice over, so each meets both
  flips -- then draws of the host helper.  hw = 1 has mid = 1: only the whole-image rectangle exists."""
  from twingan_amd import data as D
  crop = D.draw_crops(n, mid, 0.8, np.random.default_rng(92))
  if mid == 1:
    crop[:] = (0, 0, 1, 1)
    return crop
  planted = [(0, 0, mid, mid), (mid - 1, mid - 1, 1, 1), (0, mid - 1, mid, 1)]
  for i in range(min(6, n)):
    crop[i] = planted[i % 3]
  return crop


def _pre_launch(pre, tables, color_space=None, mid=None):
  """tg_preprocess_images_crop through ops.call, as data.Preprocessor.run does it, from tables packed on the host."""
  import twingan_amd.ops as O
  from twingan_amd import data as D
  d = [t.clone().to(dev()) for t in tables]
  n = tables[1].numel()
  out = torch.full((n, pre.hw, pre.hw, 3), float('nan'), dtype=pre.dtype, device=dev())
  O.call('tg_preprocess_images_crop', d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[4].data_ptr() if len(d) > 4 else 0,
         d[3].data_ptr(), out.data_ptr(), n, pre.hw, pre.mid if mid is None else mid,
         D.COLOR_SPACES[pre.color_space] if color_space is None else color_space, O._dt(out), torch.cuda.current_stream().cuda_stream)
  return out


def _pre_check(what, dname, pre, images, want, aug=None, crop=None, mode_offsets=None):
  """The batch against the oracle, element-wise: u |want| + 3e-6 (the project's own fp32 figure for the two-stage path); then
  every image of the batch bit-identical to the same image preprocessed alone."""
  out = _pre_launch(pre, pre.pack(images, aug, crop, mode_offsets=mode_offsets))
  want = np.stack(want)
  _ew_note('preprocess', dname, E.assert_elementwise(host(out), want, PRE_U[dname] * np.abs(want) + 3e-6, what))
  bits = torch.int32 if pre.dtype == torch.float32 else torch.int16
  for i, im in enumerate(images):
    one = _pre_launch(pre, pre.pack([im], None if aug is None else aug[i:i + 1], None if crop is None else crop[i:i + 1],
                                    mode_offsets=None if mode_offsets is None else mode_offsets[i:i + 1]))
    assert torch.equal(one.view(bits)[0], out.view(bits)[i]), '%s: image %d of the batch differs from the same image alone' % (what, i)


@pytest.mark.parametrize('cropping', [False, True], ids=['plain', 'cropping'])
@pytest.mark.parametrize('hw', [1, 2, 5, 16, 33])
def test_preprocess_kernel_elementwise(hw, cropping):
  """tg_preprocess_images_crop (csrc/preprocess.hip) against oracle.np_ops.preprocess_image, here and not in test_gpu_data.py so
  that it also runs over the emulated kernels: nine sources (_pre_sources) in one batch, targets of 1, 2, 5, 16 and 33 pixels
  (a ragged last workgroup at every one: hw^2 is no multiple of 256; 33^2 = 1089 takes five), PAD / CROP / RESHAPE, rgb / yiq /
  bgr / gray, fp32 / fp16 / bf16, without and with --do_random_cropping (planted rectangles: _pre_crops), flips alternating,
  the colour draws at the ends of their ranges.  Without cropping also the evaluation call (is_training=False: the kernel still
  runs saturate(c, 1) and the clip, so the bound is asserted, not equality)."""
  from twingan_amd import data as D
  images = _pre_sources()
  n = len(images)
  aug = _pre_aug(n)
  for mode in ('PAD', 'CROP', 'RESHAPE'):
    for cs in ('rgb', 'yiq', 'bgr', 'gray'):
      want, crop = None, None
      for dname in sorted(EW_DTYPES):
        pre = D.Preprocessor(hw, device='cpu', precision=PRE_PRECISION[dname], resize_mode=mode, do_random_cropping=cropping,
                             color_space=cs)
        if cropping:
          assert pre.crops and pre.mid == int(hw / 0.8)
          crop = _pre_crops(n, pre.mid, hw)
        if want is None:
          want = [N.preprocess_image(im, hw, mode, True, flip=bool(aug[i, 0]), saturation_first=bool(aug[i, 1]), delta=float(aug[i, 2]),
                                     factor=float(aug[i, 3]), crop=None if crop is None else tuple(crop[i]), color_space=cs)
                  for i, im in enumerate(images)]
        _pre_check('preprocess hw %d %s %s %s%s' % (hw, mode, cs, dname, ' cropping' if cropping else ''), dname, pre, images, want,
                   aug, crop)
      if not cropping and cs in ('rgb', 'yiq'):
        ev_want = [N.preprocess_image(im, hw, mode, False, color_space=cs) for im in images]
        for dname in sorted(EW_DTYPES):
          ev = D.Preprocessor(hw, device='cpu', precision=PRE_PRECISION[dname], resize_mode=mode, is_training=False, color_space=cs)
          _pre_check('preprocess evaluation hw %d %s %s %s' % (hw, mode, cs, dname), dname, ev, images, ev_want)


@pytest.mark.parametrize('hw', [1, 2, 5, 16, 33])
def test_preprocess_random_crop_and_reshape_elementwise(hw):
  """RANDOM_CROP_AND_RESHAPE with initial_crop_hw = hw (the second resize is 1 : 1) and hw + 7: a source smaller than the window
  is resized up to it whole, a larger one gives a window at a planted corner (first / last possible offset)."""
  from twingan_amd import data as D
  images = _pre_sources()
  aug = _pre_aug(len(images))
  for c in (hw, hw + 7):
    offs = [None if c > min(im.shape[:2]) else ((0, 0) if i % 2 else (im.shape[0] - c, im.shape[1] - c)) for i, im in enumerate(images)]
    want = [N.preprocess_image(im, hw, 'RANDOM_CROP_AND_RESHAPE', True, flip=bool(aug[i, 0]), saturation_first=bool(aug[i, 1]),
                               delta=float(aug[i, 2]), factor=float(aug[i, 3]), mode_offset=offs[i] or (0, 0), initial_crop_hw=c)
            for i, im in enumerate(images)]
    for dname in sorted(EW_DTYPES):
      pre = D.Preprocessor(hw, device='cpu', precision=PRE_PRECISION[dname], resize_mode='RANDOM_CROP_AND_RESHAPE', initial_crop_hw=c)
      _pre_check('preprocess window %d -> %d %s' % (c, hw, dname), dname, pre, images, want, aug, mode_offsets=offs)


def test_preprocess_kernel_refuses_what_it_cannot_run():
  """color_space = 4 and a crop table with an intermediate image smaller than the output (mid < hw: an up-sampling crop is not
  built) are refused; the output keeps its fill."""
  from twingan_amd import data as D
  from twingan_amd._lib import TgError
  images = _pre_sources()[:4]
  pre = D.Preprocessor(5, device='cpu', precision='fp32', resize_mode='RESHAPE', do_random_cropping=True)
  tables = pre.pack(images, _pre_aug(4), _pre_crops(4, pre.mid, 5))
  with pytest.raises(TgError):
    _pre_launch(pre, tables, color_space=4)
  with pytest.raises(TgError):
    _pre_launch(pre, tables, mid=4)
  assert bool(torch.isfinite(_pre_launch(pre, tables)).all())
