"""GPU: the twice-differentiable conv nodes of the gradient-penalty pass, each alone and element by element, and the
"premask" handshake between them.

The nodes (twingan_amd/ops.py): ConvBwdDataFn, MaskedDgradFn, UnpoolMaskedDgradFn, LReluPoolBwdFn, LReluBwdFn, and the
second-order branch of PointwiseConvFn.  Every kernel they launch is checked at first order in tests/test_gpu_ops.py; what
is checked here is the host code: which tensor a node masks with, whether a mask is applied once, what the filter gradient
is formed from, and that the routing of _conv_backward hands every LeakyReLU mask to exactly one launch.

Part 1 calls Node.apply on leaf tensors.  The mask operands are INDEPENDENT random tensors with planted +0.0 and -0.0 (both
"not positive": slope alpha), so that a swap of two masks moves about 40 % of the elements by a factor of 5.  The reference
is float64 numpy (oracle/np_ops.py) on the operands as stored; where a route stores an intermediate (vm = rnd(v m(x_act)),
g = rnd(0.25 up2(gzp) m(z))) the reference is fed the tensor the same kernel stores for the same operands, itself checked
against its own bound, so that rounding is an input and not an error.  Bounds are tests/elementwise.py's, nothing new:
  dgrad / conv of the cotangent   conv_bound with K = k k cout / k k cin, + 1 per epilogue multiply, + u |ref| (_twice) where
                                  the route stores before it masks
  filter gradients                wgrad_bound over P = n ho wo pixels
  pooled cotangent                the mean of four STORED values: u |ref| + (1 + u) pool4(bound of the stored tensor)
Once per node the closed form used here is held to float64 torch.autograd on the composed expression.

Part 2 runs the trainer's flow over a discriminator-shaped chain for every setting of (USE_GP_PREMASK, USE_DGRAD_UNPOOL_GP)
and asserts by device pointer that every layer's activation is used as a mask exactly once in the second backward.
"""
import contextlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import np_ops as N          # noqa: E402  (checker only)
import elementwise as E                 # noqa: E402
import test_gpu_ops as T                # noqa: E402  (dev / host / rounding / the [elementwise] bookkeeping)
from test_gpu_ops import ops, record_calls      # noqa: E402,F401  (fixtures)

ALPHA = float(np.float32(0.2))
DT = T.EW_DTYPES


def m(t):
  """The LeakyReLU derivative as the kernels take it: z > 0 ? 1 : alpha (+0.0 and -0.0 are not positive)."""
  return np.where(np.asarray(t) > 0, 1.0, ALPHA)


def _mask_tensor(rng, shape, dtype):
  """An independent random mask source of the storage type with planted zeros: every 7th element +0.0, every 11th -0.0."""
  a = T._round_dt(rng.randn(*shape), dtype).astype(np.float32)
  flat = a.reshape(-1)
  flat[::7] = 0.0
  flat[3::11] = -0.0
  t = torch.from_numpy(a).to(T.dev()).to(dtype).contiguous()
  assert bool((t == 0).any()) and bool(torch.signbit(t[t == 0]).any()) and not bool(torch.signbit(t[t == 0]).all())
  return t


def _dev(a, dtype):
  return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(T.dev()).to(dtype).contiguous()


def _operands(seed, n, hw, cin, cout, k, padding, dtype):
  """Leaves of one conv layer x [n, hw, hw, cin] -> y [n, ho, ho, cout]: gy, the fp32 master kernel holding values of the
  storage type, the cotangent v of the input's shape, the two mask sources."""
  rng = np.random.RandomState(seed)
  ho = hw if padding == 'SAME' else hw - k + 1
  gy = _dev(rng.randn(n, ho, ho, cout), dtype)
  w = torch.from_numpy(T._round_dt(rng.randn(k, k, cin, cout) / np.sqrt(k * k * cin), dtype).astype(np.float32)).to(T.dev()).contiguous()
  v = _dev(rng.randn(n, hw, hw, cin), dtype)
  x_act = _mask_tensor(rng, (n, hw, hw, cin), dtype)
  out_act = _mask_tensor(rng, (n, ho, ho, cout), dtype)
  return gy, w, v, x_act, out_act, ho


@contextlib.contextmanager
def _spy():
  """-> list of (entry point, args, kernel the dispatch picked) of every library call inside the block."""
  import twingan_amd.ops as O
  real, seen = O.call, []

  def spy(name, *a, **kw):
    r = real(name, *a, **kw)
    seen.append((name, a, T._last_kernel()))
    return r
  O.call = spy
  try:
    yield seen
  finally:
    O.call = real


def _names(seen):
  return [s[0] for s in seen]


def _pool4(a):
  n, h, w, c = a.shape
  return a.reshape(n, h // 2, 2, w // 2, 2, c).mean(axis=(2, 4))


def _pooled_bound(ref_full, bound_full, dtype):
  """The mean of four STORED values, each within its own bound, rounded once more (as `fwd_pool pooled`)."""
  u = E.unit_roundoff(dtype)
  return u * np.abs(_pool4(ref_full)) + (1 + u) * _pool4(bound_full) + E.tiny(dtype)


def _masked_store(O, t, src, what, dname):
  """rnd(t m(src)) as tg_lrelu_bwd stores it for these operands -- the tensor a node's backward reads after its own mask
  launch -- checked against its bound (one fp32 multiply, one storage rounding) and returned as float64."""
  got = T.host(O.lrelu_bwd_raw(t, src, 0.2))
  ref = T.host(t) * m(T.host(src))
  T._ew_note('gp node stored mask', dname, E.assert_elementwise(got, ref, T._f32_ops_bound(ref, np.abs(ref), 1, t.dtype), what))
  return got


# ------------------------------------------------------------------------------------------------ float64 torch cross-checks
def _t64(a):
  return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def _torch_dgrad_second_order(gy, w, v, padding, x_shape, x_mask=None, unpool=None):
  """float64 torch.autograd on the composed expression out = dgrad(g, w) [m(x_act)], g = gy or 0.25 up2(gzp) m(z), the dgrad
  itself taken as the gradient of torch's own conv2d -> (out, d<out, v>/d gy-or-gzp, d<out, v>/dw) as numpy.
  unpool = m(z) as an array: `gy` is then the pooled gradient."""
  import torch.nn.functional as F
  gyt, wt = _t64(gy).requires_grad_(True), _t64(w).requires_grad_(True)
  k = w.shape[0]
  g = gyt
  if unpool is not None:
    g = 0.25 * gyt.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2) * _t64(unpool)
  x0 = torch.zeros(x_shape, dtype=torch.float64, requires_grad=True)
  y = F.conv2d(x0.permute(0, 3, 1, 2), wt.permute(3, 2, 0, 1), padding=(k - 1) // 2 if padding == 'SAME' else 0).permute(0, 2, 3, 1)
  out, = torch.autograd.grad(y, x0, g, create_graph=True)
  if x_mask is not None:
    out = out * _t64(x_mask)
  a, b = torch.autograd.grad(out, [gyt, wt], _t64(v))
  return out.detach().numpy(), a.numpy(), b.numpy()


def _close64(a, b, what):
  assert np.allclose(a, b, rtol=1e-10, atol=1e-12), (what, float(np.abs(a - b).max()))


# ------------------------------------------------------------------------------------------------ part 1: the conv nodes
NODE_CASES = [
    # id, kernel family, n, hw, cin, cout, k, padding, dtypes, cross-check the closed form against torch here
    ('small_4x4', 'conv_small', 3, 4, 32, 32, 3, 'SAME', ('bf16', 'f16'), True),
    ('small_dense_4x4_valid', 'conv_small', 5, 4, 32, 32, 4, 'VALID', ('bf16', 'f16'), False),
    ('img_8x8', 'conv_img', 3, 8, 64, 32, 3, 'SAME', ('bf16', 'f16'), False),
    ('tile_16x16_c16_32', 'conv_tile', 2, 16, 16, 32, 3, 'SAME', ('bf16', 'f16'), False),
    ('tile_32x32_c32_64_n3', 'conv_tile', 3, 32, 32, 64, 3, 'SAME', ('bf16', 'f16'), False),
    ('tile_16x16_c32_48', 'conv_tile', 2, 16, 32, 48, 3, 'SAME', ('bf16', 'f16'), False),
    ('direct_6x6_k3', 'direct', 2, 6, 5, 7, 3, 'SAME', ('f32',), True),
    ('direct_7x7_k4_valid', 'direct', 2, 7, 3, 5, 4, 'VALID', ('f32',), True),
    ('direct_5x5_k1', 'direct', 2, 5, 4, 6, 1, 'SAME', ('f32',), False),
]
NODE_PARAMS = [pytest.param(c, d, id='%s-%s' % (c[0], d)) for c in NODE_CASES for d in c[8]]
UNPOOL_PARAMS = [pytest.param(c, d, id='%s-%s' % (c[0], d)) for c in NODE_CASES for d in c[8] if c[1] == 'conv_tile']


def _conv_refs(v, w, gy, k, padding):
  """conv(v, w), its magnitude, wgrad(v, gy), its magnitude (float64, oracle/np_ops.py)."""
  return (N.conv2d_gemm(v, w, padding), N.conv2d_gemm(np.abs(v), np.abs(w), padding),
          N.conv2d_bwd_weight_gemm(v, gy, (k, k), padding), N.conv2d_bwd_weight_gemm(np.abs(v), np.abs(gy), (k, k), padding))


def _check_second_order(O, what, dname, family, seen, ggy, gw, vm, wn, gyn, k, padding, out_slope, pooled_with=None):
  """ggy = conv(vm, w) [m(out_act)] (pooled_with: -> pool2(rnd(conv(vm, w) m(z)))) and gw = wgrad(vm, gy) against the oracle on
  the operands the kernels read; the conv of the cotangent ran in `family` and masked in its own epilogue."""
  dtype = ggy.dtype
  cin, cout = wn.shape[2], wn.shape[3]
  lin, lmag, rw, rwmag = _conv_refs(vm, wn, gyn, k, padding)
  convs = [s for s in seen if s[0] in ('tg_conv2d_fwd', 'tg_conv2d_fwd_masked')]
  assert len(convs) == 1 and family in convs[0][2], (what, [(s[0], s[2]) for s in seen])
  slope = out_slope if pooled_with is None else pooled_with
  if slope is None:
    assert convs[0][0] == 'tg_conv2d_fwd', (what, _names(seen))
    ref, bound = lin, E.conv_bound(lin, lmag, k * k * cin, dtype)
  else:
    assert convs[0][0] == 'tg_conv2d_fwd_masked', (what, _names(seen))      # the raw masked kernel: gradients are off here
    ref = lin * slope
    bound = E.conv_bound(ref, lmag * slope, k * k * cin + 1, dtype, T._twice(ref, slope, dtype))
  if pooled_with is not None:
    ref, bound = _pool4(ref), _pooled_bound(ref, bound, dtype)
  T._ew_note('gp node d/dgy ' + family, dname, E.assert_elementwise(T.host(ggy), ref, bound, what + ' d/dgy'))
  P = gyn.shape[0] * gyn.shape[1] * gyn.shape[2]
  T._ew_note('gp node d/dw ' + family, dname, E.assert_elementwise(T.host(gw), rw, E.wgrad_bound(rw, rwmag, P), what + ' d/dw'))
  return lin, rw


@pytest.mark.parametrize('case,dname', NODE_PARAMS)
def test_conv_bwd_data_node_first_and_second_order(ops, case, dname):
  """ConvBwdDataFn(gy, w, x_shape, spec, out_act): out = dgrad(gy, w); with the cotangent v, d/dgy = conv(v, w) [m(out_act)]
  and d/dw = wgrad(v, gy) -- the filter gradient pairs the COTANGENT with gy, and out_act masks d/dgy only."""
  import twingan_amd.ops as O
  cid, family, n, hw, cin, cout, k, padding, _, cross = case
  dtype = DT[dname]
  gy, w, v, x_act, out_act, ho = _operands(1000 + NODE_CASES.index(case), n, hw, cin, cout, k, padding, dtype)
  spec = O.ConvSpec(k, padding)
  gyn, wn, vn = T.host(gy), T.host(w), T.host(v)
  ref1 = N.conv2d_bwd_data_gemm(gyn, wn, (hw, hw), padding)
  mag1 = N.conv2d_bwd_data_gemm(np.abs(gyn), np.abs(wn), (hw, hw), padding)
  for act in (None, out_act):
    what = 'ConvBwdDataFn %s %s out_act=%s' % (cid, dname, act is not None)
    O.GradSink.clear()
    gyl, wl = gy.clone().requires_grad_(True), w.clone().requires_grad_(True)
    out = O.ConvBwdDataFn.apply(gyl, wl, (n, hw, hw, cin), spec, act)
    assert family in T._last_kernel(), (what, T._last_kernel())
    T._ew_note('gp node dgrad ' + family, dname, E.assert_elementwise(T.host(out), ref1, E.conv_bound(ref1, mag1, k * k * cout, dtype), what))
    with _spy() as seen:
      ggy, gw = torch.autograd.grad(out, [gyl, wl], v)
    assert 'tg_lrelu_bwd' not in _names(seen), (what, _names(seen))
    lin, rw = _check_second_order(O, what, dname, family, seen, ggy, gw, vn, wn, gyn, k, padding,
                                  None if act is None else m(T.host(act)))
  if cross:
    o64, a64, b64 = _torch_dgrad_second_order(gyn, wn, vn, padding, (n, hw, hw, cin))
    _close64(ref1, o64, cid + ' dgrad closed form')
    _close64(lin, a64, cid + ' d/dgy closed form')
    _close64(rw, b64, cid + ' d/dw closed form')


@pytest.mark.parametrize('case,dname', NODE_PARAMS)
def test_masked_dgrad_node_first_and_second_order(ops, case, dname):
  """MaskedDgradFn(gy, w, x_act, spec, out_act): out = dgrad(gy, w) m(x_act); the backward masks the cotangent with x_act
  ONCE (vm = rnd(v m(x_act)), or vm = v when the producer of v is flagged tg_v_premasked), d/dgy = conv(vm, w) [m(out_act)], d/dw
  = wgrad(vm, gy): both from the MASKED cotangent."""
  import twingan_amd.ops as O
  cid, family, n, hw, cin, cout, k, padding, _, cross = case
  dtype = DT[dname]
  gy, w, v, x_act, out_act, ho = _operands(1100 + NODE_CASES.index(case), n, hw, cin, cout, k, padding, dtype)
  spec = O.ConvSpec(k, padding)
  gyn, wn, vn = T.host(gy), T.host(w), T.host(v)
  xs = m(T.host(x_act))
  ref1 = N.conv2d_bwd_data_gemm(gyn, wn, (hw, hw), padding) * xs
  mag1 = N.conv2d_bwd_data_gemm(np.abs(gyn), np.abs(wn), (hw, hw), padding) * xs
  vm_stored = _masked_store(O, v, x_act, 'MaskedDgradFn %s %s vm' % (cid, dname), dname)
  for act in (None, out_act):
    O.GradSink.clear()
    gyl, wl = gy.clone().requires_grad_(True), w.clone().requires_grad_(True)
    out = O.MaskedDgradFn.apply(gyl, wl, x_act, spec, act)
    what = 'MaskedDgradFn %s %s out_act=%s' % (cid, dname, act is not None)
    assert family in T._last_kernel(), (what, T._last_kernel())
    T._ew_note('gp node dgrad_masked ' + family, dname, E.assert_elementwise(
        T.host(out), ref1, E.conv_bound(ref1, mag1, k * k * cout + 1, dtype, T._twice(ref1, xs, dtype)), what))
    for premasked in (False, True):
      if premasked:
        out.grad_fn.tg_v_premasked = True      # what the consumer of `out` sets after masking v in its own epilogue
      with _spy() as seen:
        ggy, gw = torch.autograd.grad(out, [gyl, wl], v, retain_graph=not premasked)
      masks = [s for s in seen if s[0] == 'tg_lrelu_bwd']
      assert len(masks) == (0 if premasked else 1), (what, premasked, _names(seen))
      if masks:
        assert masks[0][1][1] == x_act.data_ptr(), (what, 'the cotangent is masked with x_act')
      lin, rw = _check_second_order(O, what + ' premasked=%s' % premasked, dname, family, seen, ggy, gw,
                                    vn if premasked else vm_stored, wn, gyn, k, padding, None if act is None else m(T.host(act)))
      if cross and not premasked:      # the float64 composition masks without rounding: the closed form on v m(x_act)
        o64, a64, b64 = _torch_dgrad_second_order(gyn, wn, vn, padding, (n, hw, hw, cin), x_mask=xs)
        _close64(ref1, o64, cid + ' masked dgrad closed form')
        _close64(N.conv2d_gemm(vn * xs, wn, padding), a64, cid + ' d/dgy closed form')
        _close64(N.conv2d_bwd_weight_gemm(vn * xs, gyn, (k, k), padding), b64, cid + ' d/dw closed form')
        cross = False


@pytest.mark.parametrize('case,dname', UNPOOL_PARAMS)
def test_unpool_masked_dgrad_node_first_and_second_order(ops, case, dname):
  """UnpoolMaskedDgradFn(gzp, w, x_act, z, spec): g = rnd(0.25 up2(gzp) m(z)) -- the block end's own mask z -- and out = dgrad(g,
  w) m(x_act); backward: vm as MaskedDgradFn, d/dgzp = pool2(rnd(conv(vm, w) m(z))), d/dw = wgrad(vm, g).  Where cout is no
  multiple of 32 the kernels refuse the layer and the node must not be built (the two-node route: the test below)."""
  import twingan_amd.ops as O
  cid, family, n, hw, cin, cout, k, padding, _, _ = case
  dtype = DT[dname]
  gy, w, v, x_act, z, ho = _operands(1200 + NODE_CASES.index(case), n, hw, cin, cout, k, padding, dtype)
  spec = O.ConvSpec(k, padding)
  gzp = gy[:, ::2, ::2, :].contiguous()
  if cout % 32:
    assert not O._unpool_act_supported((n, hw, hw, cin), w, spec, dtype)
    assert O.conv_bwd_data_unpool_raw(gzp, z, w, x_act, (n, hw, hw, cin), spec, True) is None
    return
  assert O._unpool_act_supported((n, hw, hw, cin), w, spec, dtype)
  wn, vn = T.host(w), T.host(v)
  xs, zs = m(T.host(x_act)), m(T.host(z))
  # g as the kernel stores it (keep mode of the same launch), held to its own bound: a fused multiply and the slope
  g_stored = T.host(O.conv_bwd_data_unpool_raw(gzp, z, w, x_act, (n, hw, hw, cin), spec, True)[1])
  gref = 0.25 * T._up2(T.host(gzp)) * zs
  T._ew_note('gp node stored mask', dname, E.assert_elementwise(g_stored, gref, T._f32_ops_bound(gref, np.abs(gref), 2, dtype),
                                                                'UnpoolMaskedDgradFn %s %s g' % (cid, dname)))
  ref1 = N.conv2d_bwd_data_gemm(g_stored, wn, (hw, hw), padding) * xs
  mag1 = N.conv2d_bwd_data_gemm(np.abs(g_stored), np.abs(wn), (hw, hw), padding) * xs
  vm_stored = _masked_store(O, v, x_act, 'UnpoolMaskedDgradFn %s %s vm' % (cid, dname), dname)
  O.GradSink.clear()
  gzl, wl = gzp.clone().requires_grad_(True), w.clone().requires_grad_(True)
  out = O.UnpoolMaskedDgradFn.apply(gzl, wl, x_act, z, spec)
  what = 'UnpoolMaskedDgradFn %s %s' % (cid, dname)
  assert family in T._last_kernel() and 'unpoolz' in T._last_kernel(), (what, T._last_kernel())
  T._ew_note('gp node dgrad_unpool ' + family, dname, E.assert_elementwise(
      T.host(out), ref1, E.conv_bound(ref1, mag1, k * k * cout + 1, dtype, T._twice(ref1, xs, dtype)), what))
  for premasked in (False, True):
    if premasked:
      out.grad_fn.tg_v_premasked = True
    with _spy() as seen:
      ggzp, gw = torch.autograd.grad(out, [gzl, wl], v, retain_graph=not premasked)
    masks = [s for s in seen if s[0] == 'tg_lrelu_bwd']
    assert len(masks) == (0 if premasked else 1), (what, premasked, _names(seen))
    if masks:
      assert masks[0][1][1] == x_act.data_ptr(), (what, 'the cotangent is masked with x_act, not z')
    conv = [s for s in seen if s[0] == 'tg_conv2d_fwd_masked']
    assert len(conv) == 1 and conv[0][1][3] == z.data_ptr(), (what, 'the conv of the cotangent masks with z')
    _check_second_order(O, what + ' premasked=%s' % premasked, dname, family, seen, ggzp, gw, vn if premasked else vm_stored, wn,
                        g_stored, k, padding, None, pooled_with=zs)
  if n * hw * hw * cout <= 2 * 16 * 16 * 32:      # the closed form against float64 torch, at the node's smallest shape
    gzn = T.host(gzp)
    o64, a64, b64 = _torch_dgrad_second_order(gzn, wn, vn, padding, (n, hw, hw, cin), x_mask=xs, unpool=zs)
    _close64(N.conv2d_bwd_data_gemm(gref, wn, (hw, hw), padding) * xs, o64, cid + ' unpool dgrad closed form')
    _close64(_pool4(N.conv2d_gemm(vn * xs, wn, padding) * zs), a64, cid + ' d/dgzp closed form')
    _close64(N.conv2d_bwd_weight_gemm(vn * xs, gref, (k, k), padding), b64, cid + ' d/dw closed form')


def _graph_nodes(t):
  seen, stack = set(), [t.grad_fn]
  while stack:
    nd = stack.pop()
    if nd is None or nd in seen:
      continue
    seen.add(nd)
    stack.extend(f for f, _ in nd.next_functions)
  return [type(nd).__name__ for nd in seen]


@pytest.mark.parametrize('dname', ['bf16', 'f16'])
@pytest.mark.parametrize('cout', [32, 48])
def test_block_end_routes_to_one_node_only_where_the_kernels_take_it(ops, cout, dname):
  """_conv_backward over a pooled LeakyReLU block end under create_graph: UnpoolMaskedDgradFn where cout % 32 == 0, else
  LReluPoolBwdFn + MaskedDgradFn (2 x 16 x 16, 32 -> cout)."""
  import twingan_amd.ops as O
  dtype = DT[dname]
  g = torch.Generator().manual_seed(77)
  x = torch.randn(2, 16, 16, 16, generator=g).to(dtype).to(T.dev()).requires_grad_(True)
  w1 = (torch.randn(3, 3, 16, 32, generator=g) * 0.1).to(T.dev()).requires_grad_(True)
  w2 = (torch.randn(3, 3, 32, cout, generator=g) * 0.1).to(T.dev()).requires_grad_(True)
  O.GradSink.clear()
  with O.second_order():
    z1 = O.conv2d(x, w1, None, 3, 'SAME', lrelu=True)
    _, zp = O.conv2d(z1, w2, None, 3, 'SAME', lrelu=True, fuse_input_lrelu=True, pool=True, pool_only=True)
  with O.no_param_grads():
    gx, = torch.autograd.grad(zp.float().sum(), x, create_graph=True)
  names = _graph_nodes(gx)
  one = any('UnpoolMaskedDgradFn' in s for s in names)
  two = any('LReluPoolBwdFn' in s for s in names) and any(s.startswith('MaskedDgradFn') for s in names)
  assert one == (cout % 32 == 0) and two == (cout % 32 != 0), names


# ------------------------------------------------------------------------------------------------ the streaming nodes
POOL_SHAPES = [(3, 4, 4, 32), (2, 16, 16, 48), (3, 32, 32, 64), (2, 6, 6, 7)]


@pytest.mark.parametrize('dname', sorted(DT))
@pytest.mark.parametrize('shape', POOL_SHAPES, ids=['x'.join(map(str, s)) for s in POOL_SHAPES])
def test_lrelu_pool_bwd_and_lrelu_bwd_nodes_first_and_second_order(ops, shape, dname):
  """LReluPoolBwdFn(gzp, z, alpha): out = 0.25 up2(gzp) m(z); backward pool2(rnd(v m(z))), or pool2(v) when flagged
  tg_v_premasked (the conv that produced v masked it).  LReluBwdFn(g, z, alpha): out = g m(z), backward v m(z)."""
  import twingan_amd.ops as O
  dtype = DT[dname]
  n, h, w_, c = shape
  rng = np.random.RandomState(1300 + c)
  gzp, v = _dev(rng.randn(n, h // 2, w_ // 2, c), dtype), _dev(rng.randn(n, h, w_, c), dtype)
  z = _mask_tensor(rng, shape, dtype)
  zs, vn = m(T.host(z)), T.host(v)
  what = 'LReluPoolBwdFn %s %s' % (shape, dname)
  gl = gzp.clone().requires_grad_(True)
  out = O.LReluPoolBwdFn.apply(gl, z, 0.2)
  ref = 0.25 * T._up2(T.host(gzp)) * zs
  T._ew_note('gp node lrelu_pool_bwd', dname, E.assert_elementwise(T.host(out), ref, T._f32_ops_bound(ref, np.abs(ref), 2, dtype), what))
  vz_stored = _masked_store(O, v, z, what + ' v m(z)', dname)
  for premasked in (False, True):
    if premasked:
      out.grad_fn.tg_v_premasked = True
    with _spy() as seen:
      gg, = torch.autograd.grad(out, [gl], v, retain_graph=not premasked)
    masks = [s for s in seen if s[0] == 'tg_lrelu_bwd']
    assert len(masks) == (0 if premasked else 1) and all(s[1][1] == z.data_ptr() for s in masks), (what, premasked, _names(seen))
    src = vn if premasked else vz_stored
    ref2 = 0.25 * T._sum4(src)
    T._ew_note('gp node lrelu_pool_bwd bwd', dname, E.assert_elementwise(
        T.host(gg), ref2, T._sum4_bound(ref2, 0.25 * T._sum4(np.abs(src)), dtype), what + ' backward premasked=%s' % premasked))
  # closed form against float64 torch: out = 0.25 up2(gzp) m(z) is linear in gzp
  gt = _t64(T.host(gzp)).requires_grad_(True)
  o64 = 0.25 * gt.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2) * _t64(zs)
  a64, = torch.autograd.grad(o64, gt, _t64(vn))
  _close64(ref, o64.detach().numpy(), 'lrelu_pool_bwd closed form')
  _close64(0.25 * T._sum4(vn * zs), a64.numpy(), 'lrelu_pool_bwd backward closed form')
  # LReluBwdFn, first and second order: the same mask both times
  gfull = _dev(rng.randn(*shape), dtype).requires_grad_(True)
  out = O.LReluBwdFn.apply(gfull, z, 0.2)
  ref = T.host(gfull) * zs
  T._ew_note('gp node lrelu_bwd', dname, E.assert_elementwise(T.host(out), ref, T._f32_ops_bound(ref, np.abs(ref), 1, dtype),
                                                               'LReluBwdFn %s %s' % (shape, dname)))
  gg, = torch.autograd.grad(out, [gfull], v)
  ref = vn * zs
  T._ew_note('gp node lrelu_bwd', dname, E.assert_elementwise(T.host(gg), ref, T._f32_ops_bound(ref, np.abs(ref), 1, dtype),
                                                               'LReluBwdFn backward %s %s' % (shape, dname)))


@pytest.mark.parametrize('dname', sorted(DT))
@pytest.mark.parametrize('n,h,w_,c', [(3, 7, 5, 16), (2, 33, 31, 32)])
def test_pointwise_node_second_order_with_out_act(ops, n, h, w_, c, dname):
  """PointwiseConvFn at the fromRGB shape (3 -> c) with out_act, as its own create_graph backward builds it, and the backward
  of that node.  Narrow side out (g [.., c] -> [.., 3], W^T): the cotangent v [.., 3] goes through tg_pointwise_conv_fwd_masked,
  rnd(v W) m(out_act).  Wide side in (x [.., 3] -> [.., c]): the cotangent [.., c] is too wide for that kernel -- the plain
  pointwise conv, then LReluBwdFn with out_act.  K = the summed channels (fp32: products round, 2 K), + 1 for the slope."""
  import twingan_amd.ops as O
  dtype = DT[dname]
  rng = np.random.RandomState(1400 + c + n)
  u_st = E.unit_roundoff(dtype)
  wt = torch.from_numpy(T._round_dt(rng.randn(3, c) / np.sqrt(3), dtype).astype(np.float32)).to(T.dev()).contiguous()
  wn = T.host(wt)
  P = n * h * w_
  kk = (lambda s: s if dtype != torch.float32 else 2 * s)
  for narrow_out in (True, False):
    cin, cout = (c, 3) if narrow_out else (3, c)
    xin, v = _dev(rng.randn(n, h, w_, cin), dtype), _dev(rng.randn(n, h, w_, cout), dtype)
    act = _mask_tensor(rng, (n, h, w_, cin), dtype)
    W = wn.T if narrow_out else wn                         # [cin, cout]
    what = 'PointwiseConvFn %d>%d n%d %dx%d %s' % (cin, cout, n, h, w_, dname)
    O.GradSink.clear()
    xl, wl = xin.clone().requires_grad_(True), wt.clone().requires_grad_(True)
    out = O.PointwiseConvFn.apply(xl, wl, None, narrow_out, 0, 0.2, act)
    xn, vn = T.host(xin), T.host(v)
    lin, mag = xn @ W, np.abs(xn) @ np.abs(W)
    T._ew_note('gp node pointwise', dname, E.assert_elementwise(T.host(out), lin, E.conv_bound(lin, mag, kk(cin), dtype), what))
    with _spy() as seen:
      gx, gw = torch.autograd.grad(out, [xl, wl], v)
    names = _names(seen)
    slope = m(T.host(act))
    lin2, mag2 = vn @ W.T, np.abs(vn) @ np.abs(W.T)
    ref = lin2 * slope
    extra = (1 + u_st) * (u_st * np.abs(ref) + E.tiny(dtype)) * (slope != 1.0)      # stored, then masked and stored again
    if narrow_out:
      assert 'tg_pointwise_conv_fwd_masked' in names and 'tg_lrelu_bwd' not in names, (what, names)
      fm = [s for s in seen if s[0] == 'tg_pointwise_conv_fwd_masked'][0]
      assert fm[1][2] == act.data_ptr(), (what, 'masked with out_act')
    else:
      assert 'tg_pointwise_conv_fwd_masked' not in names and names.count('tg_lrelu_bwd') == 1, (what, names)
      assert [s for s in seen if s[0] == 'tg_lrelu_bwd'][0][1][1] == act.data_ptr(), (what, 'masked with out_act')
    T._ew_note('gp node pointwise d/dx', dname, E.assert_elementwise(
        T.host(gx), ref, E.conv_bound(ref, mag2 * slope, kk(cout) + 1, dtype, extra), what + ' d/dx'))
    # d/dw [3, c]: the cotangent paired with the node's own input, UNMASKED (out_act belongs to the producer of x)
    a, b = (vn, xn) if narrow_out else (xn, vn)
    rw = a.reshape(-1, 3).T @ b.reshape(-1, c)
    rwmag = np.abs(a).reshape(-1, 3).T @ np.abs(b).reshape(-1, c)
    T._ew_note('gp node pointwise d/dw', dname, E.assert_elementwise(T.host(gw), rw, E.wgrad_bound(rw, rwmag, kk(P)), what + ' d/dw'))
    if n == 3:      # the closed form against float64 torch
      xt, wtt = _t64(xn).requires_grad_(True), _t64(wn).requires_grad_(True)
      o64 = xt @ (wtt.t() if narrow_out else wtt)
      a64, b64 = torch.autograd.grad(o64, [xt, wtt], _t64(vn))
      _close64(lin, o64.detach().numpy(), what + ' closed form')
      _close64(lin2, a64.numpy(), what + ' d/dx closed form')
      _close64(rw, b64.numpy(), what + ' d/dw closed form')


# ------------------------------------------------------------------------------------------------ part 2: the handshake
# entry point -> position of the mask source among its arguments (after the name): every way a LeakyReLU mask is applied
MASK_SLOT = {'tg_lrelu_bwd': 1, 'tg_lrelu_bwd_bias': 1, 'tg_lrelu_pool_bwd': 2, 'tg_conv2d_fwd_masked': 3,
             'tg_pointwise_conv_fwd_masked': 2, 'tg_conv2d_bwd_data_masked': 3}
EPILOGUE = ('tg_conv2d_fwd_masked', 'tg_pointwise_conv_fwd_masked')
CHAIN_N, CHAIN_HW, CHAIN_C = 3, 32, (16, 32, 32, 32)
# The first seed for which the float64 reference alone meets the cap of 1e-5 on mask ties: no stored activation of either
# topology, in either type, has another sign than its float64 pre-activation (0 of 270336 and of 172032; checked on the host
# over the emulated kernels and again on an MI355X -- the test prints the count).  17 / 19 / 2 / 7 pre-activations lie INSIDE
# their accumulation bound at this seed and could have gone either way; none did
CHAIN_SEED = 0
# rel-L2 of the penalty's parameter gradients (w0 .. w3) against the float64 reference with every flag OFF, measured on an
# MI355X; every route is asserted within 2 x these (one more rounding per fused layer)
REL_L2_ALL_OFF = {
    'plain': {'bf16': [5.55e-4, 6.82e-4, 6.43e-4, 3.98e-4], 'f16': [1.22e-4, 1.43e-4, 1.41e-4, 9.58e-5]},
    'residual': {'bf16': [2.35e-4, 2.16e-4, 2.00e-4, 2.28e-4], 'f16': [8.07e-5, 8.78e-5, 7.95e-5, 5.47e-5]},
}


class _RE:
  """A float64 reference tensor with the element-wise bound of everything computed so far."""

  def __init__(self, ref, err):
    self.ref, self.err = ref, err


def _st_mask(t, slope, nops, dtype):
  """A streaming launch: t * slope with `nops` fp32 operations, stored."""
  ref, err = t.ref * slope, t.err * slope
  return _RE(ref, err + T._f32_ops_bound(np.abs(ref) + err, np.abs(ref) + err, nops, dtype))


def _st_dgrad(t, w, hw, dtype, slope=None):
  """conv^T(t, w) [m(x_act)]: the error so far goes through |w|; the launch's own bound is conv_bound on what it read.  With
  a mask: K + 1 and the second storage rounding (_twice) -- it covers the epilogue route and the separate mask launch."""
  k, cout = w.shape[0], w.shape[3]
  ref = N.conv2d_bwd_data_gemm(t.ref, w, (hw, hw), 'SAME')
  perr = N.conv2d_bwd_data_gemm(t.err, np.abs(w), (hw, hw), 'SAME')
  mag = N.conv2d_bwd_data_gemm(np.abs(t.ref) + t.err, np.abs(w), (hw, hw), 'SAME')
  if slope is None:
    return _RE(ref, perr + E.conv_bound(np.abs(ref) + perr, mag, k * k * cout, dtype))
  ref, perr, mag = ref * slope, perr * slope, mag * slope
  return _RE(ref, perr + E.conv_bound(np.abs(ref) + perr, mag, k * k * cout + 1, dtype, T._twice(np.abs(ref) + perr, slope, dtype)))


def _st_pw(t, W, dtype):
  """t @ W (the fromRGB layer's backward-data: 16 -> 3 channels), K = the summed channels."""
  ref, perr = t.ref @ W, t.err @ np.abs(W)
  mag = (np.abs(t.ref) + t.err) @ np.abs(W)
  return _RE(ref, perr + E.conv_bound(np.abs(ref) + perr, mag, W.shape[0], dtype))


def _st_up(t):
  """0.25 up2: exact."""
  return _RE(0.25 * T._up2(t.ref), 0.25 * T._up2(t.err))


def _st_sum(a, b, dtype):
  """The framework's accumulation of two gradients of one tensor: one addition, stored."""
  ref, err = a.ref + b.ref, a.err + b.err
  mag = np.abs(a.ref) + np.abs(b.ref) + err
  return _RE(ref, err + T._f32_ops_bound(np.abs(ref) + err, mag, 1, dtype))


def _chain_operands(seed, dtype, topology):
  g = torch.Generator().manual_seed(9000 + seed)
  c0, c1, c2, c3 = CHAIN_C if topology == 'plain' else (16, 16, 16, 32)
  x = torch.randn(CHAIN_N, CHAIN_HW, CHAIN_HW, 3, generator=g).to(dtype).to(T.dev())
  shapes = [(1, 1, 3, c0), (3, 3, c0, c1), (3, 3, c1, c2), (3, 3, c2, c3)]
  ws = [(torch.randn(*s, generator=g) * (2.0 / (s[0] * s[1] * s[2])) ** 0.5).to(dtype).float().to(T.dev()).contiguous() for s in shapes]
  bs = [(torch.randn(s[3], generator=g) * 0.1).to(dtype).float().to(T.dev()) for s in shapes]
  return x, ws, bs


def _forward_chain(O, topology, xin, ps, bl, fuse):
  """-> (output, the activations whose LeakyReLU masks the backward passes need, in layer order, the inputs of each layer).
  plain: fromRGB -> conv -> conv + pool -> conv, the discriminator's first block (pggan.discriminator_before_fc).
  residual: what use_res_block builds -- a0 is read by the block's first conv AND by the skip add; fuse_input_lrelu is off
  there (pggan._d_conv), `fuse`: on for the one conv whose input does have a single consumer."""
  a0 = O.pointwise_conv(xin, ps[0], bl[0], lrelu=True)
  if topology == 'plain':
    a1 = O.conv2d(a0, ps[1], bl[1], 3, 'SAME', lrelu=True, fuse_input_lrelu=True)
    z2, p2 = O.conv2d(a1, ps[2], bl[2], 3, 'SAME', lrelu=True, fuse_input_lrelu=True, pool=True, pool_only=True)
    assert z2 is not None
  else:
    a1 = O.conv2d(a0, ps[1], bl[1], 3, 'SAME', lrelu=True)
    z2 = O.conv2d(a1, ps[2], bl[2], 3, 'SAME', lrelu=True, fuse_input_lrelu=fuse)
    p2 = O.avg_pool2(O.add(a0, z2))
  a3 = O.conv2d(p2, ps[3], bl[3], 3, 'SAME', lrelu=True, fuse_input_lrelu=True)
  return a3, [a0, a1, z2, a3], [xin, a0, a1, p2]


def _run_chain(O, monkeypatch, calls, topology, x, ws, bs, premask, one_node, skip_params=True, fuse=False):
  """`calls`: the record_calls fixture's list; the library calls of the SECOND backward are cut out of it."""
  monkeypatch.setattr(O, 'USE_GP_PREMASK', premask)
  monkeypatch.setattr(O, 'USE_DGRAD_UNPOOL_GP', one_node)
  O.GradSink.clear()
  ps = [t.clone().requires_grad_(True) for t in ws]
  bl = [t.clone().requires_grad_(True) for t in bs]
  xin = O.first_order_only(x.clone().requires_grad_(True))
  with O.second_order():
    a3, acts, ins = _forward_chain(O, topology, xin, ps, bl, fuse)
  ones = O.fill(a3.shape, 1.0, a3.dtype, a3.device)
  flow = {}      # the gradient the first backward hands to each layer's input, as stored (tensor hooks)
  hooks = [t.register_hook(lambda g, key=key: flow.__setitem__(key, g.detach())) for key, t in zip(('a0', 'a1', 'p2'), ins[1:])]
  with (O.no_param_grads() if skip_params else contextlib.nullcontext()):
    gx, = torch.autograd.grad(a3, xin, grad_outputs=ones, create_graph=True)
  for h in hooks:
    h.remove()
  flagged, stack, seen_nodes = set(), [gx.grad_fn], set()
  while stack:
    nd = stack.pop()
    if nd is None or nd in seen_nodes:
      continue
    seen_nodes.add(nd)
    if getattr(nd, 'tg_v_premasked', False):
      flagged.add(nd.tg_masks_with[0])
    cls = type(nd).__name__
    if cls.startswith('ConvBwdDataFn') and nd.saved_tensors[1].data_ptr() == ps[3].data_ptr():
      flow['g3'] = nd.saved_tensors[0].detach()      # ones m(a3), as the top layer's backward-data read it
    if cls.startswith(('UnpoolMaskedDgradFn', 'MaskedDgradFn')) and nd.saved_tensors[1].data_ptr() == ps[2].data_ptr():
      flow['g2'] = nd.saved_tensors[0].detach()      # the block end's gradient, as its backward-data read (or wrote) it
    stack.extend(f for f, _ in nd.next_functions)
  last_in = gx.grad_fn.saved_tensors[0].detach()      # what the last kernel of the first backward read (fromRGB's backward-data)
  pen = ((gx.float().pow(2).sum(dim=(1, 2, 3)).sqrt() - 1.0) ** 2).mean()
  mark = len(calls)
  grads = torch.autograd.grad(pen, ps)
  seen = calls[mark:]
  return dict(gx=gx.detach(), grads=[t.detach() for t in grads], acts=[t.detach() for t in acts], ins=[t.detach() for t in ins],
              seen=seen, flagged=flagged, last_in=last_in, flow=flow, nodes=[type(nd).__name__ for nd in seen_nodes])


def _assert_every_mask_exactly_once(r, want_epilogue, what):
  """By device pointer: every activation is the mask source of exactly one launch of the second backward -- a LeakyReLU
  launch or a masked conv epilogue -- and appears in no other launch; the flagged producers skipped theirs."""
  ptrs = [t.data_ptr() for t in r['acts']]
  in_epilogue = set()
  for li, p in enumerate(ptrs):
    uses = [(name, [i for i, a in enumerate(args) if isinstance(a, int) and a == p]) for name, args in r['seen']]
    uses = [(name, pos) for name, pos in uses if pos]
    assert all(name in MASK_SLOT and pos == [MASK_SLOT[name]] for name, pos in uses), (what, 'layer %d activation read outside a mask slot' % li, uses)
    assert len(uses) == 1, '%s: the LeakyReLU mask of layer %d is applied %d times in the second backward: %s' % (what, li, len(uses), uses)
    if uses[0][0] in EPILOGUE:
      in_epilogue.add(li)
    if p in r['flagged']:
      assert uses[0][0] in EPILOGUE, (what, 'layer %d: its node is flagged tg_v_premasked and still launched' % li, uses)
  assert r['flagged'] <= set(ptrs), (what, 'a flagged node masks with a tensor that is no activation of the chain')
  # ... and the pass does nothing else: the forward's own nodes are reached with an undefined gradient (the penalty depends on the
  # activations through masks only) and must launch nothing -- one filter gradient per layer, no backward-data, no bias sums
  names = _names(r['seen'])
  idle = [s for s in names if s.startswith(('tg_conv2d_bwd_data', 'tg_channel_sum', 'tg_pool2x2_bwd', 'tg_lrelu_pool_bwd', 'tg_lrelu_bwd_bias',
                                            'tg_pointwise_conv_bwd_weight_bias'))]
  assert not idle and names.count('tg_pointwise_conv_bwd_weight') == 1 and names.count('tg_conv2d_bwd_weight') == 3, (what, names)
  assert in_epilogue == set(want_epilogue), (what, 'masks in conv epilogues: layers %s, expected %s' % (sorted(in_epilogue), sorted(want_epilogue)))


def _chain_reference(topology, r, ws, bs, dtype):
  """float64, layer by layer on the operands as STORED: the pre-activation of every layer from the stored input of that layer
  (its sign is the mask the kernels ought to have stored; `ties`: where it lies inside its own accumulation bound), then the
  first backward as a chain of linear stages with the bound of every launch carried along (_RE).  -> gx (_RE), the same with
  the device's own stored signs (equal unless there are ties), the tie count and the masks."""
  wn, bn = [T.host(w) for w in ws], [T.host(b) for b in bs]
  ins, acts = [T.host(t) for t in r['ins']], [T.host(t) for t in r['acts']]
  pre, tie = [], []
  for li in range(4):
    if li == 0:
      lin, mag, K = ins[0] @ wn[0][0, 0], np.abs(ins[0]) @ np.abs(wn[0][0, 0]), 3
    else:
      lin, mag, K = N.conv2d_gemm(ins[li], wn[li], 'SAME'), N.conv2d_gemm(np.abs(ins[li]), np.abs(wn[li]), 'SAME'), 9 * wn[li].shape[2]
    p = lin + bn[li]
    pre.append(p)
    tie.append(np.abs(p) <= (K + 2) * E.U32 * (mag + np.abs(bn[li])) + E.tiny(dtype))
  outs = []
  for masks in ([m(p) for p in pre], [m(a) for a in acts]):
    hw2 = CHAIN_HW // 2
    t = _st_mask(_RE(np.ones_like(masks[3]), np.zeros_like(masks[3])), masks[3], 1, dtype)      # ones m(a3)
    t = _st_dgrad(t, wn[3], hw2, dtype)
    t = _st_up(t)
    if topology == 'plain':
      t = _st_mask(t, masks[2], 2, dtype)                                  # g = rnd(0.25 up2 m(z2))
      t = _st_dgrad(t, wn[2], CHAIN_HW, dtype, masks[1])
      t = _st_dgrad(t, wn[1], CHAIN_HW, dtype, masks[0])
    else:
      skip = t                                                             # the add hands the same gradient to both branches
      t = _st_mask(t, masks[2], 1, dtype)
      t = _st_dgrad(t, wn[2], CHAIN_HW, dtype, masks[1])
      t = _st_dgrad(t, wn[1], CHAIN_HW, dtype)
      t = _st_mask(_st_sum(t, skip, dtype), masks[0], 1, dtype)
    outs.append(_st_pw(t, wn[0][0, 0].T, dtype))
  return outs[0], outs[1], tie, pre, acts


def _chain_torch64(topology, masks, ws):
  """The first backward with the masks as constants, then the penalty and its parameter gradients, by float64 torch.autograd."""
  import torch.nn.functional as F
  wt = [_t64(T.host(w)).requires_grad_(True) for w in ws]
  mk = [_t64(a) for a in masks]
  dg = lambda g, w: F.conv_transpose2d(g.permute(0, 3, 1, 2), w.permute(3, 2, 0, 1), padding=1).permute(0, 2, 3, 1)
  up = lambda g: 0.25 * g.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
  t = up(dg(mk[3], wt[3]))
  if topology == 'plain':
    t = dg(dg(t * mk[2], wt[2]) * mk[1], wt[1]) * mk[0]
  else:
    t = (dg(dg(t * mk[2], wt[2]) * mk[1], wt[1]) + t) * mk[0]
  gx = t @ wt[0][0, 0].t()
  pen = ((gx.pow(2).sum(dim=(1, 2, 3)).sqrt() - 1.0) ** 2).mean()
  grads = torch.autograd.grad(pen, wt)
  return gx.detach().numpy(), [g.numpy() for g in grads]


def _plain_stages_check(r, ws, dtype, dname, what):
  """The first backward of the plain chain, launch by launch on the tensors as STORED (the gradient each layer's input
  received: tensor hooks; g3 and g2: what the backward-data nodes saved): every stage against float64 on the stored output of
  the stage before it, with that launch's own bound -- the node checks of part 1 in place, the layers' own activations as
  masks."""
  wn = [T.host(w) for w in ws]
  a0, a1, z2, a3 = (m(T.host(t)) for t in r['acts'])
  f = {k: T.host(v) for k, v in r['flow'].items()}
  assert set(f) == {'g3', 'p2', 'g2', 'a1', 'a0'}, (what, sorted(f))
  hw, hw2 = CHAIN_HW, CHAIN_HW // 2
  note = lambda name, got, ref, bound: T._ew_note('gp chain stage ' + name, dname, E.assert_elementwise(got, ref, bound, '%s stage %s' % (what, name)))
  note('ones m(a3)', f['g3'], a3, T._f32_ops_bound(a3, a3, 1, dtype))

  def dgrad(g, w, hw_, slope=None):
    ref = N.conv2d_bwd_data_gemm(g, w, (hw_, hw_), 'SAME')
    mag = N.conv2d_bwd_data_gemm(np.abs(g), np.abs(w), (hw_, hw_), 'SAME')
    K = 9 * w.shape[3]
    if slope is None:
      return ref, E.conv_bound(ref, mag, K, dtype)
    ref = ref * slope
    return ref, E.conv_bound(ref, mag * slope, K + 1, dtype, T._twice(ref, slope, dtype))
  note('dgrad w3', f['p2'], *dgrad(f['g3'], wn[3], hw2))
  ref = 0.25 * T._up2(f['p2']) * z2
  note('unpool m(z2)', f['g2'], ref, T._f32_ops_bound(ref, np.abs(ref), 2, dtype))
  note('dgrad w2 m(a1)', f['a1'], *dgrad(f['g2'], wn[2], hw, a1))
  note('dgrad w1 m(a0)', f['a0'], *dgrad(f['a1'], wn[1], hw, a0))
  W = wn[0][0, 0].T
  ref = f['a0'] @ W
  note('fromRGB^T', T.host(r['gx']), ref, E.conv_bound(ref, np.abs(f['a0']) @ np.abs(W), W.shape[0], dtype))


SETTINGS = [(False, False), (True, False), (False, True), (True, True)]
# layers whose mask sits in a conv epilogue in the second backward, per (USE_GP_PREMASK, USE_DGRAD_UNPOOL_GP): the one-node
# block end masks the conv of its cotangent with z2 whatever the premask flag says; premasking moves a0's and a1's as well
PLAIN_EPILOGUE = {(False, False): (), (True, False): (0, 1, 2), (False, True): (2,), (True, True): (0, 1, 2)}


def _chain_check(O, monkeypatch, calls, topology, dname, runs, what, base=None):
  """runs: list of (label, kwargs of _run_chain, layers expected in epilogues); the first is the all-off route."""
  dtype = DT[dname]
  base = base or {}      # run index -> index of its all-off route (default: the first run)
  x, ws, bs = _chain_operands(CHAIN_SEED, dtype, topology)
  res = []
  for label, kw, want in runs:
    r = _run_chain(O, monkeypatch, calls, topology, x, ws, bs, **kw)
    _assert_every_mask_exactly_once(r, want, '%s %s %s' % (what, dname, label))
    res.append(r)
  off = res[0]
  # ---- every route against the all-off route of the same forward pass (`base`): the first backward launches the same
  # kernels on the same operands there; its last kernel is fromRGB's backward-data (K = 16)
  w0 = ws[0][0, 0]
  for i, ((label, kw, _), r) in enumerate(zip(runs, res)):
    b = res[base.get(i, 0)]
    if b is r:
      continue
    for li in range(4):
      assert torch.equal(r['acts'][li], b['acts'][li]), (what, label, 'forward activation %d differs' % li)
    mag = lambda i0, i1: (b['last_in'][i0:i1].float().abs() @ w0.abs().t()) * (1.0 + w0.shape[1] * E.U32)
    T._ew_note('gp chain %s gx vs all-off' % topology, dname, E.assert_pair_device(r['gx'], b['gx'], mag, w0.shape[1],
                                                                                   '%s %s %s gx' % (what, dname, label), roundings=4))
  if topology == 'plain':
    for (label, _, _), r in zip(runs, res):
      _plain_stages_check(r, ws, dtype, dname, '%s %s %s' % (what, dname, label))
  # ---- gx against float64 on the stored operands, the mask ties taking either slope
  ref, alt, tie, pre, acts = _chain_reference(topology, off, ws, bs, dtype)
  nties = sum(int(t.sum()) for t in tie)
  total = sum(t.size for t in tie)
  flips = sum(int((m(p) != m(a)).sum()) for p, a in zip(pre, acts))
  print('[gp chain %s %s] pre-activations inside their own bound: %d of %d; stored with the other sign: %d' % (topology, dname, nties, total, flips))
  for li in range(4):
    wrong = (m(pre[li]) != m(acts[li])) & ~tie[li]
    assert not wrong.any(), '%s %s: layer %d stored a sign its float64 pre-activation does not have at %s' % (
        what, dname, li, tuple(int(v[0]) for v in np.nonzero(wrong)))
  masks = [m(p) for p in pre]
  gx64, grads64 = _chain_torch64(topology, masks, ws)
  _close64(ref.ref, gx64, what + ' chain closed form')
  for (label, _, _), r in zip(runs, res):
    T._ew_note('gp chain %s gx' % topology, dname, E.assert_elementwise(
        T.host(r['gx']), ref.ref, ref.err, '%s %s %s gx' % (what, dname, label), alt_ref=alt.ref,
        alt_where=np.full(ref.ref.shape, nties > 0), alt_cap=1e-5))
  # ---- the penalty's parameter gradients: rel-L2, every route within twice the all-off route's measured figure
  want = REL_L2_ALL_OFF[topology][dname]
  figures = []
  for (label, _, _), r in zip(runs, res):
    e = [T.rel_l2(T.host(g), g64) for g, g64 in zip(r['grads'], grads64)]
    figures.append(e)
    print('[gp chain %s %s] %-28s rel-L2 of d penalty / d w0..w3 vs float64: %s' % (topology, dname, label, ' '.join('%.2e' % v for v in e)))
  assert want is not None, 'no measured all-off figures recorded for %s %s' % (topology, dname)
  for (label, _, _), e in zip(runs, figures):
    for li, (v, w_) in enumerate(zip(e, want)):
      assert v <= 2.0 * w_, '%s %s %s: d penalty / d w%d is %.3e from float64, more than twice the all-off route\'s %.3e' % (
          what, dname, label, li, v, w_)


@pytest.mark.parametrize('dname', ['bf16', 'f16'])
def test_handshake_applies_every_mask_exactly_once(ops, monkeypatch, record_calls, dname):
  """fromRGB + lrelu -> conv + lrelu -> conv + lrelu + pool -> conv + lrelu at 3 x 32 x 32, 16 / 32 / 32 / 32 channels, the
  trainer's flow (forward in ops.second_order, inner gradient under ops.no_param_grads with create_graph, then the penalty's
  parameter gradients) for the four settings of (USE_GP_PREMASK, USE_DGRAD_UNPOOL_GP), and once more WITHOUT no_param_grads:
  parameter gradients hang off every g there, so nothing may be premasked."""
  import twingan_amd.ops as O
  runs = [('premask=%d one_node=%d' % s, dict(premask=s[0], one_node=s[1]), PLAIN_EPILOGUE[s]) for s in SETTINGS]
  runs.append(('flags on, parameter gradients wanted', dict(premask=True, one_node=True, skip_params=False), ()))
  _chain_check(O, monkeypatch, record_calls, 'plain', dname, runs, 'handshake')


@pytest.mark.parametrize('dname', ['bf16', 'f16'])
def test_handshake_in_the_residual_topology(ops, monkeypatch, record_calls, dname):
  """The chain use_res_block builds (pggan.maybe_resblock): a0 is read by the block's first conv and by the skip add.  pggan
  turns fuse_input_lrelu off there; the second pair of runs turns it on for the one conv whose input has a single consumer.
  A premask may only fire where the flagged node's output has no other reader: a0's mask must stay a launch of its own."""
  import twingan_amd.ops as O
  runs = [('premask=0', dict(premask=False, one_node=False), ()),
          ('premask=1', dict(premask=True, one_node=True), ()),
          ('premask=0 inner conv fused', dict(premask=False, one_node=False, fuse=True), ()),
          ('premask=1 inner conv fused', dict(premask=True, one_node=True, fuse=True), (1,))]
  _chain_check(O, monkeypatch, record_calls, 'residual', dname, runs, 'residual handshake', base={2: 2, 3: 2})
