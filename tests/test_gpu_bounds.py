"""GPU: where the Python wrappers' kernels read and write (tests/guarded.py).  Every case runs a wrapper of twingan_amd/ops.py
once the ordinary way (A) and once with every tensor the wrapper allocates served between 0xA5 guard bands, its empty() results
poisoned with NaN and its inputs between NaN bands (B), then checks in this order: guards intact; inputs and their surrounds
byte-equal to a pristine clone; B finite everywhere (no poison read into a result, no element left unwritten);
torch.equal(A, B) wherever the order of a sum is fixed (everything but 16-bit sums outside the deterministic mode).

Shapes are the edge shapes of the sanitized CPU driver (tests/hipemu/bounds_cases.inc), which checks the kernels against the
sizes the C header documents; this file checks the wrappers' own sizing (statistics partials, workspaces, sign bytes, pooled
tensors) and, at the 128x128 rows of EDGE_CASES, the kernel variants the driver cannot reach in its time (test_edge_rows_*:
skipped by name over the emulated kernels, where one case takes a minute).
"""
import json
import os

import pytest
import torch

import guarded as G

pytestmark = pytest.mark.gpu

DTYPES = {'bf16': torch.bfloat16, 'f16': torch.float16, 'f32': torch.float32}
HALF = ('bf16', 'f16')
EDGE_KERNELS = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'dispatch_edge_kernels.json')


def _dev():
  return torch.empty(1, device='cuda').device


def _t(shape, dname, seed, scale=1.0):
  g = torch.Generator().manual_seed(seed)
  return (torch.randn(*shape, generator=g) * scale).to(DTYPES[dname]).to(_dev())


def _w(k, cin, cout, dname, seed, groups=1):
  """An fp32 master kernel that holds values of the storage type (its pack is then exact)."""
  lead = (groups,) if groups > 1 else ()
  dt = DTYPES[dname]
  return _t(lead + (k, k, cin, cout), 'f32', seed, (k * k * cin) ** -0.5).to(dt).float().contiguous()


def _check(run, inputs, allocates=True, **kw):
  """guarded.check on the test device; ``allocates``: the wrapper must have been served at least one guarded tensor."""
  served = []
  out = G.check(run, inputs, _dev(), sync=torch.cuda.synchronize, served=served, **kw)
  assert not allocates or served, 'the guarded run allocated nothing: the harness did not see the wrapper'
  return out


class _Deterministic:
  def __init__(self, on):
    self.on = on

  def __enter__(self):
    from twingan_amd import _lib
    self.lib = _lib.load()
    self.prev = self.lib.tg_set_deterministic(1 if self.on else 0)

  def __exit__(self, *a):
    self.lib.tg_set_deterministic(self.prev)


def _last_kernel():
  from twingan_amd import _lib
  return _lib.load().tg_last_kernel().decode()


def _ops():
  import twingan_amd.ops as O
  return O


# ------------------------------------------------------------------------------------------------------------- convs
# n, h, w, cin, cout, k, padding: off every tile, channel counts a group of 8 above / below 32 and 64, n = 1, odd batches
CONV_SHAPES = [(1, 9, 5, 8, 24, 3, 'SAME'), (3, 6, 10, 24, 40, 3, 'SAME'), (1, 5, 7, 40, 8, 1, 'SAME'), (3, 4, 4, 8, 8, 4, 'VALID'),
               (1, 16, 16, 56, 72, 3, 'SAME'), (2, 8, 8, 16, 16, 3, 'SAME')]
DIRECT_SHAPES = [(1, 9, 5, 3, 4, 3, 'SAME'), (3, 4, 4, 5, 6, 4, 'VALID'), (2, 5, 5, 4, 6, 1, 'SAME')]
CONV_CASES = [(s, d) for s in CONV_SHAPES for d in HALF] + [(s, 'f32') for s in DIRECT_SHAPES] + [(DIRECT_SHAPES[0], 'bf16')]
_cid = lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v)


def _conv_operands(shape, dname, groups=1):
  O = _ops()
  n, h, w, cin, cout, k, pad = shape
  spec = O.ConvSpec(k, pad)
  ho, wo = spec.out_hw(h, w)
  x = _t((n, h, w, cin), dname, 1)
  gy = _t((n, ho, wo, cout), dname, 2)
  wt = _w(k, cin, cout, dname, 3, groups)
  b = _t(((groups,) if groups > 1 else ()) + (cout,), 'f32', 4, 0.1)
  return O, spec, x, gy, wt, b


@pytest.mark.parametrize('shape,dname', CONV_CASES, ids=_cid)
def test_conv_forward_wrappers_stay_inside_their_tensors(shape, dname):
  from twingan_amd._lib import TG_EPI_BIAS, TG_EPI_LRELU
  O, spec, x, gy, w, b = _conv_operands(shape, dname)
  _check(lambda x, w: O.conv_fwd_raw(x, w, None, spec, 0), [x, w])
  _check(lambda x, w, b: O.conv_fwd_raw(x, w, b, spec, TG_EPI_BIAS | TG_EPI_LRELU), [x, w, b])
  _check(lambda x, w, m: O.conv_fwd_masked_raw(x, w, m, spec), [x, w, gy])


@pytest.mark.parametrize('shape,dname', CONV_CASES, ids=_cid)
def test_conv_backward_data_wrappers_stay_inside_their_tensors(shape, dname):
  O, spec, x, gy, w, b = _conv_operands(shape, dname)
  _check(lambda gy, w: O.conv_bwd_data_raw(gy, w, tuple(x.shape), spec), [gy, w])
  _check(lambda gy, w, xa: O.conv_bwd_data_masked_raw(gy, w, xa, spec), [gy, w, x])


@pytest.mark.parametrize('det', [0, 1], ids=['atomics', 'deterministic'])
@pytest.mark.parametrize('shape,dname', CONV_CASES, ids=_cid)
def test_conv_filter_gradient_wrappers_stay_inside_their_tensors(shape, dname, det):
  """Alone, with the bias gradient riding along, and accumulating into buffers that already hold values (a gradient sink)."""
  O, spec, x, gy, w, b = _conv_operands(shape, dname)
  exact = bool(det) or dname == 'f32'
  with _Deterministic(det):
    _check(lambda x, gy: O.conv_bwd_weight_raw(x, gy, spec), [x, gy], exact=exact)
    gb0 = torch.zeros_like(b)
    _check(lambda x, gy, gb: O.conv_bwd_weight_raw(x, gy, spec, gbias=gb), [x, gy, gb0], inout=(2,), exact=exact)
    sink, bsink = _t(tuple(w.shape), 'f32', 7), _t(tuple(b.shape), 'f32', 8)
    _check(lambda x, gy, out, gb: O.conv_bwd_weight_raw(x, gy, spec, out=out, gbias=gb), [x, gy, sink, bsink], inout=(2, 3), exact=exact)


# 3x3 SAME on the tile kernels' smallest maps: h % 8 == 0, w % 16 == 0; cout % 32 == 0 for the unpooling backward
TILE_SHAPES = [(1, 8, 16, 24, 32, 3, 'SAME'), (3, 16, 16, 40, 64, 3, 'SAME'), (1, 8, 16, 8, 24, 3, 'SAME')]


@pytest.mark.parametrize('dname', HALF)
@pytest.mark.parametrize('shape', TILE_SHAPES, ids=_cid)
def test_conv_statistics_pool_sign_and_unpool_wrappers_stay_inside_their_tensors(shape, dname):
  from twingan_amd._lib import TG_EPI_BIAS, TG_EPI_LRELU
  epi = TG_EPI_BIAS | TG_EPI_LRELU
  O, spec, x, gy, w, b = _conv_operands(shape, dname)
  _check(lambda x, w: O.conv_fwd_stats_raw(x, w, spec), [x, w])
  _check(lambda x, w, b: O.conv_fwd_pool_raw(x, w, b, spec, epi), [x, w, b])
  assert O.conv_fwd_pool_signs_supported(x, w, spec, epi)
  (sg, zp), _ = _check(lambda x, w, b: O.conv_fwd_pool_signs_raw(x, w, b, spec, epi), [x, w, b])
  gzp = gy[:, ::2, ::2, :].contiguous()
  _check(lambda gzp, sg: O.lrelu_pool_bwd_signs(gzp, sg, spec.alpha, None, False), [gzp, sg])
  if shape[4] % 32 == 0:
    for keep in (False, True):
      out, _ = _check(lambda gzp, sg, w, xa: O.conv_bwd_data_unpool_raw(gzp, sg, w, xa, tuple(x.shape), spec, keep), [gzp, sg, w, x])
      assert out is not None, 'unpool refused'
    z = O.conv_fwd_raw(x, w, b, spec, epi)      # the pass that kept the activation instead of its sign bytes
    _check(lambda gzp, z, w, xa: O.conv_bwd_data_unpool_raw(gzp, z, w, xa, tuple(x.shape), spec, True), [gzp, z, w, x])


@pytest.mark.parametrize('dname', HALF)
@pytest.mark.parametrize('groups', [2, 3])
def test_grouped_conv_wrappers_stay_inside_their_tensors(groups, dname):
  from twingan_amd._lib import TG_EPI_BIAS, TG_EPI_LRELU
  epi = TG_EPI_BIAS | TG_EPI_LRELU
  O, spec, x, gy, w, b = _conv_operands((2 * groups, 8, 16, 24, 40, 3, 'SAME'), dname, groups)
  _check(lambda x, w, b: O.conv_fwd_raw(x, w, b, spec, epi), [x, w, b])
  _check(lambda x, w, m: O.conv_fwd_masked_raw(x, w, m, spec), [x, w, gy])
  _check(lambda gy, w, xa: O.conv_bwd_data_masked_raw(gy, w, xa, spec), [gy, w, x])
  _check(lambda x, w, b: O.conv_fwd_pool_signs_raw(x, w, b, spec, epi), [x, w, b])
  with _Deterministic(1):
    _check(lambda x, gy: O.conv_bwd_weight_raw(x, gy, spec, groups=groups), [x, gy])
    sink, bsink = _t(tuple(w.shape), 'f32', 7), _t(tuple(b.shape), 'f32', 8)
    _check(lambda x, gy, out, gb: O.conv_bwd_weight_raw(x, gy, spec, out=out, gbias=gb), [x, gy, sink, bsink], inout=(2, 3))


@pytest.mark.parametrize('dname', HALF)
def test_paired_filter_gradient_with_unequal_batches_stays_inside_its_tensors(dname):
  """tg_conv2d_bwd_weight2 with nb != n, with and without the bias gradient, into a sink that already holds values."""
  O, spec, xa, gya, w, b = _conv_operands((2, 16, 16, 24, 40, 3, 'SAME'), dname)
  xb, gyb = _t((3, 16, 16, 24), dname, 11), _t((3, 16, 16, 40), dname, 12)
  with _Deterministic(1):
    for with_bias in (False, True):
      def run(xa, gya, xb, gyb, out, gb):
        assert O.conv_bwd_weight2_raw(xa, gya, xb, gyb, spec, out, gb if with_bias else None, 1), 'pair refused'
        return ()
      _check(run, [xa, gya, xb, gyb, _t(tuple(w.shape), 'f32', 7), _t((40,), 'f32', 8)], inout=(4, 5))


@pytest.mark.parametrize('dname', HALF)
@pytest.mark.parametrize('shape', [(1, 8, 16, 32, 32, 24, 0, ()), (3, 16, 16, 32, 64, 40, 0, ()), (4, 8, 16, 64, 32, 8, 1, (1, 0, 0, 1))], ids=_cid)
def test_upsample_concat_conv_stays_inside_its_tensors(shape, dname):
  """O.upcat_conv forward, backward-data into both sources and the filter gradient (the autograd function owns them all)."""
  O = _ops()
  n, h, w, c0, c1, cout, gsz, perm = shape
  n1 = (max(perm) + 1) * gsz if gsz else n
  x0, x1 = _t((n, h // 2, w // 2, c0), dname, 1), _t((n1, h, w, c1), dname, 2)
  wt, gy = _w(3, c0 + c1, cout, dname, 3), _t((n, h, w, cout), dname, 4)
  assert O.upcat_conv_supported(x0, x1, wt)

  def run(x0, x1, wt, gy):
    a, b, c = x0.detach().requires_grad_(True), x1.detach().requires_grad_(True), wt.detach().requires_grad_(True)
    y = O.upcat_conv(a, b, c, gsz, perm)
    return (y.detach(),) + tuple(torch.autograd.grad(y, [a, b, c], gy))
  with _Deterministic(1):
    _check(run, [x0, x1, wt, gy])


# ------------------------------------------------------------------------- the 128x128 rows: kernels the driver leaves out
EDGE_ROWS = [
    # id, k, hw, cin, cout, n below, n above (tests/test_gpu_ops.py EDGE_CASES)
    ('tile_bn', 3, 128, 48, 64, 7, 8), ('tile_mt', 3, 128, 64, 32, 7, 8), ('tile_wres16', 3, 128, 16, 32, 15, 16),
    ('tile_wres32', 3, 128, 32, 32, 15, 16), ('tile_thin16', 3, 128, 16, 16, 15, 16), ('tile_k1_wres', 1, 128, 32, 32, 15, 16),
]


@pytest.mark.parametrize('side', [0, 1], ids=['below', 'above'])
@pytest.mark.parametrize('dname', HALF)
@pytest.mark.parametrize('row', EDGE_ROWS, ids=[r[0] for r in EDGE_ROWS])
def test_edge_rows_run_the_recorded_kernel_inside_their_tensors(row, dname, side):
  """Every entry point the dispatch table records for the row, on one side of its threshold: the intended kernel symbol ran
  (tests/golden/dispatch_edge_kernels.json) and nothing was written or read outside the tensors."""
  from twingan_amd._lib import TG_EPI_BIAS, TG_EPI_LRELU
  epi = TG_EPI_BIAS | TG_EPI_LRELU
  cid, k, hw, cin, cout, n_lo, n_hi = row
  n = (n_lo, n_hi)[side]
  with open(EDGE_KERNELS) as fh:
    want = json.load(fh)[cid][dname]
  O, spec, x, gy, w, b = _conv_operands((n, hw, hw, cin, cout, k, 'SAME'), dname)
  ran = {}

  def case(entry, run, inputs, **kw):
    if entry in want:
      out = _check(run, inputs, **kw)
      ran[entry] = _last_kernel()
      return out
  case('fwd', lambda x, w: O.conv_fwd_raw(x, w, None, spec, 0), [x, w])
  case('fwd_masked', lambda x, w, m: O.conv_fwd_masked_raw(x, w, m, spec), [x, w, gy])
  if k == 3:
    case('fwd_stats', lambda x, w: O.conv_fwd_stats_raw(x, w, spec), [x, w])
    case('fwd_pool', lambda x, w, b: O.conv_fwd_pool_raw(x, w, b, spec, epi), [x, w, b])
    got = case('fwd_pool_signs', lambda x, w, b: O.conv_fwd_pool_signs_raw(x, w, b, spec, epi), [x, w, b])
    if got is not None and cout % 32 == 0:
      sg, gzp = got[0][0], gy[:, ::2, ::2, :].contiguous()
      case('bwd_data_unpool', lambda gzp, sg, w, xa: O.conv_bwd_data_unpool_raw(gzp, sg, w, xa, tuple(x.shape), spec, True), [gzp, sg, w, x])
  case('bwd_data', lambda gy, w: O.conv_bwd_data_raw(gy, w, tuple(x.shape), spec), [gy, w])
  case('bwd_data_masked', lambda gy, w, xa: O.conv_bwd_data_masked_raw(gy, w, xa, spec), [gy, w, x])
  # the table records the default mode's kernels: 16-bit sums that may end in atomics, so no bit comparison of A and B
  case('bwd_weight', lambda x, gy: O.conv_bwd_weight_raw(x, gy, spec), [x, gy], exact=False)
  case('bwd_weight_bias', lambda x, gy, gb: O.conv_bwd_weight_raw(x, gy, spec, gbias=gb), [x, gy, torch.zeros_like(b)], inout=(2,),
       exact=False)
  missing = [e for e in want if e not in ran]
  assert not missing, ('recorded entry points this test does not run', missing)
  moved = {e: (ran[e], want[e][str(n)]) for e in ran if ran[e] != want[e][str(n)]}
  assert not moved, ('not the recorded kernel', cid, dname, n, moved)


# ---------------------------------------------------------------------------------------------- the remaining wrappers
PW_SHAPES = [(4099, 3, 16), (4096, 3, 16), (35, 3, 9), (4099, 16, 3), (1, 3, 8)]


@pytest.mark.parametrize('dname', sorted(DTYPES))
@pytest.mark.parametrize('shape', PW_SHAPES, ids=_cid)
def test_pointwise_conv_and_its_gradients_stay_inside_their_tensors(shape, dname):
  O = _ops()
  npix, cin, cout = shape
  x, gy = _t((1, 1, npix, cin), dname, 1), _t((1, 1, npix, cout), dname, 2)
  w, b = _w(1, cin, cout, dname, 3), _t((cout,), 'f32', 4, 0.1)

  def run(x, w, b, gy):
    a, ww, bb = x.detach().requires_grad_(True), w.detach().requires_grad_(True), b.detach().requires_grad_(True)
    y = O.pointwise_conv(a, ww, bb, lrelu=True)
    return (y.detach(),) + tuple(torch.autograd.grad(y, [a, ww, bb], gy))
  with _Deterministic(1):      # the ordered filter gradient: the same bits on every run
    _check(run, [x, w, b, gy])
  _check(run, [x, w, b, gy], exact=dname == 'f32')


# the cheap rows of NORM_EDGE_CASES (tests/test_gpu_ops.py): n, h, w, c, pixel norm, pool, split
NORM_SHAPES = [(3, 40, 24, 16, True, True, 1), (5, 17, 13, 8, True, False, 0), (3, 5, 13, 24, False, False, 1), (3, 16, 16, 5, False, True, None),
               (3, 1, 257, 5, False, False, 2), (3, 3, 86, 3, False, False, 1), (2, 34, 30, 256, True, True, 1), (1, 9, 5, 8, True, False, None)]


@pytest.mark.parametrize('dname', sorted(DTYPES))
@pytest.mark.parametrize('shape', NORM_SHAPES, ids=_cid)
def test_normaliser_forward_and_backward_stay_inside_their_tensors(shape, dname):
  O = _ops()
  n, h, w, c, pn, pool, split = shape
  y = _t((n, h, w, c), dname, 1)
  ga, be, ga2, be2 = (_t((c,), 'f32', s, 0.5) + o for s, o in ((2, 1.0), (3, 0.0), (4, 1.0), (5, 0.0)))
  gz = _t((n, h, w, c), dname, 6)
  gzp = _t((n, h // 2, w // 2, c), dname, 7)

  def run(y, ga, be, ga2, be2, gz, gzp):
    leaves = [t.detach().requires_grad_(True) for t in (y, ga, be, ga2, be2)]
    kw = dict(gamma2=leaves[3], beta2=leaves[4], split=split) if split is not None else {}
    out = O.norm_act(leaves[0], leaves[1], leaves[2], lrelu=True, pixel_norm=pn, pool=pool, **kw)
    outs = list(out) if isinstance(out, (tuple, list)) else [out]
    gs = [gz, gzp][:len(outs)]
    wanted = leaves if split is not None else leaves[:3]
    grads = torch.autograd.grad(outs, wanted, gs, allow_unused=True)
    return [o.detach() for o in outs], [g for g in grads if g is not None]
  with _Deterministic(1):
    _check(run, [y, ga, be, ga2, be2, gz, gzp])


@pytest.mark.parametrize('dname', sorted(DTYPES))
@pytest.mark.parametrize('shape', [(1, 10, 6, 7), (3, 6, 10, 9), (3, 2, 2, 16), (1, 18, 6, 24)], ids=_cid)
def test_resampling_family_stays_inside_its_tensors(shape, dname):
  O = _ops()
  n, h, w, c = shape
  x, z = _t((n, h, w, c), dname, 1), _t((n, h, w, c), dname, 2)
  gzp = _t((n, h // 2, w // 2, c), dname, 3)
  skip = _t((n, 2 * h, 2 * w, c + 1), dname, 4)
  b = _t((c,), 'f32', 5)

  def grad_of(fn, *ts):
    def run(*ts):
      leaves = [t.detach().requires_grad_(True) for t in ts[:-1]]
      y = fn(*leaves)
      return (y.detach(),) + tuple(torch.autograd.grad(y, leaves, ts[-1]))
    return run
  _check(grad_of(O.avg_pool2, x, gzp), [x, gzp])
  _check(grad_of(lambda a: O.upsample2x_concat(a), x, _t((n, 2 * h, 2 * w, c), dname, 6)), [x, _t((n, 2 * h, 2 * w, c), dname, 6)])
  _check(grad_of(lambda a, s: O.upsample2x_concat(a, s), x, skip, _t((n, 2 * h, 2 * w, 2 * c + 1), dname, 7)),
         [x, skip, _t((n, 2 * h, 2 * w, 2 * c + 1), dname, 7)])
  _check(lambda g, z: O.lrelu_bwd_raw(g, z, 0.2), [x, z])
  with _Deterministic(1):
    _check(lambda gz, gzp, z, b: O.lrelu_pool_bwd(gz, gzp, z, 0.2, b, True), [x, gzp, z, b])
    _check(lambda gzp, z, b: O.lrelu_pool_bwd(None, gzp, z, 0.2, b, False), [gzp, z, b])
    _check(lambda g: O.channel_sum_raw(g), [x])
  _check(grad_of(lambda a, bb: O.lerp(a, bb, 0.25), x, z, x), [x, z, x])


@pytest.mark.parametrize('dname', sorted(DTYPES))
@pytest.mark.parametrize('groups', [1, 3])
def test_minibatch_stddev_all_three_orders_stay_inside_their_tensors(groups, dname):
  O = _ops()
  x, gout, v = _t((6, 4, 4, 9), dname, 1), _t((6, 4, 4, 16), dname, 2), _t((6, 4, 4, 9), dname, 3)

  def run(x, gout, v):
    a, g = x.detach().requires_grad_(True), gout.detach().requires_grad_(True)
    y = O.minibatch_state_concat(a, 16, groups)
    gx, = torch.autograd.grad(y, a, g, create_graph=True)
    ggout, gx2 = torch.autograd.grad(gx, [g, a], v)
    return y.detach(), gx.detach(), ggout, gx2
  _check(run, [x, gout, v])


@pytest.mark.parametrize('dname', HALF)
@pytest.mark.parametrize('shape', [(1, 128, 8, 64), (3, 256, 16, 64), (1, 256, 16, 128), (2, 128, 16, 256)], ids=_cid)
def test_flash_attention_all_three_orders_stay_inside_their_tensors(shape, dname):
  O = _ops()
  n, ln, dk, dv = shape
  q, k, v = _t((n, ln, dk), dname, 1, 0.5), _t((n, ln, dk), dname, 2, 0.5), _t((n, ln, dv), dname, 3)
  go = _t((n, ln, dv), dname, 4)
  _check(lambda q, k, v: O.flash_attention_fwd_raw(q, k, v), [q, k, v])
  if dv > 128:
    return
  cot = [_t((n, ln, dk), dname, 5), _t((n, ln, dk), dname, 6), _t((n, ln, dv), dname, 7)]

  def run(q, k, v, go, aq, ak, av):
    leaves = [t.detach().requires_grad_(True) for t in (q, k, v, go)]
    with O.second_order():
      o = O.flash_attention(*leaves[:3])
      first = torch.autograd.grad(o, leaves[:3], leaves[3], create_graph=True)
      second = torch.autograd.grad(first, leaves, [aq, ak, av])
    return o.detach(), [g.detach() for g in first], second
  _check(run, [q, k, v, go] + cot)


@pytest.mark.parametrize('dname', ['bf16', 'f32'])
@pytest.mark.parametrize('shape', [(1, 33, 31, 17), (3, 32, 64, 16), (2, 5, 40, 33)], ids=_cid)
def test_batched_gemm_and_softmax_stay_inside_their_tensors(shape, dname):
  O = _ops()
  bt, m, n, k = shape
  a, b, g = _t((bt, m, k), dname, 1), _t((bt, k, n), dname, 2), _t((bt, m, n), dname, 3)

  def run(a, b, g):
    la, lb = a.detach().requires_grad_(True), b.detach().requires_grad_(True)
    p = O.softmax_rows(O.bgemm(la, lb, alpha=0.5))
    ga, gb = torch.autograd.grad(p, [la, lb], g, create_graph=True)
    second = torch.autograd.grad([ga, gb], [la, lb], [a, b])
    return p.detach(), ga.detach(), gb.detach(), second
  _check(run, [a, b, g])
  bt_t = _t((bt, k, m), dname, 4)
  _check(lambda a, b: O.bgemm(a, b, ta=True, tb=True), [bt_t, _t((bt, n, k), dname, 5)])


LOSS_SHAPES = [(1, 1, 1, 1), (2, 5, 5, 3), (1, 4099, 1, 1)]


@pytest.mark.parametrize('det', [0, 1], ids=['atomics', 'deterministic'])
@pytest.mark.parametrize('dname', sorted(DTYPES))
@pytest.mark.parametrize('shape', LOSS_SHAPES, ids=_cid)
def test_loss_sums_and_the_gradient_penalty_stay_inside_their_tensors(shape, dname, det):
  """The scalar sums on whole tensors and on views that start off a 16-byte boundary, the penalty, the prediction losses."""
  O = _ops()
  a, b = _t(shape, dname, 1), _t(shape, dname, 2)
  exact = bool(det) or dname == 'f32'

  def run(a, b):
    la, lb = a.detach().requires_grad_(True), b.detach().requires_grad_(True)
    terms = [O.mean(la, 0.5), O.abs_diff_mean(la, lb, 2.0), O.gradient_penalty(la, 10.0)]
    total = O.sum_scalars(terms)
    return [t.detach() for t in terms], total.detach(), torch.autograd.grad(total, [la, lb])
  with _Deterministic(det):
    _check(run, [a, b], exact=exact)
    if a.numel() > 8:      # the loss sums of views that start 2 bytes / one element past a 16-byte boundary
      flat = _t((a.numel() + 1,), dname, 3)
      _check(lambda f: (O.mean(f[1:], 1.0), O.abs_diff_mean(f[1:], f[:-1], 1.0)), [flat], exact=exact)
  pred = _t((shape[0] * 5,), 'f32', 4)

  def tail(pred):
    lp = pred.detach().requires_grad_(True)
    terms = [O.mean(lp), O.hinge_mean(lp, 1.0, -1.0), O.sigmoid_xent_mean(lp, 1.0), O.square_mean(lp, 0.001)]
    total = O.sum_scalars(terms)
    return total.detach(), torch.autograd.grad(total, lp)
  _check(tail, [pred])


@pytest.mark.parametrize('shape', [(1, 1, 17, 63), (3, 3, 8, 257), (1, 1, 33, 1024), (3, 3, 5, 7)], ids=_cid)
def test_spectral_norm_stays_inside_its_tensors(shape):
  O = _ops()
  w, u, g = _t(shape, 'f32', 1, 0.1), _t((1, shape[3]), 'f32', 2), _t(shape, 'f32', 3)

  def run(w, u, g):
    lw = w.detach().requires_grad_(True)
    wb, u_new = O.spectral_norm(lw, u)
    return wb.detach(), u_new.detach(), torch.autograd.grad(wb, lw, g)
  _check(run, [w, u, g])


@pytest.mark.parametrize('dname', sorted(DTYPES))
def test_rows_and_cat_rows_stay_inside_their_tensors(dname):
  O = _ops()
  a, b, c = _t((3, 5, 7), dname, 1), _t((1, 5, 7), dname, 2), _t((2, 5, 7), dname, 3)
  g = _t((6, 5, 7), dname, 4)

  def run(a, b, c, g):
    leaves = [t.detach().requires_grad_(True) for t in (a, b, c)]
    y = O.cat_rows(leaves)
    return y.detach(), torch.autograd.grad(y, leaves, g)
  _check(run, [a, b, c, g])


@pytest.mark.parametrize('dname', sorted(DTYPES))
@pytest.mark.parametrize('shape', [(3, 16, 16, 3, 5), (1, 32, 48, 3, 5), (3, 64, 64, 1, 5), (3, 24, 40, 3, 3)], ids=_cid)
def test_msssim_stays_inside_its_tensors(shape, dname):
  O = _ops()
  n, h, w, c, levels = shape
  a, b = _t((n, h, w, c), dname, 1).abs().clamp(max=1), _t((n, h, w, c), dname, 2).abs().clamp(max=1)
  wts = (0.2, 0.3, 0.5) if levels == 3 else None
  _check(lambda a, b: O.msssim(a, b, scale=255., weights=wts, return_mean=True), [a, b])


@pytest.mark.parametrize('dname', sorted(DTYPES))
def test_swd_stages_stay_inside_their_tensors(dname):
  O = _ops()
  x = _t((3, 32, 32, 3), dname, 1).abs().clamp(max=1)
  levels, _ = _check(lambda x: O.swd_pyramid(x), [x])
  if dname != 'f32':
    return
  g = torch.Generator().manual_seed(5)
  for level in levels:
    s = level.shape[1]
    tab = torch.randint(3, s - 3, (3 * 16, 2), generator=g)
    _check(lambda level: O.swd_descriptors(level, tab, 16), [level])
  for N in (1, 2, 147, 768):      # one row; below and above one chunk of the statistics; a multi-block sort
    da, db = _t((N, 147), 'f32', 10 + N), _t((N, 147), 'f32', 20 + N)
    dirs = _t((2, 147, 8), 'f32', 30)
    dirs = (dirs / dirs.norm(dim=1, keepdim=True)).contiguous()
    _check(lambda d, dirs: O.swd_project(d, dirs), [da, dirs], finite=False)      # rows N..Npad-1 of the projection are +inf
    _check(lambda a, b, dirs: O.swd_distance(a, b, dirs), [da, db, dirs])


def test_spectral_norm_of_many_stays_inside_its_tensors():
  """tg_spectral_norm_fwd_multi through ops.spectral_norm_multi: one-block and many-block jobs next to each other."""
  O = _ops()
  shapes = [(3, 3, 16, 512), (1, 1, 1, 1), (1, 1, 33, 1024), (1, 1, 5, 1), (3, 3, 5, 7), (1, 1, 4096, 1), (1, 1, 16, 1023)]
  ws = [_t(s, 'f32', 40 + i, 0.1) for i, s in enumerate(shapes)]
  us = [_t((1, s[3]), 'f32', 60 + i) for i, s in enumerate(shapes)]

  def run(*ts):
    k = len(ts) // 3
    outs, _ = O.spectral_norm_multi(list(zip(ts[:k], ts[k:2 * k], ts[2 * k:])))
    return [(wb.detach(), un.detach()) for wb, un in outs]
  _check(run, ws + us + [torch.zeros_like(w) for w in ws], inout=tuple(range(2 * len(ws), 3 * len(ws))))


@pytest.mark.parametrize('numel', [1, 3, 5, 4099])
def test_adam_and_moving_average_applies_stay_inside_their_tensors(numel):
  """tg_adam_step, tg_adam_ema_step and tg_ema_update on flat buffers of a 16-byte vector - 1 / + 1 elements, one element and
  a long tail: theta, m, v, avg are updated in place (their surrounds must not change), grad and the scalars are read only."""
  O = _ops()
  th, g, m, avg = (_t((numel,), 'f32', s) for s in (1, 2, 3, 4))
  v = _t((numel,), 'f32', 5).abs()
  lr, wd = torch.full((1,), 1e-3, device=_dev()), torch.full((1,), 0.125, device=_dev())
  P = lambda t: t.data_ptr()

  def adam(th, g, m, v, lr):
    O.call('tg_adam_step', P(th), P(g), P(m), P(v), None, numel, 1e-3, P(lr), 0.5, 0.99, 1e-8, 0.5, O._stream())
    return ()

  def adam_ema(th, g, m, v, avg, lr, wd):
    O.call('tg_adam_ema_step', P(th), P(g), P(m), P(v), P(avg), numel, P(lr), 0.5, 0.99, 1e-8, 0.5, P(wd), O._stream())
    return ()

  def ema(avg, th, wd):
    O.call('tg_ema_update', P(avg), P(th), numel, P(wd), O._stream())
    return ()
  _check(adam, [th, g, m, v, lr], inout=(0, 2, 3), allocates=False)
  _check(adam_ema, [th, g, m, v, avg, lr, wd], inout=(0, 2, 3, 4), allocates=False)
  _check(ema, [avg, th, wd], inout=(0,), allocates=False)


# ------------------------------------------------------------- grouped and upsample-concat rows of the dispatch table
def _recorded(cid, dname):
  with open(EDGE_KERNELS) as fh:
    return json.load(fh)[cid][dname]


GROUPED_ROWS = [
    # id, G, k, padding, hw, cin, cout, n (tests/test_gpu_ops.py GROUPED_EDGE_CASES)
    ('g2_k1_hw8_under', 2, 1, 'SAME', 8, 32, 32, 64), ('g3_k1_hw8_under', 3, 1, 'SAME', 8, 32, 32, 48),
    ('g2_k3_hw4_under', 2, 3, 'SAME', 4, 32, 32, 256), ('g3_k3_hw4_under', 3, 3, 'SAME', 4, 32, 32, 240),
    ('g2_dense_under', 2, 4, 'VALID', 4, 8, 8, 384), ('g2_k1_hw8_n96', 2, 1, 'SAME', 8, 32, 32, 96),
    ('g3_k1_hw8_n96', 3, 1, 'SAME', 8, 32, 32, 96), ('g2_k3_hw4_n264', 2, 3, 'SAME', 4, 32, 32, 264),
    ('g2_k3_hw4_n384', 2, 3, 'SAME', 4, 32, 32, 384), ('g3_k3_hw4_n600', 3, 3, 'SAME', 4, 32, 32, 600),
    ('g2_mbstd_c264_n264', 2, 3, 'SAME', 4, 264, 256, 264), ('g2_dense_n8192', 2, 4, 'VALID', 4, 8, 8, 8192),
    ('g3_dense_n6144', 3, 4, 'VALID', 4, 8, 8, 6144), ('g2_k1_hw8_over', 2, 1, 'SAME', 8, 32, 32, 130),
    ('g3_k1_hw8_over', 3, 1, 'SAME', 8, 32, 32, 195), ('g2_k3_hw4_over', 2, 3, 'SAME', 4, 32, 32, 514),
    ('g2_dense_over', 2, 4, 'VALID', 4, 8, 8, 8194), ('g2_tile_under', 2, 3, 'SAME', 128, 16, 32, 8),
    ('g2_tile_n16', 2, 3, 'SAME', 128, 16, 32, 16), ('g3_tile_n24', 3, 3, 'SAME', 128, 16, 32, 24),
    ('g2_tile_over', 2, 3, 'SAME', 128, 16, 32, 32),
]


@pytest.mark.parametrize('dname', HALF)
@pytest.mark.parametrize('row', GROUPED_ROWS, ids=[r[0] for r in GROUPED_ROWS])
def test_edge_rows_grouped_run_the_recorded_kernel_inside_their_tensors(row, dname):
  from twingan_amd._lib import TG_EPI_BIAS, TG_EPI_LRELU
  epi = TG_EPI_BIAS | TG_EPI_LRELU
  cid, groups, k, pad, hw, cin, cout, n = row
  want = _recorded(cid, dname)
  O, spec, x, gy, w, b = _conv_operands((n, hw, hw, cin, cout, k, pad), dname, groups)
  ran = {}

  def case(entry, run, inputs):
    if entry in want:
      out = _check(run, inputs)
      ran[entry] = _last_kernel()
      return out
  case('fwd', lambda x, w, b: O.conv_fwd_raw(x, w, b, spec, epi), [x, w, b])
  case('fwd_masked', lambda x, w, m: O.conv_fwd_masked_raw(x, w, m, spec), [x, w, gy])
  case('bwd_data', lambda gy, w: O.conv_bwd_data_raw(gy, w, tuple(x.shape), spec), [gy, w])
  case('bwd_data_masked', lambda gy, w, xa: O.conv_bwd_data_masked_raw(gy, w, xa, spec), [gy, w, x])
  case('fwd_pool', lambda x, w, b: O.conv_fwd_pool_raw(x, w, b, spec, epi), [x, w, b])
  got = case('fwd_pool_signs', lambda x, w, b: O.conv_fwd_pool_signs_raw(x, w, b, spec, epi), [x, w, b])
  if got is not None:
    sg, gzp = got[0][0], gy[:, ::2, ::2, :].contiguous()
    case('bwd_data_unpool', lambda gzp, sg, w, xa: O.conv_bwd_data_unpool_raw(gzp, sg, w, xa, tuple(x.shape), spec, True), [gzp, sg, w, x])
  missing = [e for e in want if e not in ran]
  assert not missing, ('recorded entry points this test does not run', missing)
  moved = {e: (ran[e], want[e]) for e in ran if ran[e] != want[e]}
  assert not moved, ('not the recorded kernel', cid, dname, moved)


UPCAT_ROWS = [
    # id, hw (output), c0, c1, cout, n below, n above (tests/test_gpu_ops.py UPCAT_EDGE_CASES)
    ('upcat_32_32_mt_wres', 64, 32, 32, 32, 31, 32), ('upcat_64_64_bn', 64, 64, 64, 64, 15, 16), ('upcat_64_64_mt', 64, 64, 64, 64, 31, 32),
    ('upcat_32_32_thin16', 128, 32, 32, 16, 15, 16), ('upcat_32_32_upboth', 128, 32, 32, 16, 7, 8), ('upcat_64_64_wres', 128, 64, 64, 32, 7, 8),
]


@pytest.mark.parametrize('side', [0, 1], ids=['below', 'above'])
@pytest.mark.parametrize('dname', HALF)
@pytest.mark.parametrize('row', UPCAT_ROWS, ids=[r[0] for r in UPCAT_ROWS])
def test_edge_rows_upcat_run_the_recorded_kernel_inside_their_tensors(row, dname, side):
  cid, hw, c0, c1, cout, n_lo, n_hi = row
  n = (n_lo, n_hi)[side]
  want = _recorded(cid, dname)
  O = _ops()
  x0, x1 = _t((n, hw // 2, hw // 2, c0), dname, 1), _t((n, hw, hw, c1), dname, 2)
  w, gy = _w(3, c0 + c1, cout, dname, 3), _t((n, hw, hw, cout), dname, 4)
  ran = {}
  _check(lambda x0, x1, w: O.upcat_conv(x0, x1, w, 0, ()), [x0, x1, w])
  ran['upcat_fwd'] = _last_kernel()
  _check(lambda x0, x1, w: O.upcat_conv_stats(x0, x1, w, 0, ()), [x0, x1, w])
  ran['upcat_fwd_stats'] = _last_kernel()

  def grads(x0, x1, w, gy, which):
    leaves = [t.detach().requires_grad_(i in which) for i, t in enumerate((x0, x1, w))]
    y = O.upcat_conv(*leaves, 0, ())
    return torch.autograd.grad(y, [leaves[i] for i in which], gy)
  # tg_last_kernel() is per thread and autograd runs a backward on a thread of its own: the symbol is read there, right after
  # the wrapper's call (the filter gradient below is read on this thread, as the test that recorded the table reads it)
  real = O.call

  def spy(name, *a, **kw):
    rc = real(name, *a, **kw)
    if name == 'tg_conv2d_upcat_bwd_data':
      ran['upcat_bwd_data'] = _last_kernel()
    return rc
  O.call = spy
  try:
    _check(lambda x0, x1, w, gy: grads(x0, x1, w, gy, (0, 1)), [x0, x1, w, gy])
  finally:
    O.call = real
  # (the table records the default mode's filter-gradient kernel: a 16-bit sum, no bit comparison)
  _check(lambda x0, x1, w, gy: grads(x0, x1, w, gy, (2,)), [x0, x1, w, gy], exact=False)
  ran['upcat_bwd_weight'] = _last_kernel()
  assert sorted(want) == sorted(ran), (sorted(want), sorted(ran))
  moved = {e: (ran[e], want[e][str(n)]) for e in ran if ran[e] != want[e][str(n)]}
  assert not moved, ('not the recorded kernel', cid, dname, n, moved)


# ----------------------------------------------------------------------------------------- further wrappers of the issue
@pytest.mark.parametrize('dname', sorted(DTYPES))
@pytest.mark.parametrize('shape', [(3, 40, 24, 16, True), (5, 17, 13, 8, False), (3, 16, 16, 5, True), (1, 9, 5, 24, False)], ids=_cid)
def test_normaliser_with_per_image_parameters_stays_inside_its_tensors(shape, dname):
  """ops.affine_act: gamma / beta one row per image, forward and backward (ggamma / gbeta [n][c] are written)."""
  O = _ops()
  n, h, w, c, pool = shape
  pn = c >= 8 and c & (c - 1) == 0
  y, gz, gzp = _t((n, h, w, c), dname, 1), _t((n, h, w, c), dname, 2), _t((n, h // 2, w // 2, c), dname, 3)
  ga, be = _t((n, c), 'f32', 4, 0.5) + 1.0, _t((n, c), 'f32', 5, 0.5)

  def run(y, ga, be, gz, gzp):
    leaves = [t.detach().requires_grad_(True) for t in (y, ga, be)]
    out = O.affine_act(*leaves, lrelu=True, pixel_norm=pn, pool=pool)
    outs = list(out) if isinstance(out, (tuple, list)) else [out]
    return [o.detach() for o in outs], torch.autograd.grad(outs, leaves, [gz, gzp][:len(outs)])
  with _Deterministic(1):
    _check(run, [y, ga, be, gz, gzp])


@pytest.mark.parametrize('dname', HALF)
@pytest.mark.parametrize('shape', [(1, 8, 16, 32, 32), (3, 16, 16, 24, 40)], ids=_cid)
def test_normaliser_fed_by_the_convs_statistics_partials_stays_inside_its_tensors(shape, dname):
  """ops.conv2d_stats -> ops.norm_act(conv_stats=...): the partials the conv writes are sized by the wrapper and consumed by
  tg_norm_act_fwd_conv_stats; forward and backward of the pair."""
  O = _ops()
  n, h, w, cin, cout = shape
  x, wt, gz = _t((n, h, w, cin), dname, 1), _w(3, cin, cout, dname, 2), _t((n, h, w, cout), dname, 3)
  ga, be = _t((cout,), 'f32', 4, 0.5) + 1.0, _t((cout,), 'f32', 5, 0.5)
  seen = []

  def run(x, wt, ga, be, gz):
    leaves = [t.detach().requires_grad_(True) for t in (x, wt, ga, be)]
    y, st = O.conv2d_stats(leaves[0], leaves[1])
    seen.append(st is not None)
    z = O.norm_act(y, leaves[2], leaves[3], lrelu=True, pixel_norm=cout == 32, conv_stats=st)
    return z.detach(), torch.autograd.grad(z, leaves, gz)
  with _Deterministic(1):
    _check(run, [x, wt, ga, be, gz])
  assert all(seen), 'the conv wrote no statistics partials at this shape'


@pytest.mark.parametrize('dname', sorted(DTYPES))
def test_rows_stay_inside_their_tensors(dname):
  """ops.rows (RowsFn): a view, a gathered copy of two ranges and a repeat; the backward sums the ranges that overlap."""
  O = _ops()
  x = _t((5, 3, 7), dname, 1)
  specs = ((0, 2), ((3, 5), (0, 1)), ((1, 2), (1, 2), (4, 5)))
  gs = [_t((2, 3, 7), dname, 2), _t((3, 3, 7), dname, 3), _t((3, 3, 7), dname, 4)]

  def run(x, g0, g1, g2):
    leaf = x.detach().requires_grad_(True)
    outs = O.rows(leaf, specs)
    return [o.detach().clone() for o in outs], torch.autograd.grad(outs, leaf, [g0, g1, g2])
  _check(run, [x] + gs)


def test_batched_loss_tail_stays_inside_its_tensors():
  """ops.pred_losses: 3 groups of 5 predictions, 12 jobs over 8 terms (the limits), forward and backward."""
  O = _ops()
  pred = _t((15, 1), 'f32', 1)
  jobs = tuple((i % 3, i % 8, i % 4, 1.0, -1.0, 0.5) for i in range(12))
  gts = [_t((1,), 'f32', 10 + t) for t in range(8)]

  def run(pred, *gts):
    leaf = pred.detach().requires_grad_(True)
    terms = O.pred_losses(leaf, 5, jobs, 8)
    return [t.detach().clone() for t in terms], torch.autograd.grad(terms, leaf, list(gts))
  _check(run, [pred] + gts)


@pytest.mark.parametrize('dname', HALF)
def test_multi_pack_refresh_stays_inside_its_tensors(dname):
  """PackCache.refresh: every pack of three registered weights (one of them two stacked sets) rebuilt by ONE
  tg_conv2d_pack_weights_multi launch from a job table the wrapper sizes; the rebuilt packs equal the single-launch ones."""
  O = _ops()
  shapes = [((1, 9, 5, 8, 24, 3, 'SAME'), 1), ((4, 8, 16, 24, 40, 3, 'SAME'), 2), ((3, 4, 4, 8, 8, 4, 'VALID'), 1)]
  ws = [_w(s[5], s[3], s[4], dname, 20 + i, g) for i, (s, g) in enumerate(shapes)]

  def run(*ws):
    packs = []
    try:
      for wt, (s, g) in zip(ws, shapes):
        O.PackCache.register(wt)
        d = O._desc(s[:4], s[4], O.ConvSpec(s[5], s[6]), DTYPES[dname], 0, g)
        packs += [O.PackCache.get(wt, d, mode) for mode in (0, 1)]
      single = [p.clone() for p in packs]
      for p in packs:
        p.fill_(float('nan'))      # what the refresh does not rewrite stays visible
      O.PackCache.version += 1
      assert O.PackCache.refresh(list(ws)) == len(packs)
      torch.cuda.synchronize()
      for p, q in zip(packs, single):
        assert torch.equal(p, q), 'a refreshed pack differs from the pack of the single launch'
      return [p.clone() for p in packs]
    finally:
      for wt in ws:
        O.PackCache.unregister(wt)
  _check(run, ws)


@pytest.mark.parametrize('skip', [0, 1], ids=['applied', 'skipped'])
@pytest.mark.parametrize('numel', [1, 3, 5, 4099])
def test_guarded_applies_and_the_loss_scale_state_stay_inside_their_tensors(numel, skip):
  """tg_nonfinite_check, tg_loss_scale_tick, tg_adam_step_guarded and tg_adam_ema_step_guarded as Trainer._apply issues
  them (the trainer calls the library on its own flat buffers: there is no wrapper that allocates).  The 32-byte state, the
  step counter and the rate sit between NaN bands like every other operand."""
  import ctypes
  from twingan_amd import _lib
  O = _ops()
  th, g, m, avg = (_t((numel,), 'f32', s) for s in (1, 2, 3, 4))
  v = _t((numel,), 'f32', 5).abs()
  if skip:
    g[numel // 2] = float('inf')
  st = _lib.TgLossScaleState(scale=128.0, seed=128.0, inv_scale=1.0 / 128.0)
  assert ctypes.sizeof(st) == _lib.load().tg_loss_scale_state_bytes() == 32
  state = torch.frombuffer(bytearray(bytes(st)), dtype=torch.uint8).to(_dev())
  step, lr = torch.full((1,), 3, dtype=torch.int64, device=_dev()), torch.full((1,), 1e-3, device=_dev())
  wd = torch.full((1,), 0.125, device=_dev())
  P = lambda t: t.data_ptr()

  def run(th, g, m, v, avg, state, step, lr, wd):
    s = O._stream()
    O.call('tg_nonfinite_check', P(g), numel, P(state), s)
    O.call('tg_loss_scale_tick', P(state), P(step), P(lr), 1e-3, 0.5, 0.99, 2, 65536.0, 1, s)
    O.call('tg_adam_step_guarded', P(th), P(g), P(m), P(v), numel, P(lr), 0.5, 0.99, 1e-8, P(state), s)
    O.call('tg_adam_ema_step_guarded', P(th), P(g), P(m), P(v), P(avg), numel, P(lr), 0.5, 0.99, 1e-8, P(state), P(wd), s)
    return ()
  _, B = _check(run, [th, g, m, v, avg, state, step, lr, wd], inout=(0, 2, 3, 4, 5, 6, 7), allocates=False, finite=not skip)


def test_multi_tensor_moving_average_stays_inside_its_tensors():
  """tg_ema_update_multi over a job table built as Trainer._build_ema_table builds it: one-element, off-vector and
  multi-block tensors next to each other; the averages change in place, the variables and the table are read only."""
  import ctypes
  from twingan_amd import _lib
  O = _ops()
  numels = [1, 4099, 3, 5, 70001, 7]
  avgs = [_t((k,), 'f32', 10 + i) for i, k in enumerate(numels)]
  vars_ = [_t((k,), 'f32', 30 + i) for i, k in enumerate(numels)]
  wd = torch.full((1,), 0.125, device=_dev())

  def run(*ts):
    k = len(numels)
    a, v, w = ts[:k], ts[k:2 * k], ts[2 * k]
    host = ctypes.create_string_buffer(_lib.load().tg_ema_table_bytes(k))
    blocks = ctypes.c_int32(0)
    for j in range(k):
      O.call('tg_ema_table_fill', a[j].data_ptr(), v[j].data_ptr(), a[j].numel(), j, ctypes.addressof(host), ctypes.byref(blocks))
    table = G.guarded_input(torch.frombuffer(bytearray(host.raw), dtype=torch.uint8).to(_dev()), 'job table')
    O.call('tg_ema_update_multi', table.t.data_ptr(), k, blocks.value, w.data_ptr(), O._stream())
    torch.cuda.synchronize()
    assert table.intact() is None, table.intact()
    return ()
  _check(run, avgs + vars_ + [wd], inout=tuple(range(len(numels))), allocates=False)


@pytest.mark.parametrize('crops', [False, True], ids=['resize', 'crop'])
@pytest.mark.parametrize('precision', ['fp32', 'bf16', 'fp16'])
def test_preprocessing_stays_inside_its_tensors(precision, crops):
  """data.Preprocessor.run (tg_preprocess_images_crop): three images of different odd sizes, one smaller than the output, PAD
  rectangles that reach outside the image; the packed bytes and the offset / rect / aug / crop tables are device tensors
  between NaN bands, the output is the wrapper's own allocation."""
  import numpy as np
  from twingan_amd import data
  rng = np.random.RandomState(3)
  images = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in ((9, 23), (33, 17), (21, 5))]
  pre = data.Preprocessor(16, device=_dev(), precision=precision, resize_mode='PAD', is_training=True, seed=1, do_random_cropping=crops)
  tables = [t.to(_dev()) for t in pre.pack(images)]
  files = (os.path.join('twingan_amd', 'data.py'),)
  served = []
  G.check(lambda *d: pre.run(*d), tables, _dev(), sync=torch.cuda.synchronize, served=served, files=files)
  assert served, 'the guarded run did not see the preprocessor allocate its output'
