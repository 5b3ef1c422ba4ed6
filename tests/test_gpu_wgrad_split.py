"""GPU parity of the filter-gradient kernels across their OWN work split (conv_wgrad_tile.hip wg_split / wg_waves / wg_quad /
wg_thin, conv_mfma.hip wgrad_split): which of the five kernels runs, how the batch's tiles are cut into workgroup ranges, and
the slab reduction behind them.  The operator tests of tests/test_gpu_ops.py and the bench shapes only meet splits whose tile
count divides evenly and whose ranges end where the first batch segment ends; the rows below are the other cells: a ragged
last range, the segment boundary inside a range, an odd batch on the pair-of-images kernel, the quadrant kernel below the
bench shape, non-square maps and maps with h % 16 == 8, slice counts that are multiples of 8 (the XCD decode of the block id)
together with a ragged last slice, a workspace that is not 16-byte aligned, sinks that already hold values.

The rows are DATA (as EDGE_CASES of tests/test_gpu_ops.py): every row states the kernel it expects and its tile count, first
segment's tile count, tiles per workgroup and slice count.  The tests do not recompute the split: they assert the symbol of
tg_last_kernel(), that the workspace the library asks for holds exactly the stated number of slabs (nslices 9 cin cout 4
bytes), and -- from the row's own numbers -- the property the row exists for, so that a row whose split has moved fails with
"no longer covers ...".  tests/golden/wgrad_split_kernels.json pins symbol and workspace per (row, dtype);
TG_RECORD_WGRAD_SPLIT_KERNELS=<path> re-records into <path>.

Bounds (tests/elementwise.py): every element of the fp32 filter gradient against oracle.np_ops.conv2d_bwd_weight_gemm on the
same 16-bit operands, summed over both segments: wgrad_bound(ref, oracle(|x|, |gy|), P) with P = (n + nb) h w, and
EDGE_F32_TOL on the rel-L2; the bias gradient by the same bound on the pixel sums.  Into a sink that holds values the kernel's
sum s (|s - ref| <= B) is added with ONE fp32 rounding, fl(sink + s): |got - sink - ref| <= B + 2^-24 |sink + s| <=
(1 + 2^-24) B + 2^-24 (|sink| + |ref|).  (The fused bias gradient reaches its sink by one atomic per slice, i.e. `slices`
roundings of a running value <= |sink| + mag; the P 2^-24 mag term of wgrad_bound counts P roundings of which the kernels
spend fewer than P / 2 -- one per 16-pixel MFMA step, the cross-wave sum and the slices -- so the same one-rounding widening
holds while |sink| <= mag, which the N(0, 1) sinks against sums over >= 64 pixels are.)
"""
import collections
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import np_ops as N          # noqa: E402  (checker only)
import elementwise as E                 # noqa: E402
import test_gpu_ops as T                # noqa: E402  (dev / host / rel_l2 / the [elementwise] bookkeeping)

GOLDEN_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'wgrad_split_kernels.json')
RECORD_ENV = 'TG_RECORD_WGRAD_SPLIT_KERNELS'
DTYPES = T.EDGE_DTYPES
TG_EINVAL = -1      # include/twingan_hip.h

# what tg_last_kernel() reports for the five kernels (the pair-of-images form is the 4-wave kernel's TW = 8 instantiation: it
# shares the symbol and is told apart by the 8x8 map) and for the first-generation kernel
SYMBOL = {'pair': 'conv_wgrad_tile_kernel', 'tile4': 'conv_wgrad_tile_kernel', 'tile8': 'conv_wgrad_tile_kernel<8 waves>',
          'quad': 'conv_wgrad_quad_kernel', 'thin': 'conv_wgrad_thin_kernel<16>'}
# rows x columns of one tile of each kernel (conv_wgrad_tile.hip, the kernels' headers); 'pair': two whole 8x8 images
TILE = {'tile4': (8, 16), 'quad': (8, 16), 'tile8': (16, 16), 'thin': (16, 16)}

Row = collections.namedtuple('Row', 'id n nb h w cin cout bias kernel tiles tiles_a per_wg slices covers')

# 'ragged'    the last workgroup range is short (tiles % per_wg != 0): the clamp of tile_end, and with one tile left a range
#             shorter than the two-stage pipeline
# 'boundary'  the first segment ends inside a range (tiles_a % per_wg != 0): the cursor's recomputation mid-range
# 'odd'       pair kernel, an odd segment in a range of several tiles: the last pair's second image contributes nothing
# 'slices8'   slices % 8 == 0: the block id is decoded XCD-wise, (slice / 8) 8 npairs + pair 8 + slice % 8
# 'h8'        h % 16 == 8 (what turns 8 waves into 4);  'nonsquare'  h != w
# 'cin_tail' / 'cout_tail'   a channel count that is no multiple of 32: zero-filled tails through the buffer resource
SPLIT_ROWS = [
    Row('r01_pair', 1, 3, 8, 8, 192, 512, False, 'pair', 3, 1, 2, 2, ('ragged', 'boundary', 'odd')),
    Row('r02_pair', 3, 5, 8, 8, 192, 512, False, 'pair', 5, 2, 3, 2, ('ragged', 'boundary', 'odd')),
    Row('r03_pair', 5, 5, 8, 8, 192, 256, False, 'pair', 6, 3, 2, 3, ('boundary', 'odd')),
    Row('r04_pair', 11, 5, 8, 8, 40, 512, False, 'pair', 9, 6, 2, 5, ('ragged', 'odd', 'cin_tail')),
    Row('r05_pair_bias', 7, 3, 8, 8, 32, 32, True, 'pair', 6, 4, 1, 6, ()),
    Row('r06_quad', 9, 2, 8, 16, 512, 192, False, 'quad', 11, 9, 2, 6, ('ragged', 'boundary', 'h8', 'nonsquare')),
    Row('r07_quad_single', 3, 0, 8, 16, 128, 64, False, 'quad', 3, 3, 1, 3, ('h8', 'nonsquare')),
    Row('r08_quad', 6, 5, 8, 16, 512, 192, False, 'quad', 11, 6, 2, 6, ('ragged', 'h8', 'nonsquare')),
    Row('r09_thin', 5, 5, 64, 32, 128, 16, False, 'thin', 80, 40, 3, 27, ('ragged', 'boundary', 'nonsquare')),
    Row('r10_thin_bias', 4, 5, 64, 64, 64, 16, True, 'thin', 144, 64, 3, 48, ('boundary', 'slices8')),
    Row('r11_tile4', 9, 2, 24, 16, 8, 256, False, 'tile4', 33, 27, 2, 17, ('ragged', 'boundary', 'h8', 'nonsquare', 'cin_tail')),
    Row('r12_tile4_bias', 5, 5, 16, 32, 512, 8, True, 'tile4', 40, 20, 3, 14, ('ragged', 'boundary', 'nonsquare', 'cout_tail')),
    Row('r13_tile4', 10, 5, 24, 48, 8, 40, False, 'tile4', 135, 90, 2, 68, ('ragged', 'h8', 'nonsquare', 'cin_tail', 'cout_tail')),
    Row('r14_tile4_bias', 5, 2, 24, 48, 8, 192, True, 'tile4', 63, 45, 2, 32,
        ('ragged', 'boundary', 'slices8', 'h8', 'nonsquare', 'cin_tail')),
    Row('r15_tile8', 7, 2, 16, 16, 40, 512, False, 'tile8', 9, 7, 2, 5, ('ragged', 'boundary', 'cin_tail')),
    Row('r16_tile8_bias', 5, 5, 32, 32, 8, 512, True, 'tile8', 40, 20, 3, 14, ('ragged', 'boundary', 'cin_tail')),
    Row('r17_tile8', 12, 5, 16, 16, 8, 512, False, 'tile8', 17, 12, 2, 9, ('ragged', 'cin_tail')),
    Row('r18_tile8_single_bias', 5, 0, 16, 32, 24, 40, True, 'tile8', 10, 10, 1, 10, ('nonsquare', 'cin_tail', 'cout_tail')),
    Row('r19_quad', 10, 5, 8, 16, 512, 192, False, 'quad', 15, 10, 2, 8, ('ragged', 'slices8', 'h8', 'nonsquare')),
    Row('r20_tile8_single', 9, 0, 32, 32, 40, 512, False, 'tile8', 36, 36, 5, 8, ('ragged', 'slices8', 'cin_tail')),
    Row('r21_thin', 12, 5, 64, 32, 256, 16, False, 'thin', 136, 96, 9, 16, ('ragged', 'boundary', 'slices8', 'nonsquare')),
    Row('r22_pair', 10, 5, 8, 8, 8, 8, False, 'pair', 8, 5, 1, 8, ('slices8', 'cin_tail', 'cout_tail')),
    Row('r23_quad', 6, 5, 16, 16, 256, 192, False, 'quad', 22, 12, 2, 11, ()),
    Row('r24_quad', 6, 3, 16, 16, 512, 256, False, 'quad', 18, 12, 3, 6, ()),
]


def _properties(kernel, n, nb, h, w, cin, cout, tiles, tiles_a, per_wg, slices):
  """What a row covers, from its stated numbers alone (after checking that the numbers agree with each other)."""
  if kernel == 'pair':
    seg = lambda m: (m + 1) // 2
    assert h == 8 and w == 8
  else:
    th, tw = TILE[kernel]
    assert h % th == 0 and w % tw == 0 and w != 8, (kernel, h, w)
    seg = lambda m: (h // th) * (w // tw) * m
  assert (tiles_a, tiles) == (seg(n), seg(n) + seg(nb)), ('the row states tiles / tiles_a that its batch does not have', seg(n), seg(nb))
  assert slices == -(-tiles // per_wg), 'the row states a slice count that is not ceil(tiles / per_wg)'
  have = set()
  if tiles % per_wg:
    have.add('ragged')
  if nb and tiles_a % per_wg:
    have.add('boundary')
  if kernel == 'pair' and per_wg > 1 and (n % 2 or nb % 2):
    have.add('odd')
  if slices % 8 == 0:
    have.add('slices8')
  if h % 16 == 8:
    have.add('h8')
  if h != w:
    have.add('nonsquare')
  if cin % 32:
    have.add('cin_tail')
  if cout % 32:
    have.add('cout_tail')
  return have


def _assert_covers(r, have):
  for p in r.covers:
    assert p in have, '%s no longer covers %r (its numbers give %s): move the row, do not drop the property' % (r.id, p, sorted(have))


def _golden_check(case_id, dname, rec):
  """rec of one (row, dtype) against the recorded table, or into it."""
  dst = os.environ.get(RECORD_ENV)
  if dst:
    table = {}
    if os.path.exists(dst):
      with open(dst) as fh:
        table = json.load(fh)
    table.setdefault(case_id, {})[dname] = rec
    with open(dst, 'w') as fh:
      json.dump(table, fh, indent=1, sort_keys=True)
    return
  assert os.path.exists(GOLDEN_PATH), 'record with %s=tests/golden/wgrad_split_kernels.json' % RECORD_ENV
  with open(GOLDEN_PATH) as fh:
    want = json.load(fh).get(case_id, {}).get(dname)
  assert want == rec, ('the filter-gradient split moved', case_id, dname, rec, want)


def _note(family, dname, ratio):
  """The [elementwise] line of tests/test_gpu_ops.py, and the ratio once more with its exponent: these bounds count one
  rounding per summed pixel and the kernels stay two to four orders of magnitude inside them."""
  T._ew_note(family, dname, ratio)
  print('[wgrad split ratio] %-28s %-4s %.3e' % (family, dname, ratio))


def _lib():
  from twingan_amd import _lib as L
  return L.load()


class _Deterministic:
  def __enter__(self):
    self.prev = _lib().tg_set_deterministic(1)

  def __exit__(self, *a):
    _lib().tg_set_deterministic(self.prev)


def _randn(g, shape, dtype):
  return torch.randn(*shape, generator=g).to(dtype).to(T.dev())


@functools.lru_cache(maxsize=2)
def _row_data(idx, dname):
  """Operands of a row on the device, fp32 sinks that hold values, and the float64 oracle per segment: computed once and
  shared by every test of the row (nothing below writes to any of it)."""
  r, dtype = SPLIT_ROWS[idx], DTYPES[dname]
  g = torch.Generator().manual_seed(4100 + idx)
  d = {'xa': _randn(g, (r.n, r.h, r.w, r.cin), dtype), 'gya': _randn(g, (r.n, r.h, r.w, r.cout), dtype)}
  if r.nb:
    d['xb'], d['gyb'] = _randn(g, (r.nb, r.h, r.w, r.cin), dtype), _randn(g, (r.nb, r.h, r.w, r.cout), dtype)
  d['sink'] = torch.randn(3, 3, r.cin, r.cout, generator=g).to(T.dev())
  d['bsink'] = torch.randn(r.cout, generator=g).to(T.dev())
  for s in ('a', 'b') if r.nb else ('a',):
    x, gy = T.host(d['x' + s]), T.host(d['gy' + s])
    d['ref_' + s] = N.conv2d_bwd_weight_gemm(x, gy, (3, 3))
    d['mag_' + s] = N.conv2d_bwd_weight_gemm(np.abs(x), np.abs(gy), (3, 3))
    d['bref_' + s], d['bmag_' + s] = gy.sum(axis=(0, 1, 2)), np.abs(gy).sum(axis=(0, 1, 2))
  return d


def _into_sink(bound, sink, ref, roundings=1):
  """The bound of a sum added into a sink that holds values: `roundings` fp32 roundings of sink + sum (the module docstring)."""
  return (1 + roundings * E.U32) * bound + roundings * E.U32 * (np.abs(sink) + np.abs(ref))


def _segments(r, d, segs=3):
  """(filter-gradient ref, mag, P), (bias ref, mag, P) over the segments selected by the bits of `segs`."""
  pick = [s for bit, s in ((1, 'a'), (2, 'b')) if segs & bit and ('ref_' + s) in d]
  P = sum({'a': r.n, 'b': r.nb}[s] for s in pick) * r.h * r.w
  tot = lambda key: sum(d[key + s] for s in pick)
  return (tot('ref_'), tot('mag_'), P), (tot('bref_'), tot('bmag_'), P)


def _check_gw(what, dname, got, ref, bound):
  e = T.rel_l2(got, ref)
  print('[wgrad split %s] rel-L2 %.3e (bound %.1e)' % (what, e, T.EDGE_F32_TOL))
  assert e < T.EDGE_F32_TOL, (what, e)
  return E.assert_elementwise(got, ref, bound, what)


def _workspace(O, r, dtype):
  d = O._desc((r.n, r.h, r.w, r.cin), r.cout, O.ConvSpec(3, 'SAME'), dtype, 0)
  if r.nb:
    return d, int(_lib().tg_conv2d_bwd_weight2_workspace(ctypes.byref(d), r.nb))
  return d, int(_lib().tg_conv2d_bwd_weight_workspace(ctypes.byref(d)))


def _launch(O, r, d, sink=None, bsink=None, segs=3):
  """One launch of the row through the product's wrappers -> (gw, gbias, symbol)."""
  spec = O.ConvSpec(3, 'SAME')
  gb = None if bsink is None else bsink.clone()
  if r.nb:
    out = sink.clone()      # the paired route always accumulates
    assert O.conv_bwd_weight2_raw(d['xa'], d['gya'], d['xb'], d['gyb'], spec, out, gbias=gb, bias_segs=segs), 'paired launch refused'
  else:
    out = O.conv_bwd_weight_raw(d['xa'], d['gya'], spec, out=None if sink is None else sink.clone(), gbias=gb)
  return out, gb, T._last_kernel()


def _expect_symbol(r, fused_bias):
  return 'conv_wgrad_thin_kernel<16,bias>' if (r.kernel == 'thin' and fused_bias) else SYMBOL[r.kernel]


@pytest.mark.parametrize('dname', sorted(DTYPES))
@pytest.mark.parametrize('idx', range(len(SPLIT_ROWS)), ids=[r.id for r in SPLIT_ROWS])
def test_filter_gradient_at_a_split_cell(idx, dname):
  """One row: the stated kernel ran on the stated split; filter and bias gradient element by element against the float64
  oracle, into sinks that hold values; bias_segs 1 / 2 / 3 add exactly the selected segments; the paired launch equals two
  single launches into one sink."""
  import twingan_amd.ops as O
  r, dtype = SPLIT_ROWS[idx], DTYPES[dname]
  _assert_covers(r, _properties(r.kernel, r.n, r.nb, r.h, r.w, r.cin, r.cout, r.tiles, r.tiles_a, r.per_wg, r.slices))
  assert (r.kernel == 'pair') == (r.w == 8)
  _, nbytes = _workspace(O, r, dtype)
  assert nbytes == r.slices * 36 * r.cin * r.cout, ('%s: the workspace holds %g slabs, the row states %d slices: the split moved'
                                                    % (r.id, nbytes / (36.0 * r.cin * r.cout), r.slices))
  d = _row_data(idx, dname)
  sink, bsink = T.host(d['sink']), T.host(d['bsink'])
  (ref, mag, P), _ = _segments(r, d)
  bound = E.wgrad_bound(ref, mag, P)
  rec = {'workspace': nbytes}
  worst = 0.0
  if r.nb == 0:      # single launch: once into a fresh tensor ...
    gw, _, rec['symbol'] = _launch(O, r, d)
    worst = _check_gw(r.id + ' out=None', dname, T.host(gw), ref, bound)
  # ... and (paired: always) accumulating into a sink that holds values
  gw, _, sym = _launch(O, r, d, sink=d['sink'])
  assert rec.setdefault('symbol', sym) == sym == _expect_symbol(r, False), (r.id, sym)
  plain = T.host(gw)
  worst = max(worst, _check_gw(r.id + ' into a sink', dname, plain - sink, ref, _into_sink(bound, sink, ref)))
  if r.bias:
    for segs in ((3, 1, 2) if r.nb else (3,)):
      gw, gb, sym = _launch(O, r, d, sink=d['sink'], bsink=d['bsink'], segs=segs)
      assert rec.setdefault('symbol_bias', sym) == sym == _expect_symbol(r, True), (r.id, sym)
      what = '%s bias_segs=%d' % (r.id, segs)
      worst = max(worst, _check_gw(what, dname, T.host(gw) - sink, ref, _into_sink(bound, sink, ref)))
      _, (bref, bmag, bP) = _segments(r, d, segs)
      rb = E.assert_elementwise(T.host(gb) - bsink, bref, _into_sink(E.wgrad_bound(bref, bmag, bP), bsink, bref), what + ' bias gradient')
      _note('wgrad split %s bias' % r.kernel, dname, rb)
  if r.nb:           # two single launches into one sink: two roundings of the sink, each single's own bound
    spec = O.ConvSpec(3, 'SAME')
    two = d['sink'].clone()
    O.conv_bwd_weight_raw(d['xa'], d['gya'], spec, out=two)
    O.conv_bwd_weight_raw(d['xb'], d['gyb'], spec, out=two)
    b2 = E.wgrad_bound(d['ref_a'], d['mag_a'], r.n * r.h * r.w) + E.wgrad_bound(d['ref_b'], d['mag_b'], r.nb * r.h * r.w)
    b2 = _into_sink(b2, sink, np.abs(d['ref_a']) + np.abs(d['ref_b']), roundings=2)
    E.assert_elementwise(T.host(two) - sink, ref, b2, r.id + ' two single launches')
    e = T.rel_l2(plain, T.host(two))
    assert e < 1e-5, (r.id, 'paired vs two launches', e)      # the bound of test_paired_filter_gradient_matches_two_launches
    E.assert_elementwise(plain, T.host(two), _into_sink(bound, sink, ref) + b2, r.id + ' paired vs two single launches')
  _note('wgrad split ' + r.kernel, dname, worst)
  _golden_check(r.id, dname, rec)


# ---------------------------------------------------------------------------------------------- concat input
URow = collections.namedtuple('URow', 'id n h w c0 c1 cout gsz perm kernel tiles per_wg slices ws_slices covers')

# tg_conv2d_upcat_bwd_weight: conv3x3(concat(up2(x0), skip)) read from its two sources.  ws_slices: the workspace query does
# not know where the input splits, so it is sized for the larger of the quadrant and the tile split; `slices` is the launch's.
UPCAT_ROWS = [
    # cin > cout, all multiples of 64, but the sources meet at channel 32: the quadrant kernel refuses, the tile kernel runs
    URow('u1_tile4_quad_refused', 17, 16, 16, 32, 96, 64, 0, (), 'tile4', 34, 2, 17, 34, ('quad_refused',)),
    URow('u2_quad', 17, 32, 32, 64, 64, 64, 0, (), 'quad', 136, 2, 68, 68, ()),
    # three groups of 7 images read skip groups 1, 0, 1; the last range holds one tile
    URow('u3_tile8_perm', 21, 16, 16, 32, 32, 256, 7, (1, 0, 1), 'tile8', 21, 2, 11, 11, ('ragged', 'perm')),
    URow('u4_tile4_8x16', 11, 8, 16, 288, 224, 192, 0, (), 'tile4', 11, 6, 2, 6, ('ragged', 'h8', 'nonsquare', 'quad_refused')),
]


def _upcat_operands(r, dtype, seed):
  g = torch.Generator().manual_seed(seed)
  n1 = (max(r.perm) + 1) * r.gsz if r.gsz else r.n
  x0 = _randn(g, (r.n, r.h // 2, r.w // 2, r.c0), dtype)
  x1 = _randn(g, (n1, r.h, r.w, r.c1), dtype)
  gy = _randn(g, (r.n, r.h, r.w, r.cout), dtype)
  sink = torch.randn(3, 3, r.c0 + r.c1, r.cout, generator=g).to(T.dev())
  src = [r.perm[i // r.gsz] * r.gsz + i % r.gsz if r.gsz else i for i in range(r.n)]      # the skip image that image i reads
  cat = np.concatenate([T.host(x0).repeat(2, axis=1).repeat(2, axis=2), T.host(x1)[src]], axis=3)
  return x0, x1, gy, sink, cat


def _upcat_call(O, r, x0, x1, gy, gw, accumulate, ws_ptr, nbytes):
  return _lib().tg_conv2d_upcat_bwd_weight(x0.data_ptr(), x1.data_ptr(), gy.data_ptr(), gw.data_ptr(), accumulate, ws_ptr, nbytes,
                                           r.n, r.h, r.w, r.c0, r.c1, r.cout, r.gsz, O._pack_perm(r.perm), O._dt(gy), O._stream())


@pytest.mark.parametrize('dname', sorted(DTYPES))
@pytest.mark.parametrize('idx', range(len(UPCAT_ROWS)), ids=[r.id for r in UPCAT_ROWS])
def test_concat_input_filter_gradient_at_a_split_cell(idx, dname):
  import twingan_amd.ops as O
  r, dtype = UPCAT_ROWS[idx], DTYPES[dname]
  cin = r.c0 + r.c1
  have = _properties(r.kernel, r.n, 0, r.h, r.w, cin, r.cout, r.tiles, r.tiles, r.per_wg, r.slices)
  if r.gsz and tuple(r.perm) != tuple(range(len(r.perm))) and len(set(r.perm)) < len(r.perm):
    have.add('perm')      # a permutation that is not the identity and reads one skip group twice
  if cin % 64 == 0 and r.cout % 64 == 0 and cin > r.cout and r.c0 % 64:
    have.add('quad_refused')
  _assert_covers(r, have)
  nbytes = int(_lib().tg_conv2d_upcat_bwd_weight_workspace(r.n, r.h, r.w, r.c0, r.c1, r.cout))
  assert nbytes == r.ws_slices * 36 * cin * r.cout and r.ws_slices >= r.slices, (r.id, nbytes / (36.0 * cin * r.cout), r.ws_slices)
  x0, x1, gy, sink_d, cat = _upcat_operands(r, dtype, 4300 + idx)
  ref = N.conv2d_bwd_weight_gemm(cat, T.host(gy), (3, 3))
  bound = E.wgrad_bound(ref, N.conv2d_bwd_weight_gemm(np.abs(cat), np.abs(T.host(gy)), (3, 3)), r.n * r.h * r.w)
  ws = torch.empty(nbytes, dtype=torch.uint8, device=T.dev())
  gw = torch.full((3, 3, cin, r.cout), float('nan'), device=T.dev())
  assert _upcat_call(O, r, x0, x1, gy, gw, 0, ws.data_ptr(), nbytes) == 0, _lib().tg_last_error()
  sym = T._last_kernel()
  assert sym == SYMBOL[r.kernel], (r.id, sym)
  worst = _check_gw(r.id + ' accumulate=0', dname, T.host(gw), ref, bound)
  acc = sink_d.clone()
  assert _upcat_call(O, r, x0, x1, gy, acc, 1, ws.data_ptr(), nbytes) == 0, _lib().tg_last_error()
  sink = T.host(sink_d)
  worst = max(worst, _check_gw(r.id + ' into a sink', dname, T.host(acc) - sink, ref, _into_sink(bound, sink, ref)))
  # the launch needs exactly the stated slices: one byte less is refused and the sink stays as it was
  need = r.slices * 36 * cin * r.cout
  keep = sink_d.clone()
  assert _upcat_call(O, r, x0, x1, gy, keep, 1, ws.data_ptr(), need - 1) == TG_EINVAL
  assert torch.equal(keep, sink_d)
  assert _upcat_call(O, r, x0, x1, gy, keep, 1, ws.data_ptr(), need) == 0, _lib().tg_last_error()
  assert torch.equal(keep, acc)
  _note('wgrad split upcat ' + r.kernel, dname, worst)
  _golden_check(r.id, dname, {'symbol': sym, 'workspace': nbytes})


# ---------------------------------------------------------------------------------------------- first-generation kernel
GRow = collections.namedtuple('GRow', 'id k n h w cin cout tile_img tile_h tiles per_wg slices')

# conv_wgrad_mfma<1,1> / <3,3> (conv_mfma.hip wgrad_split) at maps the tile kernels refuse; a tile is 128 pixels:
# tile_img images x tile_h rows x 16 (4x4 maps: 4) columns.  Every row is ragged: the slice count does not divide the tiles.
GEN1_ROWS = [
    GRow('g1_k3_12x12', 3, 5, 12, 12, 512, 512, 1, 8, 10, 4, 3),
    GRow('g2_k1_20x12', 1, 3, 20, 12, 256, 512, 1, 8, 9, 2, 5),
    GRow('g3_k3_4x4_odd', 3, 33, 4, 4, 512, 512, 8, 4, 5, 2, 3),
    GRow('g4_k1_4x4_odd', 1, 33, 4, 4, 512, 512, 8, 4, 5, 2, 3),
]


@pytest.mark.parametrize('dname', sorted(DTYPES))
@pytest.mark.parametrize('idx', range(len(GEN1_ROWS)), ids=[r.id for r in GEN1_ROWS])
def test_first_generation_filter_gradient_at_a_ragged_split(idx, dname):
  import twingan_amd.ops as O
  r, dtype = GEN1_ROWS[idx], DTYPES[dname]
  assert r.tiles == -(-r.n // r.tile_img) * -(-r.h // r.tile_h), 'the row states tiles that its batch does not have'
  assert r.slices == -(-r.tiles // r.per_wg), 'the row states a slice count that is not ceil(tiles / per_wg)'
  assert r.tiles % r.per_wg and r.tiles % r.slices, '%s no longer covers a ragged last slice' % r.id
  assert r.tile_img == 1 or r.n % 2, '%s no longer covers an odd batch' % r.id
  spec = O.ConvSpec(r.k, 'SAME')
  d = O._desc((r.n, r.h, r.w, r.cin), r.cout, spec, dtype, 0)
  nbytes = int(_lib().tg_conv2d_bwd_weight_workspace(ctypes.byref(d)))
  assert nbytes == r.slices * 4 * r.k * r.k * r.cin * r.cout, (r.id, nbytes / (4.0 * r.k * r.k * r.cin * r.cout), r.slices)
  g = torch.Generator().manual_seed(4400 + idx)
  x, gy = _randn(g, (r.n, r.h, r.w, r.cin), dtype), _randn(g, (r.n, r.h, r.w, r.cout), dtype)
  sink_d = torch.randn(r.k, r.k, r.cin, r.cout, generator=g).to(T.dev())
  ref = N.conv2d_bwd_weight_gemm(T.host(x), T.host(gy), (r.k, r.k))
  bound = E.wgrad_bound(ref, N.conv2d_bwd_weight_gemm(np.abs(T.host(x)), np.abs(T.host(gy)), (r.k, r.k)), r.n * r.h * r.w)
  gw = O.conv_bwd_weight_raw(x, gy, spec)
  sym = T._last_kernel()
  assert sym == 'conv_wgrad_mfma<%d,%d>' % (r.k, r.k), (r.id, sym)
  worst = _check_gw(r.id + ' out=None', dname, T.host(gw), ref, bound)
  acc = O.conv_bwd_weight_raw(x, gy, spec, out=sink_d.clone())
  sink = T.host(sink_d)
  worst = max(worst, _check_gw(r.id + ' into a sink', dname, T.host(acc) - sink, ref, _into_sink(bound, sink, ref)))
  _note('wgrad split gen1 k%d' % r.k, dname, worst)
  _golden_check(r.id, dname, {'symbol': sym, 'workspace': nbytes})


# ---------------------------------------------------------------------------------------------- planted structure
# kernel, n, nb, h, w, cin, cout: the smallest paired launch of each kernel on a non-square map (the pair kernel's map is 8x8:
# there the planted image is the last one of an odd segment)
PLANT_CASES = [('pair', 1, 3, 8, 8, 32, 32), ('tile4', 1, 1, 24, 16, 32, 32), ('tile8', 1, 1, 16, 32, 32, 32),
               ('quad', 2, 1, 8, 16, 128, 64), ('thin', 1, 1, 64, 32, 16, 16)]


@pytest.mark.parametrize('dname', sorted(DTYPES))
@pytest.mark.parametrize('case', PLANT_CASES, ids=[c[0] for c in PLANT_CASES])
def test_filter_gradient_is_not_transposed(case, dname):
  """In the spirit of test_conv_mfma_transpose_detecting: x one-hot at one asymmetric pixel of the last image of each segment,
  gy one-hot where ONE chosen tap pairs it with that pixel.  All operands and sums are exactly representable: the gradient is
  the sink plus exactly two ones.  Swapped rows / columns, a flipped tap or a segment read from the other's tensors move
  or lose a one."""
  import twingan_amd.ops as O
  kernel, n, nb, h, w, cin, cout = case
  dtype = DTYPES[dname]
  xa, ga = np.zeros((n, h, w, cin)), np.zeros((n, h, w, cout))
  xb, gb = np.zeros((nb, h, w, cin)), np.zeros((nb, h, w, cout))
  # gw[ky, kx, ci, co] = sum_p x[p + (ky - 1, kx - 1), ci] gy[p, co]
  plants = [(xa, ga, n - 1, (h - 3, 2), (0, 2), 3, cout - 2),      # x pixel (row, col), tap (ky, kx), ci, co
            (xb, gb, nb - 1, (1, w - 2), (2, 1), cin - 5, 9)]
  want = np.zeros((3, 3, cin, cout))
  for x, gy, img, (py, px), (ky, kx), ci, co in plants:
    x[img, py, px, ci] = 1.0
    gy[img, py - (ky - 1), px - (kx - 1), co] = 1.0
    want[ky, kx, ci, co] = 1.0
  assert np.array_equal(N.conv2d_bwd_weight_gemm(xa, ga, (3, 3)) + N.conv2d_bwd_weight_gemm(xb, gb, (3, 3)), want)
  sink = torch.randint(-8, 9, (3, 3, cin, cout), generator=torch.Generator().manual_seed(5)).float().to(T.dev())
  out = sink.clone()
  td = lambda a: T.to_dev(a, dtype)
  assert O.conv_bwd_weight2_raw(td(xa), td(ga), td(xb), td(gb), O.ConvSpec(3, 'SAME'), out)
  assert T._last_kernel() == SYMBOL[kernel], T._last_kernel()
  got = T.host(out) - T.host(sink)
  assert np.array_equal(got, want), ('ones at', np.argwhere(got != 0).tolist(), 'expected at', np.argwhere(want != 0).tolist())


# ---------------------------------------------------------------------------------------------- the C entry points directly
def _row(rid):
  return [r.id for r in SPLIT_ROWS].index(rid)


def _direct(O, r, d, desc, gw, accumulate, ws_ptr, nbytes):
  lib, s = _lib(), O._stream()
  if r.nb:
    return lib.tg_conv2d_bwd_weight2(ctypes.byref(desc), r.nb, d['xa'].data_ptr(), d['gya'].data_ptr(), d['xb'].data_ptr(),
                                     d['gyb'].data_ptr(), gw.data_ptr(), accumulate, ws_ptr, nbytes, s)
  return lib.tg_conv2d_bwd_weight(ctypes.byref(desc), d['xa'].data_ptr(), d['gya'].data_ptr(), gw.data_ptr(), accumulate, ws_ptr,
                                  nbytes, s)


@pytest.mark.parametrize('dname', sorted(DTYPES))
@pytest.mark.parametrize('rid', ['r18_tile8_single_bias', 'r07_quad_single'])
def test_workspace_off_the_16_byte_grid_takes_the_scalar_slab_stores(rid, dname):
  """The C ABI does not refuse a workspace that is 4 bytes past a 16-byte boundary: the kernels then store their slabs
  element by element (vec_ok = 0) and the result is bit-equal to the aligned call's."""
  import twingan_amd.ops as O
  idx = _row(rid)
  r, dtype, d = SPLIT_ROWS[idx], DTYPES[dname], _row_data(idx, dname)
  desc, nbytes = _workspace(O, r, dtype)
  ws = torch.zeros(nbytes + 32, dtype=torch.uint8, device=T.dev())
  base = ws.data_ptr() + (-ws.data_ptr()) % 16
  res = []
  for off in (0, 4):
    gw = torch.full((3, 3, r.cin, r.cout), float('nan'), device=T.dev())
    assert _direct(O, r, d, desc, gw, 0, base + off, nbytes) == 0, _lib().tg_last_error()
    assert T._last_kernel() == SYMBOL[r.kernel]
    res.append(gw)
  assert torch.equal(res[0], res[1])
  (ref, mag, P), _ = _segments(r, d)
  _check_gw(rid + ' misaligned workspace', dname, T.host(res[1]), ref, E.wgrad_bound(ref, mag, P))


@pytest.mark.parametrize('dname', sorted(DTYPES))
@pytest.mark.parametrize('rid', ['r07_quad_single', 'r15_tile8', 'r09_thin'])
def test_short_workspace_is_refused_and_the_gradient_untouched(rid, dname):
  """One byte less than the launch needs: TG_EINVAL from the single and the paired entry point (the concat entry point: in
  test_concat_input_filter_gradient_at_a_split_cell), with and without the bias gradient, and nothing written."""
  import twingan_amd.ops as O
  idx = _row(rid)
  r, dtype, d = SPLIT_ROWS[idx], DTYPES[dname], _row_data(idx, dname)
  desc, nbytes = _workspace(O, r, dtype)
  ws = torch.empty(nbytes, dtype=torch.uint8, device=T.dev())
  gw = torch.full((3, 3, r.cin, r.cout), -7.5, device=T.dev())
  gb = torch.full((r.cout,), -7.5, device=T.dev())
  for accumulate in (0, 1):
    assert _direct(O, r, d, desc, gw, accumulate, ws.data_ptr(), nbytes - 1) == TG_EINVAL
  lib, s = _lib(), O._stream()
  if r.nb:
    rc = lib.tg_conv2d_bwd_weight2_bias(ctypes.byref(desc), r.nb, d['xa'].data_ptr(), d['gya'].data_ptr(), d['xb'].data_ptr(),
                                        d['gyb'].data_ptr(), gw.data_ptr(), gb.data_ptr(), 3, 1, ws.data_ptr(), nbytes - 1, s)
  else:
    rc = lib.tg_conv2d_bwd_weight_bias(ctypes.byref(desc), d['xa'].data_ptr(), d['gya'].data_ptr(), gw.data_ptr(), gb.data_ptr(), 1,
                                       ws.data_ptr(), nbytes - 1, s)
  assert rc == TG_EINVAL
  assert bool((gw == -7.5).all()) and bool((gb == -7.5).all())


@pytest.mark.parametrize('dname', sorted(DTYPES))
@pytest.mark.parametrize('rid', ['r05_pair_bias', 'r10_thin_bias', 'r12_tile4_bias', 'r16_tile8_bias'])
def test_deterministic_mode_at_a_split_cell(rid, dname):
  """Deterministic mode (the bias gradient leaves the filter-gradient kernel: no float atomics across workgroups): two runs
  are bit-equal, inside the same bounds, and the kernel without the bias MFMA ran."""
  import twingan_amd.ops as O
  idx = _row(rid)
  r, d = SPLIT_ROWS[idx], _row_data(idx, dname)
  with _Deterministic():
    assert O.deterministic()
    runs = [_launch(O, r, d, sink=d['sink'], bsink=d['bsink']) for _ in range(2)]
  assert not O.deterministic()
  (gw0, gb0, sym), (gw1, gb1, _) = runs
  assert torch.equal(gw0, gw1) and torch.equal(gb0, gb1)
  assert sym == _expect_symbol(r, False), sym
  sink, bsink = T.host(d['sink']), T.host(d['bsink'])
  (ref, mag, P), (bref, bmag, _) = _segments(r, d)
  _check_gw(rid + ' deterministic', dname, T.host(gw0) - sink, ref, _into_sink(E.wgrad_bound(ref, mag, P), sink, ref))
  E.assert_elementwise(T.host(gb0) - bsink, bref, _into_sink(E.wgrad_bound(bref, bmag, P), bsink, bref),
                       rid + ' deterministic bias gradient')
  _golden_check(rid + ':deterministic', dname, {'symbol': sym})
