"""Sliced Wasserstein distance on the GPU (ops.swd_*: the HIP kernels of twingan_amd/csrc/preprocess.hip;
evaluate.SlicedWasserstein) against the float64 restatement of the algorithm (tests/swd_np.py; there is no reference code to
run: image_generation.py:926-931).

Bounds.  Pyramid levels and projections, element by element: elementwise.e32_bound = 2^-24 |ref| + 16 E32, E32 = max |float32
restatement - float64| of that level / that projection.  Statistics: 16 E32 against the float64 value (both evaluations
accumulate them in float64, so E32 is the distance of the true value to the float32 grid -- the least a stored fp32 can be off
by).  Gathers and sorts are exact.  Distances: 4 |float32 restatement - float64| + 1e-6 |float64| (the factor 4 for a third
summation order, as in tests/test_gpu_metrics.py).  Shapes are the smallest at which each kernel can still go wrong."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import elementwise as EW      # noqa: E402
import swd_np as S      # noqa: E402

pytestmark = pytest.mark.gpu
TORCH_DT = {'fp32': torch.float32, 'bf16': torch.bfloat16, 'fp16': torch.float16}
DEV = 'cuda:0'
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _dev(x, dtype='fp32'):
  return torch.from_numpy(np.ascontiguousarray(x)).to(DEV).to(TORCH_DT[dtype]).contiguous()


def _stored(x, dtype):
  """The values the kernel reads: the float32 array rounded to the storage type."""
  return torch.from_numpy(np.ascontiguousarray(x)).to(TORCH_DT[dtype]).float().numpy()


def _np(t):
  return t.detach().cpu().numpy()


# ---- pyramid -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('quantize', [True, False])
@pytest.mark.parametrize('dtype', ['fp32', 'bf16', 'fp16'])
@pytest.mark.parametrize('hw', [16, 32, 64])
def test_pyramid_every_element(hw, dtype, quantize):
  from twingan_amd import ops
  x = S.images(8100 + hw, 5, hw)
  got = ops.swd_pyramid(_dev(x, dtype), quantize=quantize)
  v = S.pixels(_stored(x, dtype), 255., quantize)
  ref, ref32 = S.pyramid(v), S.pyramid(v, np.float32)
  assert [tuple(g.shape) for g in got] == [(5, s, s, 3) for s in S.resolutions(hw)]
  for l, g in enumerate(got):
    assert g.dtype == torch.float32
    e32 = EW.e32(ref32[l], ref[l])
    worst = EW.assert_elementwise(_np(g).astype(np.float64), ref[l], EW.e32_bound(ref[l], e32, 'f32'),
                                  'swd pyramid hw %d %s quantize %d level %d' % (hw, dtype, quantize, l))
    print('hw %d %s q%d level %d: E32 %.3e worst ratio %.3f' % (hw, dtype, quantize, l, e32, worst))
  if hw == 16 and quantize:      # a single level is the quantised image itself
    assert np.array_equal(_np(got[0]), v)


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_pyramid_does_not_depend_on_the_batch(dtype):
  from twingan_amd import ops
  x = _dev(S.images(8200, 5, 64), dtype)
  whole = [_np(t) for t in ops.swd_pyramid(x)]
  for i in range(5):
    for a, b in zip(ops.swd_pyramid(x[i:i + 1].contiguous()), whole):
      assert np.array_equal(_np(a)[0], b[i])


# ---- descriptors ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('per', [1, 16, 128])
def test_descriptors_equal_a_gather_of_the_kernels_own_pyramid(per):
  from twingan_amd import ops
  n = 3
  levels = ops.swd_pyramid(_dev(S.images(8300, n, 32)))
  for l, level in enumerate(levels):
    s = level.shape[1]
    tab = S.centre_table(8310 + l, n * per, s)
    forced = np.array([[3, 3], [s - 4, s - 4], [3, s - 4], [s - 4, 3], [5, 7], [5, 7]], np.int32)      # both ends, a repeat
    if per >= 16:
      tab[:6], tab[-6:] = forced, forced
    else:
      tab[:] = forced[:n * per]
    offset = 5
    out = torch.full((offset + n * per + 2, S.K), -7.0, device=DEV)
    ret = ops.swd_descriptors(level, tab, per, out=out, row_offset=offset)
    assert ret.data_ptr() == out.data_ptr()
    got = _np(out)
    assert np.array_equal(got[offset:offset + n * per], S.descriptors(_np(level), tab, per))
    assert np.all(got[:offset] == -7.0) and np.all(got[offset + n * per:] == -7.0)
    fresh = ops.swd_descriptors(level, torch.from_numpy(tab), per)
    assert np.array_equal(_np(fresh), got[offset:offset + n * per])


# ---- statistics and projection -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', ['dc_offset', 'flat_channel'])
@pytest.mark.parametrize('n', [1, 2, 147, 768])
def test_projection_every_element(n, family):
  from twingan_amd import ops
  desc = S.dc_offset_set(8400 + n, n) if family == 'dc_offset' else S.flat_channel_set(8400 + n, n)
  dirs = S.directions(8450 + n, 2, 24)      # 48 columns: one full chunk of 32 and a ragged one
  proj, mean, rstd = ops.swd_project(_dev(desc), _dev(dirs))
  npad = ops.swd_npad(n)
  assert tuple(proj.shape) == (48, npad) and npad >= n and npad & (npad - 1) == 0 and npad < 2 * max(n, 1)
  m64, r64 = S.statistics(desc)
  for got, want in ((mean, m64), (rstd, r64)):
    e32 = np.abs(want.astype(np.float32).astype(np.float64) - want)
    err = np.abs(_np(got).astype(np.float64) - want)
    print('%s n %d: statistics err %s E32 %s' % (family, n, err, e32))
    assert np.all(err <= 16.0 * e32.max()), (err, e32)
  if family == 'flat_channel' and n > 1:
    assert _np(rstd)[1] == 0.0 and _np(mean)[1] == np.float32(37.25)
  got = _np(proj)
  assert np.isfinite(got[:, :n]).all()
  assert np.all(np.isposinf(got[:, n:]))
  want = np.stack([S.normalise(desc) @ dirs[r].astype(np.float64) for r in range(2)])            # [R, N, D]
  want32 = np.stack([S.normalise(desc, np.float32) @ dirs[r] for r in range(2)])
  want, want32 = want.transpose(0, 2, 1).reshape(48, n), want32.transpose(0, 2, 1).reshape(48, n)
  e32 = EW.e32(want32, want)
  worst = EW.assert_elementwise(got[:, :n].astype(np.float64), want, EW.e32_bound(want, e32, 'f32'),
                                'swd projection %s n %d' % (family, n))
  print('%s n %d: projection E32 %.3e worst ratio %.3f' % (family, n, e32, worst))


def test_statistics_of_more_chunks_than_one_pass_of_the_second_stage():
  """N > 256 * 256 rows: the second stage walks the chunk sums in more than one trip; and a column count below one chunk."""
  from twingan_amd import ops
  n = 256 * 256 + 300
  desc = S.dc_offset_set(8470, n)
  dirs = S.directions(8471, 1, 3)
  proj, mean, rstd = ops.swd_project(_dev(desc), _dev(dirs))
  m64, r64 = S.statistics(desc)
  for got, want in ((mean, m64), (rstd, r64)):
    e32 = np.abs(want.astype(np.float32).astype(np.float64) - want)
    assert np.all(np.abs(_np(got).astype(np.float64) - want) <= 16.0 * e32.max())
  got = _np(proj)
  want = (S.normalise(desc) @ dirs[0].astype(np.float64)).T
  want32 = (S.normalise(desc, np.float32) @ dirs[0]).T
  EW.assert_elementwise(got[:, :n].astype(np.float64), want, EW.e32_bound(want, EW.e32(want32, want), 'f32'), 'swd projection, many chunks')
  assert got.shape == (3, 131072) and np.all(np.isposinf(got[:, n:]))


def test_mean_abs_diff_over_several_row_chunks():
  """More than one 4096-row chunk per column and more than 256 chunk sums per repeat; the +inf tail must not be read.
  Bound: every |a - b| is one fp32 subtraction (2^-24 relative), the sums are double, the result is rounded to fp32 once."""
  from twingan_amd import ops
  n, r, d = 4 * ops.SWD_SORT_BLOCK + 5, 2, 80
  npad = ops.swd_npad(n)
  rs = np.random.RandomState(8480)
  a, b = np.full((r * d, npad), np.inf, np.float32), np.full((r * d, npad), np.inf, np.float32)
  a[:, :n], b[:, :n] = np.sort(rs.randn(r * d, n), axis=1), np.sort(rs.randn(r * d, n) * 1.5 + 0.2, axis=1)
  mean, per = ops.swd_mean_abs_diff(_dev(a), _dev(b), n, r)
  want = np.abs(a[:, :n].astype(np.float64) - b[:, :n].astype(np.float64)).reshape(r, d * n).mean(axis=1)
  assert np.all(np.abs(_np(per).astype(np.float64) - want) <= 2.0 * EW.U32 * want + EW.TINY), (_np(per), want)
  assert abs(float(_np(mean)[0]) - want.mean()) <= 3.0 * EW.U32 * want.mean() + EW.TINY
  again = ops.swd_mean_abs_diff(_dev(a), _dev(b), n, r)
  assert torch.equal(again[0], mean) and torch.equal(again[1], per)


# ---- sort ----------------------------------------------------------------------------------------------------------------
def _sort_sizes():
  from twingan_amd import ops
  b = ops.SWD_SORT_BLOCK
  return [1, 2, 768, b - 1, b, b + 1, 4 * b + 5]


@pytest.mark.parametrize('which', range(7))
def test_sort_columns_equals_np_sort(which):
  from twingan_amd import _lib, ops
  assert _lib.load().tg_swd_sort_block() == ops.SWD_SORT_BLOCK
  n = _sort_sizes()[which]
  npad = ops.swd_npad(n)
  rs = np.random.RandomState(8500 + which)
  cols = [rs.randn(n), np.round(rs.randn(n) * 2) / 2, np.sort(rs.randn(n)), np.sort(rs.randn(n))[::-1],
          np.where(rs.rand(n) < 0.5, 0.0, -0.0) * np.where(rs.rand(n) < 0.3, 0.0, 1.0) + np.where(rs.rand(n) < 0.2, rs.randn(n), 0.0)]
  keys = np.full((len(cols), npad), np.inf, np.float32)
  for i, c in enumerate(cols):
    keys[i, :n] = c.astype(np.float32)
  got = _np(ops.swd_sort_columns(_dev(keys)))
  assert np.array_equal(got[:, :n], np.sort(keys[:, :n], axis=1))
  assert np.all(np.isposinf(got[:, n:]))


# ---- distance and accumulator ----------------------------------------------------------------------------------------------
def _fed_case(seed, hw, sizes, per):
  reals = [S.images(seed + 10 * k, n, hw) for k, n in enumerate(sizes)]
  fakes = [np.clip(0.85 * S.images(seed + 10 * k + 5, n, hw, noise=0.12) + 0.05, 0, 1).astype(np.float32) for k, n in enumerate(sizes)]
  centres = [[(S.centre_table(seed + 100 * k + 2 * l, n * per, s), S.centre_table(seed + 100 * k + 2 * l + 1, n * per, s))
              for l, s in enumerate(S.resolutions(hw))] for k, n in enumerate(sizes)]
  return reals, fakes, centres


def _run_accumulator(reals, fakes, centres, dirs, hw, per, dtype='fp32'):
  from twingan_amd.evaluate import SlicedWasserstein
  acc = SlicedWasserstein(hw, sum(r.shape[0] for r in reals), per=per, repeats=dirs[0].shape[0], dirs=dirs[0].shape[2])
  acc.begin()
  for r, f, c in zip(reals, fakes, centres):
    acc.feed(_dev(r, dtype), _dev(f, dtype), centres=c)
  return acc.end(dirs=[torch.from_numpy(d) for d in dirs])


@pytest.mark.parametrize('case', ['small', 'defaults'])
def test_accumulator_matches_the_restatement(case):
  hw, sizes = 32, (4, 6, 2)
  per, r, d = (16, 2, 16) if case == 'small' else (128, 4, 128)
  reals, fakes, centres = _fed_case(8600, hw, sizes, per)
  dirs = [S.directions(8650 + l, r, d) for l in range(2)]
  got = _run_accumulator(reals, fakes, centres, dirs, hw, per)
  assert got['resolutions'] == [32, 16]
  want = S.swd(reals, fakes, centres, dirs, per)
  want32 = S.swd(reals, fakes, centres, dirs, per, dtype=np.float32)
  for key, w, w32 in (('real', want[0], want32[0]), ('fake', want[1], want32[1])):
    for l in range(2):
      bound = 4.0 * abs(w32[l] - w[l]) + 1e-6 * abs(w[l])
      print('%s %s level %d: got %.9f want %.9f f32 %.9f bound %.3e' % (case, key, l, got[key][l], w[l], w32[l], bound))
      assert abs(got[key][l] - w[l]) <= bound, (key, l, got[key][l], w[l], bound)
  assert got['average'] == (sum(got['real']) / 2, sum(got['fake']) / 2)


def test_identical_sets_score_exactly_zero_and_runs_are_bit_identical():
  from twingan_amd.evaluate import SlicedWasserstein
  x = [_dev(S.images(8700 + k, n, 32), 'bf16') for k, n in enumerate((4, 2))]
  y = [_dev(S.images(8750 + k, n, 32), 'bf16') for k, n in enumerate((4, 2))]
  same = SlicedWasserstein(32, 6, per=16, repeats=2, dirs=16)
  same.begin()
  for k, t in enumerate(x):
    c = [(S.centre_table(8760 + 10 * k + l, t.shape[0] * 16, s),) * 2 for l, s in enumerate((32, 16))]
    same.feed(t, t, centres=c)
  assert same.end()['fake'] == [0.0, 0.0]

  def run(seed):
    acc = SlicedWasserstein(32, 6, per=16, repeats=2, dirs=16, seed=seed)
    acc.begin()
    for a, b in zip(x, y):
      acc.feed(a, b)
    return acc.end()
  first, again, other = run(3), run(3), run(4)
  assert first == again
  assert first['fake'] != other['fake'] and first['real'] != other['real']
  assert all(v > 0.0 for v in first['fake'] + first['real'])


def test_an_odd_number_of_images_raises_on_end():
  from twingan_amd._lib import TgError
  from twingan_amd.evaluate import SlicedWasserstein
  acc = SlicedWasserstein(16, 4, per=4, repeats=1, dirs=4)
  acc.begin()
  x = _dev(S.images(8800, 3, 16))
  acc.feed(x, x)
  with pytest.raises(TgError, match='even'):
    acc.end()
  with pytest.raises(TgError, match='buffers hold'):
    acc.feed(x, x)


# ---- evaluate_translation --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_evaluate_translation_with_targets(precision):
  """The SWD columns of a stage at the size of tests/golden/infer_hw16_c8_*: equal to the restatement applied to the very images
  twingan.translate produced, with the draws SlicedWasserstein makes at its defaults (seed 0)."""
  from twingan_amd import Config
  from twingan_amd.evaluate import SlicedWasserstein, evaluate_translation
  from twingan_amd.inference import ImageInferer
  from twingan_amd.twingan import translate
  g = dict(np.load(os.path.join(GOLDEN, 'infer_hw16_c8_instance_norm.npz')))
  sd = {k[len('param/'):]: torch.from_numpy(v).float() for k, v in g.items() if k.startswith('param/')}
  cfg = Config(hw=16, max_ch=8, precision=precision, generator_norm_type='instance_norm')
  src, tgt = S.images(8900, 8, 16), S.images(8950, 8, 16)
  got = evaluate_translation(cfg, sd, src, to='t', batch=4, device=DEV, targets=tgt)
  assert sorted(got) == ['ms_ssim_cycle', 'ms_ssim_diversity', 'swd_fake', 'swd_real', 'swd_resolutions']
  assert got['swd_resolutions'] == [16]
  plain = evaluate_translation(cfg, sd, src, to='t', batch=4, device=DEV)
  assert sorted(plain) == ['ms_ssim_cycle', 'ms_ssim_diversity']
  assert plain['ms_ssim_cycle'] == got['ms_ssim_cycle'] and plain['ms_ssim_diversity'] == got['ms_ssim_diversity']

  inf = ImageInferer(cfg, sd, device=DEV)
  x = _dev(src, precision)
  with torch.cuda.device(inf.device):
    ys = [translate(inf.store.P, x[i:i + 4].contiguous(), cfg, 't', None) for i in (0, 4)]
  draws = SlicedWasserstein(16, 8)
  draws.begin()
  centres = [[tuple(t.numpy() for t in pair) for pair in draws.draw_centres(4)] for _ in range(2)]
  dirs = [d.numpy() for d in draws.draw_dirs()]
  reals = [_stored(tgt[i:i + 4], precision) for i in (0, 4)]
  fakes = [y.float().cpu().numpy() for y in ys]
  want = S.swd(reals, fakes, centres, dirs, 128)
  want32 = S.swd(reals, fakes, centres, dirs, 128, dtype=np.float32)
  for key, w, w32 in (('swd_real', want[0], want32[0]), ('swd_fake', want[1], want32[1])):
    bound = 4.0 * abs(w32[0] - w[0]) + 1e-6 * abs(w[0])
    print('%s %s: got %.9f want %.9f bound %.3e' % (precision, key, got[key][0], w[0], bound))
    assert abs(got[key][0] - w[0]) <= bound, (key, got[key][0], w[0], bound)


def test_identity_stand_in_feeds_its_output_as_fakes():
  from twingan_amd import Config
  from twingan_amd.evaluate import evaluate_translation
  src = S.images(9000, 6, 16)
  got = evaluate_translation(Config(hw=16, max_ch=8, precision='bf16'), None, src, batch=4, device=DEV,
                             translate_fn=lambda x, to: x, targets=S.images(9050, 6, 16))
  assert got['swd_resolutions'] == [16] and got['swd_fake'][0] > 0.0 and got['swd_real'][0] > 0.0


# ---- errors ----------------------------------------------------------------------------------------------------------------
def test_swd_errors_are_loud():
  from twingan_amd import ops
  from twingan_amd._lib import TgError
  from twingan_amd.evaluate import SlicedWasserstein
  with pytest.raises(TgError, match='power of two'):
    ops.swd_pyramid(torch.zeros(1, 8, 8, 3, device=DEV))
  with pytest.raises(TgError, match='power of two'):
    ops.swd_pyramid(torch.zeros(1, 48, 48, 3, device=DEV))
  with pytest.raises(TgError, match='c = 3'):
    ops.swd_pyramid(torch.zeros(1, 16, 16, 1, device=DEV))
  with pytest.raises(ValueError, match='power of two'):
    SlicedWasserstein(8, 2)
  level = ops.swd_pyramid(torch.zeros(1, 16, 16, 3, device=DEV))[0]
  for bad in ([[2, 5]], [[5, 13]], [[-1, 5]]):
    with pytest.raises(TgError, match='outside'):
      ops.swd_descriptors(level, np.array(bad, np.int32), 1)
  ops.swd_descriptors(level, np.array([[3, 12]], np.int32), 1)
  dirs = _dev(S.directions(9100, 1, 4))
  a, b = _dev(S.dc_offset_set(9101, 8)), _dev(S.dc_offset_set(9102, 6))
  with pytest.raises(TgError, match='same number'):
    ops.swd_distance(a, b, dirs)
