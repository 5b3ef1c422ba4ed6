"""CPU, no kernels: the element-wise checker (tests/elementwise.py) checked against the rel-L2 thresholds it stands beside.

On float64 references at the bench's shapes -- the 64 x 256 x 256 x 16 forward of `k3:c32>16`, a 32 x 128 x 128 x 64 normaliser
output with its pooled tensor, a 256-channel parameter gradient -- the clean reference rounded to bf16 passes the new check with a
ratio <= 1, and each planted fault (a numpy edit of that rounded tensor, of the kind kernels produce: one pixel, a tile edge,
a channel group, a tail chunk, one channel of a reduction) PASSES the rel-L2 threshold that guards the tensor in the GPU tests
today and FAILS the new check, with a message that names the place.  Both halves are asserted for every fault.
"""
import numpy as np
import pytest
import torch

import elementwise as E


def rel_l2(a, b):
  return float(np.linalg.norm((a - b).ravel()) / (np.linalg.norm(b.ravel()) + 1e-30))


def bf16(a):
  return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).float().numpy().astype(np.float64)


def randn_bf16(shape, seed):
  g = torch.Generator().manual_seed(seed)
  return torch.randn(shape, generator=g).to(torch.bfloat16)


# ------------------------------------------------------------------------------------------------ the bench conv
@pytest.fixture(scope='module')
def conv_case():
  """k3:c32>16 at 256 x 256, n = 64: float64 reference, its magnitude term, the bound, and the clean bf16 output."""
  n, hw, cin, cout = 64, 256, 32, 16
  x = randn_bf16((n, hw, hw, cin), 1)
  w = (torch.randn(3, 3, cin, cout, generator=torch.Generator().manual_seed(3)) / (9 * cin) ** 0.5).to(torch.bfloat16)
  ref = np.empty((n, hw, hw, cout))
  mag = np.empty((n, hw, hw, cout))
  for i in range(0, n, 8):
    xd = x[i:i + 8].double()
    ref[i:i + 8] = E.conv_taps(xd, w.double(), 'SAME').numpy()
    mag[i:i + 8] = E.conv_taps(xd.abs(), w.double().abs(), 'SAME').numpy()
  bound = E.conv_bound(ref, mag, 9 * cin, torch.bfloat16)
  del mag
  # the kernel's side of it: fp32 accumulation (here: the float64 sum rounded to fp32), then one rounding to bf16
  clean = bf16(ref.astype(np.float32))
  return dict(n=n, hw=hw, cout=cout, ref=ref, bound=bound, clean=clean)


def conv_guard_today(got, direct, ref, n):
  """tests/test_gpu_bench_shapes.py as it stands: rel-L2 < 2e-3 over the whole batch against the direct kernel's output
  (`direct`: the clean rounded reference stands for it) and < 4e-3 against the oracle on images {0, n-1}."""
  sel = [0, n - 1]
  return rel_l2(got, direct) < 2e-3 and rel_l2(got[sel], ref[sel]) < 4e-3


def test_clean_bf16_conv_output_passes_with_ratio_at_most_one(conv_case):
  c = conv_case
  worst = E.assert_elementwise(c['clean'], c['ref'], c['bound'], 'clean k3:c32>16')
  print('clean conv worst ratio %.3f' % worst)
  assert 0.5 < worst <= 1.0      # rounding-dominated: the bound is tight, not merely sufficient
  assert conv_guard_today(c['clean'], c['clean'], c['ref'], c['n'])


def _plant_zero_pixel(a):
  a[37, 129, 200, :] = 0.0
  return dict(n=(37, 37), h=(129, 129), w=(200, 200))


def _plant_tile_edge_row(a):
  a[21, 32, 32:36, :] = a[21, 31, 32:36, :]      # the first pixels of a 32-pixel tile read the row above
  return dict(n=(21, 21), h=(32, 32), w=(32, 35))


def _plant_last_channel_group(a):
  a[5, 77, :, 8:] *= 1.25                        # the last 8 channels of one row of one image
  return dict(n=(5, 5), h=(77, 77), c=(8, 15))


def _plant_nan(a):
  a[40, 3, 3, 3] = np.nan
  return dict(n=(40, 40), h=(3, 3), w=(3, 3), c=(3, 3))


@pytest.mark.parametrize('plant', [_plant_zero_pixel, _plant_tile_edge_row, _plant_last_channel_group],
                         ids=['one_pixel_zeroed', 'tile_edge_row_from_above', 'last_channel_group_scaled'])
def test_planted_conv_fault_passes_rel_l2_and_fails_element_wise(conv_case, plant):
  c = conv_case
  got = c['clean'].copy()
  box = plant(got)
  e_all = rel_l2(got, c['clean'])
  print('%s: whole-batch rel-L2 %.2e against the clean output (that one against the oracle: %.2e)'
        % (plant.__name__, e_all, rel_l2(c['clean'], c['ref'])))
  assert conv_guard_today(got, c['clean'], c['ref'], c['n']), e_all                      # half one: today's thresholds let it through
  worst, msg = E.check_elementwise(got, c['ref'], c['bound'], plant.__name__)
  assert msg is not None and worst > 10.0, (worst, msg)                       # half two: the element-wise check does not
  for axis, (lo, hi) in box.items():                                          # ... and says where
    assert '%s %d..%d' % (axis, lo, hi) in msg, (axis, lo, hi, msg)
  with pytest.raises(AssertionError):
    E.assert_elementwise(got, c['ref'], c['bound'], plant.__name__)


def test_non_finite_output_is_always_a_violation(conv_case):
  c = conv_case
  got = c['clean'].copy()
  box = _plant_nan(got)
  worst, msg = E.check_elementwise(got, c['ref'], c['bound'], 'nan')
  assert msg is not None and '1 of %d' % got.size in msg
  for axis, (lo, hi) in box.items():
    assert '%s %d..%d' % (axis, lo, hi) in msg


# ------------------------------------------------------------------------------------------------ the bench normaliser
@pytest.fixture(scope='module')
def norm_case():
  """instance norm (two domains) + LeakyReLU + pixel norm + pool at 32 x 128 x 128 x 64 (the encoder's third block)."""
  n, hw, c = 32, 128, 64
  y = (randn_bf16((n, hw, hw, c), 11).float() * 0.7 + 0.3).to(torch.bfloat16)
  g = torch.Generator().manual_seed(12)
  par = [torch.randn(c, generator=g) * s + o for s, o in ((0.2, 1.0), (0.2, 0.0)) * 2]
  gz, gzp = randn_bf16((n, hw, hw, c), 13), randn_bf16((n, hw // 2, hw // 2, c), 14)
  out = {}
  for dt in (torch.float64, torch.float32):
    r = E.norm_act_reference(y.to(dt), par[0], par[1], gz, par[2], par[3], split=n // 2, pool=True, gzp=gzp)
    out[dt] = {k: (v.numpy() if k != 'grads' else [t.numpy() for t in v]) for k, v in r.items() if v is not None}
  r64, r32 = out[torch.float64], out[torch.float32]
  return dict(n=n, hw=hw, c=c, y=y.double().numpy(), r=r64,
              e32={k: E.e32(r32[k], r64[k]) for k in ('z', 'zp', 'gy')})


def norm_guard_today(got, ref, n, tol):
  """test_norm_act_at_bench_shapes: rel-L2 per image on images (0, split-1, split, n-1) only."""
  return all(rel_l2(got[i], ref[i]) < tol for i in (0, n // 2 - 1, n // 2, n - 1))


def test_clean_bf16_normaliser_outputs_pass(norm_case):
  c = norm_case
  for k, tol in (('z', 6e-3), ('zp', 6e-3), ('gy', 1.5e-2)):
    ref = c['r'][k]
    worst = E.assert_elementwise(bf16(ref), ref, E.e32_bound(ref, c['e32'][k], torch.bfloat16), 'clean ' + k)
    print('clean normaliser %s worst ratio %.3f (E32 %.2e)' % (k, worst, c['e32'][k]))
    assert worst <= 1.0 and norm_guard_today(bf16(ref), ref, c['n'], tol)


def test_tail_chunk_left_unnormalised_passes_rel_l2_and_fails_element_wise(norm_case):
  """The last pixels of ONE middle image (a tail chunk the second pass never reached) keep the kernel's input.  Today's
  check looks at four images of 32; over the whole tensor the fault is 2.0e-3 in rel-L2, under 6e-3 too."""
  c = norm_case
  ref = c['r']['z']
  got = bf16(ref)
  flat, yflat = got.reshape(c['n'], -1, c['c']), c['y'].reshape(c['n'], -1, c['c'])
  flat[9, -3:, :] = yflat[9, -3:, :]
  e_all = rel_l2(got, ref)
  print('tail chunk: whole-tensor rel-L2 %.2e' % e_all)
  assert e_all < 6e-3 and norm_guard_today(got, ref, c['n'], 6e-3)
  worst, msg = E.check_elementwise(got, ref, E.e32_bound(ref, c['e32']['z'], torch.bfloat16), 'z tail chunk')
  assert msg is not None and worst > 10.0, (worst, msg)
  assert 'n 9..9' in msg and 'h 127..127' in msg and 'w 125..127' in msg, msg


def test_pooled_block_from_its_neighbour_passes_rel_l2_and_fails_element_wise(norm_case):
  c = norm_case
  ref = c['r']['zp']
  got = bf16(ref)
  got[20, 31, 16, :] = got[20, 31, 15, :]      # one 2x2 block's mean taken from the block to its left
  e_all = rel_l2(got, ref)
  print('pooled block: whole-tensor rel-L2 %.2e' % e_all)
  assert e_all < 6e-3 and norm_guard_today(got, ref, c['n'], 6e-3)
  worst, msg = E.check_elementwise(got, ref, E.e32_bound(ref, c['e32']['zp'], torch.bfloat16), 'zp block')
  assert msg is not None and worst > 10.0, (worst, msg)
  assert 'n 20..20' in msg and 'h 31..31' in msg and 'w 16..16' in msg, msg


def test_one_image_gradient_row_wrong_passes_rel_l2_and_fails_element_wise(norm_case):
  """Eight pixels of one row of gy of a middle image carry the row above's values (a halo row read at a chunk edge)."""
  c = norm_case
  ref = c['r']['gy']
  got = bf16(ref)
  got[13, 64, 32:40, :] = got[13, 63, 32:40, :]
  assert rel_l2(got, ref) < 1.5e-2 and norm_guard_today(got, ref, c['n'], 1.5e-2)
  worst, msg = E.check_elementwise(got, ref, E.e32_bound(ref, c['e32']['gy'], torch.bfloat16), 'gy row')
  assert msg is not None and worst > 10.0 and 'n 13..13' in msg and 'h 64..64' in msg and 'w 32..39' in msg, (worst, msg)


# ------------------------------------------------------------------------------------------------ a 256-channel reduction
def test_one_channel_of_a_parameter_gradient_off_by_40_percent():
  """test_norm_act's (3, 4, 4, 256) case guards the gamma gradient with tol_for(bf16, grad) = 3e-2: one channel of 256 off by
  40 % is 0.4 / 16 = 2.5e-2 of the norm.  The element-wise bound of an fp32 reduction is 2^-24 |ref| + 16 E32."""
  n, h, w, c = 3, 4, 4, 256
  rng = np.random.RandomState(6)
  y = torch.from_numpy(bf16(rng.randn(n, h, w, c) * 1.5 + 0.7))
  gamma, beta = torch.from_numpy(1.0 + 0.2 * rng.randn(c)), torch.from_numpy(0.1 * rng.randn(c))
  gz = torch.from_numpy(bf16(rng.randn(n, h, w, c)))
  r64 = E.norm_act_reference(y, gamma, beta, gz)
  r32 = E.norm_act_reference(y.float(), gamma, beta, gz)
  ref = r64['grads'][0].numpy()
  bound = E.e32_bound(ref, E.e32(r32['grads'][0].numpy(), ref), torch.float32)
  clean = ref.astype(np.float32).astype(np.float64)
  assert E.assert_elementwise(clean, ref, bound, 'clean gamma gradient') <= 1.0
  rms = np.sqrt(np.mean(ref ** 2))
  ch = int(np.argmin(np.abs(np.abs(ref) - rms)))       # a channel of typical size: |g_c| = rms -> 0.4 / sqrt(256) of the norm
  got = clean.copy()
  got[ch] *= 1.4
  e = rel_l2(got, ref)
  print('gamma gradient, channel %d x 1.4: rel-L2 %.3e' % (ch, e))
  assert e < 3e-2                                                     # tol_for(torch.bfloat16, grad=True)
  worst, msg = E.check_elementwise(got, ref, bound, 'gamma gradient')
  assert msg is not None and worst > 100.0 and 'd0 %d..%d' % (ch, ch) in msg, (worst, msg)


# ------------------------------------------------------------------------------------------------ the LeakyReLU alternate
def _lrelu_case():
  rng = np.random.RandomState(5)
  pre = rng.randn(4, 8, 8, 16)
  pre[1, 2, 3, 4] = 1e-9                       # a pre-activation inside its own bound
  pre[2, 5, 5, 5] = 0.3                        # one that is not
  g = rng.randn(*pre.shape)
  ref = g * np.where(pre > 0, 1.0, 0.2)
  alt = g * np.where(pre > 0, 0.2, 1.0)
  pre_bound = 2.0 ** -24 * np.abs(pre) + 1e-7
  return pre, ref, alt, np.abs(pre) < pre_bound, E.rounded_bound(ref, torch.float32)


def test_lrelu_alternate_is_accepted_only_where_the_pre_activation_is_inside_its_bound():
  pre, ref, alt, where, bound = _lrelu_case()
  assert where.sum() == 1
  got = ref.copy()
  got[1, 2, 3, 4] = alt[1, 2, 3, 4]            # the computed sign fell on the other side of zero: accepted ...
  assert E.check_elementwise(got, ref, bound, 'x')[1] is not None
  E.assert_elementwise(got, ref, bound, 'near zero', alt_ref=alt, alt_where=where, alt_cap=1e-3)
  got[2, 5, 5, 5] = alt[2, 5, 5, 5]            # ... a wrong slope at |pre| = 0.3 is not
  worst, msg = E.check_elementwise(got, ref, bound, 'far from zero', alt_ref=alt, alt_where=where, alt_cap=1e-3)
  assert msg is not None and '(2, 5, 5, 5)' in msg, msg


def test_lrelu_alternate_is_refused_beyond_its_cap():
  pre, ref, alt, where, bound = _lrelu_case()
  got = ref.copy()
  got[1, 2, 3, 4] = alt[1, 2, 3, 4]
  # one element of 4096 is 2.4e-4 of the tensor: over the default cap of 1e-5
  worst, msg = E.check_elementwise(got, ref, bound, 'cap', alt_ref=alt, alt_where=where)
  assert msg is not None and 'cap' in msg and 'other LeakyReLU slope' in msg, msg
  with pytest.raises(AssertionError):
    E.assert_elementwise(got, ref, bound, 'cap', alt_ref=alt, alt_where=where)


def test_bounds_are_the_documented_formulas():
  assert E.unit_roundoff(torch.bfloat16) == 2.0 ** -8 and E.unit_roundoff(torch.float16) == 2.0 ** -11
  assert E.unit_roundoff(torch.float32) == 2.0 ** -24
  ref, mag = np.array([2.0, -4.0]), np.array([8.0, 16.0])
  u = 2.0 ** -8
  assert np.array_equal(E.conv_bound(ref, mag, 288, torch.bfloat16), u * np.abs(ref) + (1 + u) * 288 * 2.0 ** -24 * mag + 2.0 ** -126)
  assert np.array_equal(E.wgrad_bound(ref, mag, 1000), 2.0 ** -24 * np.abs(ref) + 1000 * 2.0 ** -24 * mag + 2.0 ** -126)
  assert E.tiny(torch.float16) == 2.0 ** -25 and E.tiny(torch.bfloat16) == E.tiny(torch.float32) == 2.0 ** -126
  assert np.array_equal(E.pair_bound(ref, -ref * 2, mag, 288, torch.float16),
                        2 * (2.0 ** -11 * np.abs(ref) * 2 + 2.0 ** -25) + 2 * 288 * 2.0 ** -24 * mag)
  assert np.array_equal(E.e32_bound(ref, 1e-6, torch.bfloat16), u * np.abs(ref) + 16 * 1e-6 + 2.0 ** -126)
  # every representable bf16 / fp16 rounding of a value sits inside u |x|
  x = np.random.RandomState(0).randn(100000) * np.exp(np.random.RandomState(1).randn(100000) * 3)
  assert np.all(np.abs(bf16(x) - x) <= u * np.abs(x))
  h = torch.from_numpy(x).to(torch.float16).double().numpy()
  ok = (np.abs(x) > 2.0 ** -14) & (np.abs(x) < 6e4)      # fp16 normal range
  assert np.all(np.abs(h - x)[ok] <= 2.0 ** -11 * np.abs(x)[ok])
  # ... and below its normal range fp16 rounds to multiples of 2^-24: the bound's tiny(float16) = 2^-25 covers that
  sub = np.abs(x) <= 2.0 ** -14
  assert sub.sum() > 100 and np.all(np.abs(h - x)[sub] <= 2.0 ** -25) and np.any(np.abs(h - x)[sub] > 2.0 ** -11 * np.abs(x)[sub])


# ------------------------------------------------------------------------------------------------ minibatch stddev at n = 2
@pytest.mark.parametrize('coincide', [False, True])
@pytest.mark.parametrize('n,groups,c', [(2, 1, 8), (16, 1, 256)])
def test_mbstd_conditioning_term_keeps_the_fp32_check_alive(n, groups, c, coincide):
  """The derived term the fp32 minibatch-stddev check adds to u |ref| + 16 E32 (elementwise.mbstd_conditioning; eps under the
  root, as in the formula) is small next to that bound -- also at n = 2 with a position whose two samples coincide EXACTLY,
  where a root without eps would divide by zero -- and planted faults in the second-order outputs still fail:
  one element of gx2 taken from its neighbour sample, the statistic channel of ggo off by 1 %.  (With the coincidence
  planted, fp32 really does lose the statistic channel's digits there -- rounding noise of x - mean over sigma = 1e-4 -- so the
  ggo half is asserted on the natural inputs.)"""
  rng = np.random.RandomState(400 + n + c)
  f32 = lambda a: torch.from_numpy(a.astype(np.float32)).double()
  x, v, go = f32(rng.randn(n, 4, 4, c)), f32(rng.randn(n, 4, 4, c)), f32(rng.randn(n, 4, 4, c + 1))
  if coincide:
    x[:, 1, 2, 3] = x[0, 1, 2, 3]                # one position where every sample coincides: sigma^2 = eps there
  eps = 1e-8
  r64 = E.mbstd_reference(x, go, v, groups, eps, torch.float64)
  r32 = E.mbstd_reference(x, go, v, groups, eps, torch.float32)
  ex_gx, ex_T, ex_gx2 = E.mbstd_conditioning(x, go, v, groups, eps)
  assert np.all(np.isfinite(ex_gx)) and np.all(np.isfinite(ex_T)) and np.all(np.isfinite(ex_gx2))
  base = {i: E.e32_bound(r64[i], E.e32(r32[i], r64[i]), torch.float32) for i in (1, 2, 3)}
  away = np.ones(x.shape, bool)
  away[:, 1, 2, 3] = False                       # everywhere but the degenerate position the term is a correction, not the bound
  assert np.median(ex_gx / base[1]) < 0.1 and np.median(ex_gx2[away] / base[3][away]) < 1.0
  # the statistic channel's term is a worst-case sum over every element (its errors do not cancel in a bound): 1e-5 on a
  # value of order 0.1 for unit-scale inputs -- a hundred times the E32 term, a hundred times below a 1 % fault
  assert coincide or ex_T.max() < 1e-4
  # clean fp32 outputs (the float64 values rounded once) pass ...
  ex_ggo = np.zeros_like(r64[2])
  ex_ggo[..., c] = np.repeat(ex_T, n // groups).reshape(n, 1, 1)
  bound = {1: base[1] + ex_gx, 2: base[2] + ex_ggo, 3: base[3] + ex_gx2}
  for i in ((1, 3) if coincide else (1, 2, 3)):
    assert E.assert_elementwise(r64[i].astype(np.float32).astype(np.float64), r64[i], bound[i], 'clean mbstd output %d' % i) <= 1.0
  # ... a gx2 element that took the other sample's value does not (at the position where gx2 is largest, away from the planted one)
  g2 = r64[3].copy()
  mag = np.where(away, np.abs(g2), 0.0)
  i0 = np.unravel_index(int(np.argmax(mag)), g2.shape)
  j0 = ((i0[0] + 1) % n,) + tuple(i0[1:])
  g2[i0] = r64[3][j0]
  worst, msg = E.check_elementwise(g2, r64[3], bound[3], 'gx2 from the neighbour sample')
  assert msg is not None and worst > 2.0 and str(tuple(int(k) for k in i0)) in msg, (worst, msg)
  if coincide:
    return
  # ... nor does a statistic channel of ggo that is 1 % off
  gg = r64[2].copy()
  gg[..., c] *= 1.01
  worst, msg = E.check_elementwise(gg, r64[2], bound[2], 'ggo statistic off by 1 %')
  assert msg is not None and 'c %d..%d' % (c, c) in msg, (worst, msg)
