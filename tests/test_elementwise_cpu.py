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
from oracle import np_ops as N      # noqa: E402  (checker only)


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


# ------------------------------------------------------------------------------------------------ flash attention forward
def f16(a):
  return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.float16).float().numpy().astype(np.float64)


def _r16(a, dtype):
  """float64 -> the 16-bit type, round to nearest even, straight from float64."""
  return torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(dtype).double().numpy()


def flash_fwd_model(q, k, v, dtype, skip_rescale=None, drop_block=None, v_from_image=None):
  """csrc/flash.hip's forward in numpy: float64 where the kernel is fp32, its 16-bit pack of P, its stale running maximum
  (raised only when a 32-key block beats it by more than 6, decided per query, taken per 32-query wave), its row sum of the
  PACKED probabilities -- the clean output the planted faults are edits of:
      skip_rescale = (image, query, block)          that query's accumulators are not multiplied by corr at that block
      drop_block = (image, query, feature block, key block)    32 features of one row leave one 32-key block out
      v_from_image = (image, source)                image `image` reads the V of image `source`
  -> (O rounded to dtype, lse)."""
  n, ln, dv = v.shape
  out, lse = np.empty((n, ln, dv)), np.empty((n, ln))
  for im in range(n):
    s = q[im] @ k[im].T
    vi = v[v_from_image[1]] if v_from_image is not None and v_from_image[0] == im else v[im]
    m = np.full(ln, -np.inf)
    acc, l = np.zeros((ln, dv)), np.zeros(ln)
    for kb in range(ln // 32):
      sb = s[:, 32 * kb:32 * kb + 32]
      mx = sb.max(1)
      rs = mx > m + E.K_STALE
      wave = np.repeat(rs.reshape(-1, 32).any(1), 32)
      m_new = np.where(rs, mx, m)
      with np.errstate(invalid='ignore'):
        corr = np.where(np.isinf(m), 0.0, np.exp(m - m_new))
      corr = np.where(wave, corr, 1.0)
      if skip_rescale is not None and skip_rescale[0] == im and skip_rescale[2] == kb:
        corr[skip_rescale[1]] = 1.0
      acc *= corr[:, None]
      l *= corr
      m = np.where(wave, m_new, m)
      pk = _r16(np.exp(sb - m[:, None]), dtype)
      l += pk.sum(1)
      add = pk @ vi[32 * kb:32 * kb + 32]
      if drop_block is not None and drop_block[0] == im and drop_block[3] == kb:
        add[drop_block[1], 32 * drop_block[2]:32 * drop_block[2] + 32] = 0.0
      acc += add
    out[im] = _r16(acc / l[:, None], dtype)
    lse[im] = m + np.log(l)
  return out, lse


FLASH_TODAY = {'fwd': [(2, 256, 8, 64), (1, 1024, 16, 128), (3, 128, 8, 256)]}      # tests/test_gpu_ops.py's forward cases


def flash_guard_today(o, lse, t, dtype):
  """test_flash_attention_forward's assertions: rel-L2 of O, max |lse - want|."""
  bf = dtype == torch.bfloat16
  return rel_l2(o, t['o']) < (6e-3 if bf else 8e-4), float(np.abs(lse - t['lse']).max()) < (2e-3 if bf else 3e-4)


def _flash_case(family, n, ln, dk, dv, dtype, seed=7):
  rng = np.random.RandomState(seed)
  rnd = lambda a: _r16(a, dtype)
  q, k = E.attention_family(family, n, ln, dk, rng, rnd)
  v = rnd(rng.randn(n, ln, dv))
  t = E.attention_terms(q, k, v)
  return q, k, v, t, E.attention_fwd_bound(t, dk, dtype), E.attention_lse_bound(t, dk, dtype)


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'f16'])
@pytest.mark.parametrize('family', E.ATTENTION_FAMILIES)
def test_flash_forward_model_is_inside_the_derived_bound(family, dtype):
  """The numpy model of the forward kernel (its pack, its stale maximum, its rescales) on every score family: every element of
  O and lse inside the bound derived in elementwise.attention_fwd_bound / attention_lse_bound, and not by orders of
  magnitude -- the bound is of the size of the pack's rounding, which the model performs (late_spike: every row attends to
  one key with p = 1 exactly, O is that key's V, no rounding happens)."""
  q, k, v, t, bo, bl = _flash_case(family, 2, 256, 8, 64, dtype)
  o, lse = flash_fwd_model(q, k, v, dtype)
  wo = E.assert_elementwise(o, t['o'], bo, 'model O %s' % family)
  wl = E.assert_elementwise(lse, t['lse'], bl, 'model lse %s' % family)
  print('flash model %-10s %s: worst ratio O %.3f lse %.3f' % (family, dtype, wo, wl))
  assert wo <= 1.0 and wl <= 1.0 and (wo > 0.05 or family == 'late_spike')


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'f16'])
def test_planted_flash_fault_one_key_block_missing_from_one_feature_block(dtype):
  """One (query row, 32-feature block) of O accumulated without one 32-key block (a lost MFMA step), at today's (1, 1024, 16,
  128): 32 elements of 131072 move by a few per cent of their magnitude -- inside today's rel-L2, outside the element bound,
  and the message names the row and the feature block."""
  q, k, v, t, bo, bl = _flash_case('benign', 1, 1024, 16, 128, dtype)
  # the (row, key block) whose share of the row's probability is nearest 5 % (bf16) / 1 % (fp16): about ten times the pack's
  # rounding, well under what rel-L2 over the tensor notices
  mass = t['p'][0].reshape(1024, 32, 32).sum(-1)
  row, kb = np.unravel_index(int(np.argmin(np.abs(mass - (0.05 if dtype == torch.bfloat16 else 0.01)))), mass.shape)
  o, lse = flash_fwd_model(q, k, v, dtype, drop_block=(0, int(row), 1, int(kb)))
  assert flash_guard_today(o, lse, t, dtype) == (True, True)
  worst, msg = E.check_elementwise(o, t['o'], bo, 'key block dropped')
  assert msg is not None and worst > 3.0 and 'd0 0..0' in msg and 'd1 %d..%d' % (row, row) in msg, (worst, msg)
  lo = [int(x) for x in msg.split('d2 ')[1].split(';')[0].split('..')]
  assert 32 <= lo[0] and lo[1] <= 63, msg


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'f16'])
def test_planted_flash_fault_one_row_lse_off_by_4u(dtype):
  """One row's lse off by 4 u.  Today's guard on lse is an absolute 2e-3 (bf16) / 3e-4 (fp16) = u / 2 and u / 1.6: it does
  catch 4 u on the benign family -- and it rejects the CLEAN model on the families it was never run on (one dominant,
  rounded probability moves lse by up to u), so it cannot be carried over to them.  The derived bound accepts the clean
  model everywhere (the test above) and rejects 4 u on every family."""
  u = E.unit_roundoff(dtype)
  rejected_clean = 0
  for family in E.ATTENTION_FAMILIES:
    q, k, v, t, bo, bl = _flash_case(family, 1, 256, 8, 64, dtype)
    o, lse = flash_fwd_model(q, k, v, dtype)
    rejected_clean += not flash_guard_today(o, lse, t, dtype)[1]
    lse[0, 130] += 4 * u
    worst, msg = E.check_elementwise(lse, t['lse'], bl, 'lse + 4u')
    assert msg is not None and worst > 1.5 and 'd1 130..130' in msg, (family, worst, msg)
  assert rejected_clean >= 1


def test_planted_flash_fault_one_rescale_skipped():
  """One query of a ramp keeps its accumulators unscaled at ONE rescale, the one before the last.  Scores: q0 = 4 against a
  staircase k0 rising by 6.5 / 4 per 32-key block (every block beats the stale maximum by just over kStaleMax), the other key
  features zero; V = +1, +1, -1, -1 by block plus noise, so that what the blocks before the skipped rescale hold differs from
  the row's value.  They then weigh e^6.5 times too much: e^-6.5 = 1.5e-3 of the row -- the largest effect a skipped rescale can
  have short of the last one (a rescale happens only above kStaleMax = 6, so what it scales is at most e^-6 of the row once
  another follows).  That is under one bf16 u -- no element check can see it there, nor is it an error worth seeing -- so this
  fault is planted in fp16: 64 elements of one row, inside today's rel-L2 (8e-4), outside the element bound."""
  dtype = torch.float16
  n, ln, dk, dv = 3, 256, 16, 64
  rng = np.random.RandomState(21)
  rnd = lambda a: _r16(a, dtype)
  q, k = E.attention_family('benign', n, ln, dk, rng, rnd)
  q[:, :, 0] = 4.0
  k[:] = 0.0
  k[:, :, 0] = rnd(6.5 / 4.0 * (np.arange(ln) // 32))      # a staircase: one step per block
  v = rnd(np.where((np.arange(ln) // 32) % 4 < 2, 1.0, -1.0)[None, :, None] + 0.1 * rng.randn(n, ln, dv))
  t = E.attention_terms(q, k, v)
  bo, bl = E.attention_fwd_bound(t, dk, dtype), E.attention_lse_bound(t, dk, dtype)
  o, lse = flash_fwd_model(q, k, v, dtype)
  assert E.assert_elementwise(o, t['o'], bo, 'clean staircase') <= 1.0
  of, lf = flash_fwd_model(q, k, v, dtype, skip_rescale=(2, 41, ln // 32 - 2))
  assert flash_guard_today(of, lf, t, dtype)[0]
  worst, msg = E.check_elementwise(of, t['o'], bo, 'rescale skipped')
  assert msg is not None and worst > 1.5 and 'd0 2..2' in msg and 'd1 41..41' in msg, (worst, msg)
  # lse sees it too: l is too large by the same e^-6.5 of itself
  worst, msg = E.check_elementwise(lf, t['lse'], bl, 'rescale skipped, lse')
  assert msg is not None and 'd1 41..41' in msg, (worst, msg)


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'f16'])
def test_planted_flash_fault_image_one_of_three_reads_image_zeros_v(dtype):
  """Image 1 of 3 computed from image 0's V (the img * d_v * len offset of the packed V workspace), at (3, 256, 16, 64).
  Today's forward test has no case of this template instance (d_qk 16 with d_v 64) and none with three images of two loop
  trips: the guard the suite has today is never asked.  Where it IS asked -- the same fault at its own (3, 128, 8, 256) --
  it fails, as it should: the gap is the shape list, not the measure.  The element check fails on image 1 only, and so does
  the comparison of image 1 with the same image run alone (bit for bit on the clean model)."""
  shape = (3, 256, 16, 64)
  assert shape not in FLASH_TODAY['fwd'] and not any(s[2:] == shape[2:] for s in FLASH_TODAY['fwd'])
  q, k, v, t, bo, bl = _flash_case('benign', *shape, dtype=dtype)
  o, lse = flash_fwd_model(q, k, v, dtype, v_from_image=(1, 0))
  worst, msg = E.check_elementwise(o, t['o'], bo, 'image 1 from V[0]')
  assert msg is not None and worst > 100.0 and 'd0 1..1' in msg, (worst, msg)
  clean, _ = flash_fwd_model(q, k, v, dtype)
  alone, _ = flash_fwd_model(q[1:2], k[1:2], v[1:2], dtype)
  assert np.array_equal(clean[1], alone[0]) and not np.array_equal(o[1], alone[0])
  q, k, v, t, bo, bl = _flash_case('benign', 3, 128, 8, 256, dtype=dtype)
  o, lse = flash_fwd_model(q, k, v, dtype, v_from_image=(1, 0))
  assert not flash_guard_today(o, lse, t, dtype)[0]


# ------------------------------------------------------------------------------------------------ flash attention backwards
def flash_bwd_maps(q, k, v, go, dtype):
  """What csrc/flash.hip's two backward passes hold per (query, key) before their second products, in numpy: the probability
  recomputed from the forward model's lse, D = <dO, O> from the forward model's STORED O, and the 16-bit packs of P and dS --
  the clean maps the planted faults below are edits of -> dict(p16, ds16, ph, D, gp)."""
  o16, lse = flash_fwd_model(q, k, v, dtype)
  ph = np.exp(np.einsum('nid,njd->nij', q, k) - lse[..., None])
  gp = np.einsum('nid,njd->nij', go, v)
  D = (go * o16).sum(-1, keepdims=True)
  return dict(p16=_r16(ph, dtype), ds16=_r16(ph * (gp - D), dtype), ph=ph, D=D, gp=gp)


def _dropped_block(m, x, ref, bound, tol=None):
  """Among every (image, row, block of 32) of the sum over the last index of m against x: the block whose loss moves its row
  furthest outside `bound` -- with `tol`, among those that keep the whole tensor's rel-L2 under half of it (the loss LEAST
  visible to rel-L2 for what it does to its row; searched, not tuned) -> (image, row, block, delta [d], ratio)."""
  n, ln, _ = m.shape
  delta = np.einsum('nibj,nbjd->nibd', m.reshape(n, ln, ln // 32, 32), x.reshape(n, ln // 32, 32, -1))      # [n, i, block, d]
  ratio = (np.abs(delta) / bound[:, :, None, :]).max(-1)
  if tol is not None:
    ratio = np.where(np.sqrt((delta ** 2).sum(-1)) / np.linalg.norm(ref) < 0.5 * tol, ratio, 0.0)
  im, row, kb = (int(i) for i in np.unravel_index(int(np.argmax(ratio)), ratio.shape))
  return im, row, kb, delta[im, row, kb], float(ratio[im, row, kb])


def _flash_bwd_case(family, dtype):
  n, ln, dk, dv = 1, 512, 16, 128      # a case of today's test_flash_attention_backward
  rng = np.random.RandomState(11)
  rnd = lambda a: _r16(a, dtype)
  q, k = E.attention_family(family, n, ln, dk, rng, rnd)
  v, go = rnd(rng.randn(n, ln, dv)), rnd(rng.randn(n, ln, dv))
  t = E.attention_terms(q, k, v)
  r = E.attention_grads_reference(q, k, v, go, t)
  bounds = E.attention_bwd_bounds(q, k, v, go, t, r, dk, dtype)
  mp = flash_bwd_maps(q, k, v, go, dtype)
  raw = (np.einsum('nij,njd->nid', mp['ds16'], k), np.einsum('nij,nid->njd', mp['ds16'], q), np.einsum('nij,nid->njd', mp['p16'], go))
  return q, k, go, r, bounds, mp, raw, rnd


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'f16'])
def test_planted_flash_faults_in_the_first_order_backward(dtype):
  """The numpy model of the packed P and dS at today's (1, 512, 16, 128): dQ, dK and dV inside attention_bwd_bounds.
  (a) dV: one key's row summed without one block of 32 queries (a lost MFMA step of flash_bwd_kv_kernel) passes today's guard
      -- rel-L2 of every gradient under 1.2e-2 (bf16) / 2e-3 (fp16) -- and is far outside the element bound, which names the row.
  (b) dQ: the same fault in flash_bwd_q_kernel.  Here the bound is NOT the sharper measure on benign rows: D = <dO, O> from the
      16-bit O (d_v worst-case roundings, about 17 u of dS at d_v = 128) and the pack on |dO| |V|^T make it about 50 u of
      the row, and the worst dropped block that rel-L2 still passes reaches a ratio of 0.36 (bf16) / 0.49 (fp16), printed
      below.  What the bound adds for dQ and dK is the families rel-L2 cannot be asked on: on ramp_up the CLEAN model has a
      rel-L2 of 1.8e-2 / 2.4e-3 -- today's guard rejects an honest kernel (cancellation along the ramp) -- while every element
      is inside the bound, and a row that lost one key block is outside it."""
  tol = 1.2e-2 if dtype == torch.bfloat16 else 2e-3
  names = ('dq', 'dk', 'dv')
  q, k, go, r, bounds, mp, raw, rnd = _flash_bwd_case('benign', dtype)
  worst = [E.assert_elementwise(rnd(g), r[nm], b, 'model ' + nm) for g, nm, b in zip(raw, names, bounds)]
  print('flash bwd model %s: worst ratios dq %.3f dk %.3f dv %.3f' % ((dtype,) + tuple(worst)))
  assert max(worst) <= 1.0
  im, row, qb, delta, _ = _dropped_block(mp['p16'].transpose(0, 2, 1), go, r['dv'], bounds[2], tol)
  bad = raw[2].copy()
  bad[im, row] -= delta
  assert all(rel_l2(rnd(g), r[nm]) < tol for g, nm in zip(raw[:2] + (bad,), names))      # today's guard
  w, msg = E.check_elementwise(rnd(bad), r['dv'], bounds[2], 'query block missing from dV')
  print('flash bwd fault %s: dV key %d query block %d, rel-L2 %.2e, worst ratio %.2f' % (dtype, row, qb, rel_l2(rnd(bad), r['dv']), w))
  assert msg is not None and w > 5.0 and 'd1 %d..%d' % (row, row) in msg, (w, msg)
  print('flash bwd %s: the worst key block a row of dQ can lose under today\'s rel-L2: ratio %.2f'
        % (dtype, _dropped_block(mp['ds16'], k, r['dq'], bounds[0], tol)[4]))
  q, k, go, r, bounds, mp, raw, rnd = _flash_bwd_case('ramp_up', dtype)
  assert E.assert_elementwise(rnd(raw[0]), r['dq'], bounds[0], 'model dq, ramp_up') <= 1.0
  assert rel_l2(rnd(raw[0]), r['dq']) > tol      # today's guard rejects the clean model: it cannot be asked here
  im, row, kb, delta, _ = _dropped_block(mp['ds16'], k, r['dq'], bounds[0])
  bad = raw[0].copy()
  bad[im, row] -= delta
  w, msg = E.check_elementwise(rnd(bad), r['dq'], bounds[0], 'key block missing from dQ, ramp_up')
  print('flash bwd fault %s: ramp_up dQ row %d key block %d, worst ratio %.2f' % (dtype, row, kb, w))
  assert msg is not None and w > 2.0 and 'd1 %d..%d' % (row, row) in msg, (w, msg)


def flash_bb_model(q, k, v, go, aq, ak, av, dtype, e_from_image=None):
  """csrc/flash.hip's second-order pass in numpy: the statistics D (from the stored O), E and F in float64, the four maps P,
  gS, T, U packed to 16 bit, then the closed form's products (oracle/np_ops.attention_backward_backward).  e_from_image =
  (image, source): image `image` reads the E statistic of image `source` (a wrong per-image offset of the statistics
  workspace).  -> the unrounded (adj q, adj k, adj v, adj dO) and the packed maps."""
  mp = flash_bwd_maps(q, k, v, go, dtype)
  p, D, gp = mp['ph'], mp['D'], mp['gp']
  w = np.einsum('nid,njd->nij', aq, k) + np.einsum('nid,njd->nij', q, ak)
  e = (p * w).sum(-1, keepdims=True)
  if e_from_image is not None:
    e = e.copy()
    e[e_from_image[0]] = e[e_from_image[1]]
  x = np.einsum('nid,njd->nij', go, av) + w * (gp - D) - e * gp
  f = (p * x).sum(-1, keepdims=True)
  m = dict(pv=mp['p16'], gs=mp['ds16'], tv=_r16(p * (w - e), dtype), uv=_r16(p * (x - f), dtype))
  kj = lambda a, b: np.einsum('nij,njd->nid', a, b)
  qi = lambda a, b: np.einsum('nij,nid->njd', a, b)
  return [kj(m['gs'], ak) + kj(m['uv'], k), qi(m['gs'], aq) + qi(m['uv'], q), qi(m['tv'], go), kj(m['pv'], av) + kj(m['tv'], v)], m


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'f16'])
def test_planted_flash_faults_in_the_second_order_pass(dtype):
  """Second order at today's (2, 256, 8, 64): the numpy model of the four packed maps gives the four adjoints inside
  attention_bwd_bwd_bounds.  (a) One query row of adj dO = P aV + T V whose T V sum misses one 32-key block passes today's
  guard (rel-L2 under 2.5e-2 bf16 / 4e-3 fp16 on all four) and is outside the element bound, which names the row.  (b) Image
  1 reading image 0's E statistic is outside the bound on image 1 alone, in adj v and adj dO (the maps E enters); rel-L2 sees
  that one too at this shape -- it is here to show the bound rejects it, and the device test's image-alone comparison is
  what pins the offsets at every shape."""
  n, ln, dk, dv = 2, 256, 8, 64
  rng = np.random.RandomState(13)
  rnd = lambda a: _r16(a, dtype)
  q, k = E.attention_family('benign', n, ln, dk, rng, rnd)
  v, go, av = (rnd(rng.randn(n, ln, dv)) for _ in range(3))
  aq, ak = rnd(rng.randn(n, ln, dk)), rnd(rng.randn(n, ln, dk))
  t = E.attention_terms(q, k, v)
  r = E.attention_grads_reference(q, k, v, go, t)
  r['bb'] = N.attention_backward_backward(q, k, v, go, aq, ak, av)
  bounds = E.attention_bwd_bwd_bounds(q, k, v, go, aq, ak, av, t, r, dk, dtype)
  raw, m = flash_bb_model(q, k, v, go, aq, ak, av, dtype)
  names = ('adj q', 'adj k', 'adj v', 'adj dO')
  worst = [E.assert_elementwise(rnd(g), ref, b, 'model ' + nm) for g, ref, b, nm in zip(raw, r['bb'], bounds, names)]
  print('flash bwd_bwd model %s: worst ratios %s' % (dtype, ' '.join('%s %.3f' % x for x in zip(names, worst))))
  assert max(worst) <= 1.0
  tol = 2.5e-2 if dtype == torch.bfloat16 else 4e-3
  im, row, kb, delta, _ = _dropped_block(m['tv'], v, r['bb'][3], bounds[3], tol)
  bad = raw[3].copy()
  bad[im, row] -= delta
  assert all(rel_l2(rnd(g), ref) < tol for g, ref in zip(raw[:3] + [bad], r['bb']))      # today's guard
  w, msg = E.check_elementwise(rnd(bad), r['bb'][3], bounds[3], 'key block missing from adj dO')
  print('flash bwd_bwd fault %s: image %d row %d block %d, rel-L2 %.2e, worst ratio %.2f' % (dtype, im, row, kb, rel_l2(bad, r['bb'][3]), w))
  assert msg is not None and w > 2.0 and 'd0 %d..%d' % (im, im) in msg and 'd1 %d..%d' % (row, row) in msg, (w, msg)
  off, _ = flash_bb_model(q, k, v, go, aq, ak, av, dtype, e_from_image=(1, 0))
  for i in (2, 3):
    w, msg = E.check_elementwise(rnd(off[i]), r['bb'][i], bounds[i], names[i] + ', E of image 0 in image 1')
    assert msg is not None and w > 2.0 and 'd0 1..1' in msg, (names[i], w, msg)


# ------------------------------------------------------------------------------------------------ batched GEMM
def test_planted_gemm_fault_one_vector_of_the_last_ragged_tile_keeps_its_old_value():
  """C (+)= 0.5 A B at (2, 1032, 520, 8) in bf16 onto a non-zero C: the last row tile has 8 of its 128 rows, the last column tile
  8 of its 64 columns.  One 8-element vector of that corner keeps the value C held before: 8 of a million elements -- rel-L2
  2.7e-3 < today's 4e-3; outside the element bound."""
  rng = np.random.RandomState(5)
  b_, m, n, k = 2, 1032, 520, 8
  a, b, c0 = bf16(rng.randn(b_, m, k)), bf16(rng.randn(b_, k, n)), bf16(rng.randn(b_, m, n))
  ref = 0.5 * (a @ b) + c0
  bound = E.gemm_bound(ref, 0.5 * (np.abs(a) @ np.abs(b)), k, torch.bfloat16, c0=c0)
  clean = bf16(ref.astype(np.float32))
  assert 0.5 < E.assert_elementwise(clean, ref, bound, 'clean gemm') <= 1.0
  got = clean.copy()
  got[1, 1031, 512:520] = c0[1, 1031, 512:520]
  assert rel_l2(got, ref) < 4e-3
  worst, msg = E.check_elementwise(got, ref, bound, 'stale vector')
  assert msg is not None and worst > 10.0 and 'd0 1..1' in msg and 'd1 1031..1031' in msg and 'd2 512..519' in msg, (worst, msg)


# ------------------------------------------------------------------------------------------------ scalar reductions
def _sum_model(x, V, threads, drop_tail=False):
  """sum_kernel's order in fp32: per thread its vectors (grid stride), then its tail elements, then the tree."""
  x = x.astype(np.float32)
  nvec = x.size // V
  acc = np.zeros(threads, np.float32)
  body = x[:nvec * V].reshape(nvec, V)
  for i0 in range(0, nvec, threads):
    chunk = body[i0:i0 + threads]
    for j in range(V):
      acc[:chunk.shape[0]] += chunk[:, j]
  if not drop_tail:
    tail = x[nvec * V:]
    acc[:tail.size] += tail
  return float(acc.reshape(-1, 2).sum(1, dtype=np.float32).sum(dtype=np.float32))


def test_planted_sum_fault_the_vector_tail_dropped():
  """tg_sum at the sizes the suite has today (384 and 768 elements, 6 x 64 x 64 x 32 in the ordered test) has no vector tail:
  a kernel that drops the tail loop returns the same bits there, whatever the guard.  At 4099 = 512 vectors of 8 + 3, with the
  tail elements (and each workgroup's first and last element) a thousand times the rest, the dropped tail is far outside
  L 2^-24 sum|x| -- and so would ONE dropped or doubled element of them be."""
  rng = np.random.RandomState(9)
  for numel in (384, 768):
    x = bf16(rng.rand(numel))
    assert numel % 8 == 0 and _sum_model(x, 8, 256) == _sum_model(x, 8, 256, drop_tail=True)
  numel = 4099
  x = bf16(rng.rand(numel))
  x[4096:] *= 1e3
  L, blocks = E.reduction_chain(numel, torch.bfloat16, 1024)
  assert blocks == 3 and L == 1 * 8 + 1 + 6 + 4 + 3 + 1
  bound = E.reduction_bound(np.abs(x).sum(), L)
  ref = x.sum()
  assert abs(_sum_model(x, 8, 256 * blocks) - ref) <= bound
  assert abs(_sum_model(x, 8, 256 * blocks, drop_tail=True) - ref) > 100 * bound
  assert np.abs(x[4096:]).min() > 100 * bound      # one spiked element alone is visible
  # the geometry: a 16 x 256 x 256 x 3 tensor takes more than one grid-stride trip at every workgroup cap the entry points use
  big = 16 * 256 * 256 * 3
  for cap in (1024, 512, 64):
    Lb, nb = E.reduction_chain(big, torch.bfloat16, cap)
    assert nb == cap and Lb >= 2 * 8 + cap
  assert E.reduction_chain(75, torch.bfloat16, 64, vec=False) == (1 + 6 + 4 + 1 + 1, 1)


# ------------------------------------------------------------------------------------------------ Adam
def test_adam_bound_accepts_fp32_arithmetic_and_rejects_a_wrong_epsilon_placement():
  """adam_step_bounds: numpy's float32 evaluation of the kernel's formula (with and without the products contracted into the
  sums) sits inside the per-element bounds for theta, m and v over ten steps with |g| from 1e-20 to 1e4 and g = 0; epsilon
  inside the root (the other Adam), a missing grad_scale, and beta2 used for m do not."""
  rng = np.random.RandomState(3)
  f = np.float32
  n = 257
  th, m, v = f(rng.randn(n)), np.zeros(n, f), np.zeros(n, f)
  th[::8] = 0.0      # where theta is of the update's own size nothing hides the update behind theta's rounding
  scale = np.where(np.arange(n) % 4 == 1, 1e4, np.where(np.arange(n) % 4 == 2, 1e-20, 1.0))
  scale[np.arange(n) % 4 == 3] = 0.0
  b1, b2, eps, gs = f(0.5), f(0.99), f(1e-8), f(1.0 / 1024)
  for step in range(1, 11):
    g = f(rng.randn(n) * scale * 1024)
    lr_t = f(1e-4 * np.sqrt(1 - 0.99 ** step) / (1 - 0.5 ** step))
    (rt, rm, rv), (bt, bm, bv) = E.adam_step_bounds(th.astype(np.float64), g.astype(np.float64), m.astype(np.float64),
                                                    v.astype(np.float64), lr_t, b1, b2, eps, gs)
    with np.errstate(under='ignore'):
      gi = g * gs
      mi = b1 * m + (f(1) - b1) * gi
      vi = b2 * v + (f(1) - b2) * gi * gi
      t = th - lr_t * mi / (np.sqrt(vi) + eps)
      assert E.assert_elementwise(t, rt, bt, 'theta') <= 1.0 and E.assert_elementwise(mi, rm, bm, 'm') <= 1.0
      assert E.assert_elementwise(vi, rv, bv, 'v') <= 1.0
      # contracted: products in float64, one rounding at the sum
      mc = f(np.float64(b1) * m + np.float64(f(1) - b1) * gi)
      assert E.assert_elementwise(mc, rm, bm, 'm contracted') <= 1.0
      if step == 3:
        wrong = th - lr_t * mi / np.sqrt(vi + eps)
        assert E.check_elementwise(wrong, rt, bt, 'eps inside the root')[1] is not None
        assert E.check_elementwise(th - lr_t * (b1 * m + (f(1) - b1) * g) / (np.sqrt(vi) + eps), rt, bt, 'no grad_scale')[1] is not None
        assert E.check_elementwise(b2 * m + (f(1) - b2) * gi, rm, bm, 'beta2 for m')[1] is not None
    th, m, v = t, mi, vi


# ------------------------------------------------------------------------------------------------ spectral norm
F32 = np.float32


def sn_model(w, u, G, drop_cols_from=None, drop_last_split_row=False, drop_b=False, unclamped_nv=False):
  """csrc/sn.hip in numpy float32 (sums by numpy: the order is not what the faults are about) with a planted fault:
      drop_cols_from        sn_finish's ur[j] loop stops after j = 0: columns >= 256 of u_raw read 0
      drop_last_split_row   sn_coldot's last K split (ks = 15) leaves its last row out
      drop_b                the b (x) u term missing from the gradient
      unclamped_nv          stats[1] = |v_raw| instead of sqrt(max(|v_raw|^2, 1e-12))
  -> dict(w_bar, u_new, v, stats, gw)."""
  w, u, G = F32(w), F32(u).reshape(-1), F32(G)
  K, cout = w.shape
  v_raw = w @ u
  ss = F32((v_raw * v_raw).sum())
  inv_v = F32(1.0) / np.sqrt(np.maximum(ss, F32(1e-12)))
  rows = np.ones(K, bool)
  per = -(-K // 16)
  if drop_last_split_row and 15 * per < K:
    rows[K - 1] = False
  u_raw = (v_raw[rows] @ w[rows]) * inv_v
  if drop_cols_from is not None:
    u_raw[drop_cols_from:] = 0
  ssu = F32((u_raw * u_raw).sum())
  inv_u = F32(1.0) / np.sqrt(np.maximum(ssu, F32(1e-12)))
  sigma = ssu * inv_u
  u_new, v = u_raw * inv_u, v_raw * inv_v
  nv = np.sqrt(ss) if unclamped_nv else F32(1.0) / inv_v
  a = w @ u_new
  b = np.zeros_like(a) if drop_b else (a - v * F32((v * a).sum())) / nv
  s = F32((G * w).sum())
  gw = G / sigma - (s / (sigma * sigma)) * (np.outer(v, u_new) + np.outer(b, u))
  return dict(w_bar=w / sigma, u_new=u_new, v=v, stats=np.array([sigma, nv]), gw=gw)


def _sn_case(K, cout, scale=0.1, converged=False, seed=5):
  g = torch.Generator().manual_seed(seed)
  w = (scale * torch.randn(K, cout, generator=g, dtype=torch.float64)).float()
  u = torch.randn(1, cout, generator=g, dtype=torch.float64)
  if converged == 'svd':
    u = torch.linalg.svd(w.double())[2][:1]
  elif converged:
    l2n = lambda x: x / x.norm()
    for _ in range(30):
      u = l2n(l2n(u @ w.double().t()) @ w.double())
  return w, u.float(), torch.randn(K, cout, generator=g)


def sn_guard_today(got, ref):
  """test_spectral_norm_matches_oracle as it stands: rel-L2 < 2e-5 on w_bar and u', < 1e-4 on the gradient."""
  return rel_l2(got['w_bar'], ref['w_bar']) < 2e-5 and rel_l2(got['u_new'], ref['u_new']) < 2e-5 and rel_l2(got['gw'], ref['gw']) < 1e-4


def _sn_rejects(got, ref, bound, keys=('w_bar', 'u_new', 'v', 'stats', 'gw')):
  return [k for k in keys if E.check_elementwise(got[k], ref[k], bound[k], k)[1] is not None]


SN_OLD = [(144, 32), (3, 16), (1024, 64), (2376, 256), (45, 7)]      # test_spectral_norm_matches_oracle's five, as [K, cout]


def test_planted_spectral_norm_faults():
  """The clean numpy model is inside sn_bounds at every shape used here.  Then, per fault, what the new check and the old
  guard (rel-L2 at the old five shapes, w ~ 0.1 N(0, 1), a random u) make of it:
    columns >= 256 of u_raw dropped     old shapes have cout <= 256: the faulty model returns the SAME BITS there -- no guard can see
                                        it; at cout = 257 u'[256] = 0 is outside its bound (rel-L2 would see it at that shape too: the
                                        gain is the shape)
    last row of the last K split        rejected by both wherever split 15 is not empty (K = 144, 1024, 2376 of the old five):
                                        the old guard was as sharp
    b (x) u missing, random u           rejected by both
    b (x) u missing, u after 30 iterations   a random 144 x 32 matrix has a small spectral gap: b is not yet 0, the gradient is
                                        off by 7.7e-5 in rel-L2 -- UNDER the old 1e-4 -- and by 136 bounds element-wise: the one
                                        arithmetic fault here that the old guard passes
    b (x) u missing, u the singular vector   b = 0 up to rounding: NEITHER sees it -- which is why the random state stays in the test
    stats[1] unclamped                  the same bits wherever |v_raw| >= 1e-6; below the clamp the saved stats (checked directly now,
                                        never before) are outside their bound
  For fp32 spectral norm the rel-L2 guard at 2e-5 is about as sharp as the bound (16 E32 is of the same order): what is new is
  the shapes, the states and the entry points, not the arithmetic of the bound."""
  for K, cout in SN_OLD + [(72, 257), (16, 129), (1, 1), (5, 1)]:
    w, u, G = _sn_case(K, cout)
    ref, bound = E.sn_bounds(w, u, G)
    assert _sn_rejects(sn_model(w, u, G), ref, bound) == [], (K, cout)
  # columns >= 256
  for K, cout in SN_OLD:
    w, u, G = _sn_case(K, cout)
    a, b = sn_model(w, u, G), sn_model(w, u, G, drop_cols_from=256)
    assert all(np.array_equal(a[k], b[k]) for k in a)
  w, u, G = _sn_case(72, 257)
  ref, bound = E.sn_bounds(w, u, G)
  bad = sn_model(w, u, G, drop_cols_from=256)
  assert 'u_new' in _sn_rejects(bad, ref, bound) and not sn_guard_today(bad, ref)
  # last row of the last K split
  seen_old = []
  for K, cout in SN_OLD + [(16, 129)]:
    w, u, G = _sn_case(K, cout)
    ref, bound = E.sn_bounds(w, u, G)
    bad = sn_model(w, u, G, drop_last_split_row=True)
    hit = 15 * -(-K // 16) < K
    assert bool(_sn_rejects(bad, ref, bound)) == hit and (not sn_guard_today(bad, ref)) == hit, (K, cout)
    seen_old.append(hit)
  assert seen_old == [True, False, True, True, False, True]
  # b (x) u
  w, u, G = _sn_case(144, 32)
  ref, bound = E.sn_bounds(w, u, G)
  bad = sn_model(w, u, G, drop_b=True)
  assert _sn_rejects(bad, ref, bound) == ['gw'] and not sn_guard_today(bad, ref)
  w, u, G = _sn_case(144, 32, converged=True)
  ref, bound = E.sn_bounds(w, u, G)
  bad = sn_model(w, u, G, drop_b=True)
  assert _sn_rejects(bad, ref, bound) == ['gw'] and sn_guard_today(bad, ref) and 5e-5 < rel_l2(bad['gw'], ref['gw']) < 1e-4
  w, u, G = _sn_case(144, 32, converged='svd')
  ref, bound = E.sn_bounds(w, u, G)
  bad = sn_model(w, u, G, drop_b=True)
  assert _sn_rejects(bad, ref, bound) == [] and sn_guard_today(bad, ref)
  # stats[1]
  w, u, G = _sn_case(144, 32)
  a, b = sn_model(w, u, G), sn_model(w, u, G, unclamped_nv=True)
  assert all(np.array_equal(a[k], b[k]) for k in a)
  w, u, G = _sn_case(144, 32, scale=1e-8 / (144 * 32) ** 0.5)
  ref, bound = E.sn_bounds(w, u, G)
  fwd = ('w_bar', 'u_new', 'v', 'stats')
  assert ref['stats'][1] == 1e-6 and _sn_rejects(sn_model(w, u, G), ref, bound, fwd) == []
  assert _sn_rejects(sn_model(w, u, G, unclamped_nv=True), ref, bound, fwd) == ['stats']


def test_planted_spectral_norm_sink_and_job_table_faults():
  """accumulate overwriting the sink: the sink holds gw (the last call's) and not sink0 + 2 gw -- outside the two-call bound at
  every element where sink0 + gw is not ~ 0; no test asked before.  Job 17's blocks of the finish pass taking job 16's fin0: its
  local block index is off by job 16's block count, so its first blocks of w_bar and (local block 0 never runs) u', v and stats
  keep what the buffers held -- the bit-for-bit comparison with the one-kernel path fails; the old table had 6 jobs: no test."""
  w, u, G = _sn_case(63, 17)
  ref, bound = E.sn_bounds(w, u, G)
  gw = sn_model(w, u, G)['gw']
  sink0 = np.random.RandomState(1).randn(63, 17).astype(np.float32)
  want = sink0.astype(np.float64) + 2.0 * ref['gw']
  b2 = 2.0 * bound['gw'] + 2.0 * E.U32 * np.abs(want)
  assert E.check_elementwise((sink0 + gw) + gw, want, b2, 'sink')[1] is None
  worst, msg = E.check_elementwise(gw, want, b2, 'sink overwritten')
  assert msg is not None and worst > 1e3
  # the job table: fin0 = running total of ceil(K cout / 1024) blocks
  sizes = [63 * 129, 1 * 1, 33 * 1024, 5 * 1] * 5
  fin0 = np.concatenate([[0], np.cumsum([-(-s // 1024) for s in sizes])])
  j = 17
  w17 = np.random.RandomState(2).randn(sizes[j]).astype(np.float32)
  out = np.full(sizes[j], -7.25, np.float32)      # what the buffer held
  shift = int(fin0[j] - fin0[j - 1])                  # blockIdx - fin0[16] = local + shift
  for blk in range(-(-sizes[j] // 1024)):
    lo = (blk + shift) * 1024
    out[lo:min(sizes[j], lo + 1024)] = w17[lo:min(sizes[j], lo + 1024)] * F32(0.5)
  assert shift >= 1 and not np.array_equal(out, w17 * F32(0.5))


# ------------------------------------------------------------------------------------------------ the loss tail
def test_planted_loss_tail_faults():
  """None of these entry points had an operator test ("no test" is the old guard throughout):
    cosine backward without the clamped branch    (ehat - phat cos) / |p| below the clamp: outside the bound on the clamped family
    pred_losses dividing by 256, not group_size   the same bits at group_size = 256, outside at 255 and 257
    a hinge derivative taken with >=              differs only where a + b x = 0 exactly: the planted +-1
    the wave GEMM kernel at k = 31                lanes 31..63 add terms from past the row: garbage of the operands' size
    FC gb missing columns >= 64                   the same bits for n <= 64 (every listed shape); outside at n = 70
    the dot product's last partial dropped        the same bits at one partial (the 132 elements of the old test); outside at 16385"""
  rng = np.random.RandomState(8)
  # cosine
  e, p = torch.from_numpy(F32(rng.randn(3, 5))), torch.from_numpy(F32(rng.randn(3, 5) * 1e-8))
  ref, _, b_gp = E.cosine_bounds(e, p, 0.7, 2.5)
  en, pn = e.double().numpy(), p.double().numpy()
  ie, ip = 1 / np.sqrt((en * en).sum(1, keepdims=True)), 1e6
  k = -0.7 * 2.5 / 3
  clean = k * (en * ie) * ip
  assert E.check_elementwise(F32(clean), ref['gp'], b_gp, 'clamped branch')[1] is None
  cos = (en * pn).sum(1, keepdims=True) * ie * ip
  assert E.check_elementwise(F32(k * (en * ie - pn * ip * cos) * ip), ref['gp'], b_gp, 'no clamped branch')[1] is not None
  # pred_losses / 256
  for gs, same in ((255, False), (256, True), (257, False)):
    x = F32(rng.randn(gs) * 4).astype(np.float64)
    f, df, parts, term_ops, _ = E.pred_loss_reference(x, 1, 1.0, -1.0)
    bound = E.pred_loss_fwd_bound(parts.sum(), gs, 0.5 / gs, term_ops, extra_ops=3)
    assert abs(F32(0.5 * f.sum() / gs) - 0.5 * f.sum() / gs) <= bound
    assert (abs(F32(0.5 * f.sum() / 256) - 0.5 * f.sum() / gs) <= bound) == same
  # hinge >=
  x = np.array([0.5, 1.0, 3.0, -1.0])
  f, df, _, _, _ = E.pred_loss_reference(x, 1, 1.0, -1.0)
  g = 0.25
  wrong = g * np.where(1.0 - x >= 0, -1.0, 0.0)
  assert E.check_elementwise(g * df, g * df, E.pred_loss_bwd_bound(g * df, g, None), 'hinge')[1] is None
  w, msg = E.check_elementwise(wrong, g * df, E.pred_loss_bwd_bound(g * df, g, None), 'hinge >=')
  assert msg is not None and 'd0 1..1' in msg
  # wave kernel at k = 31
  a, b = F32(rng.randn(3, 31)).astype(np.float64), F32(rng.randn(31, 5)).astype(np.float64)
  ref_c = a @ b
  bound = E.conv_bound(ref_c, np.abs(a) @ np.abs(b), 31, 'f32')
  assert E.check_elementwise(F32(ref_c), ref_c, bound, 'gemm')[1] is None
  garbage = (rng.randn(3, 33) @ rng.randn(33, 5))
  assert E.check_elementwise(F32(ref_c + garbage), ref_c, bound, 'gemm lanes >= k')[1] is not None
  # FC gb
  for n, same in ((16, True), (64, True), (70, False)):
    gq = F32(rng.randn(3, n)).astype(np.float64)
    rgb = gq.sum(0)
    got = F32(rgb).copy()
    got[64:] = 0
    assert (E.check_elementwise(got, rgb, E.wgrad_bound(rgb, np.abs(gq).sum(0), 3), 'fc gb')[1] is None) == same
  # dot
  for numel, same in ((132, True), (16385, False)):
    x, y = F32(rng.randn(numel)).astype(np.float64), F32(rng.randn(numel)).astype(np.float64)
    x[-1], y[-1] = 3.0, 3.0
    L, nparts, per = E.dot_chain(numel)
    bound = E.reduction_bound(np.abs(x * y).sum(), L, term_ops=1)
    kept = (x * y)[:(nparts - 1) * per].sum() if nparts > 1 else (x * y).sum()
    assert abs(F32((x * y).sum()) - (x * y).sum()) <= bound and (abs(kept - (x * y).sum()) <= bound) == same


# ------------------------------------------------------------------------------------------------ preprocessing
def test_planted_preprocessing_faults(monkeypatch):
  """The oracle with a fault planted, against the clean oracle under the new test's bound (3e-6 in fp32), and what the old checks
  (tests/test_gpu_data.py: max-abs < 2e-6 / 3e-6, sources at least as large as the target, hw = 32 / 256, random pixels) make of it:
    bot / right not clamped       a tap past the rectangle reads the zero padding.  Down-sampling (scale >= 1) never reaches it:
                                  the same values at the old sizes.  A 1 x 1 source up-sampled to 5 x 5 goes dark: rejected
    the flip applied to the source, not to the resized image
                                  bilinear without half-pixel centres is not mirror-symmetric: rejected, and by the old check too
                                  (its fixture has flips); with a crop rectangle, which the old batch tests did not flip, as well
    saturate dividing by s = 0    NaN on grey, black and white pixels; random pixels are never exactly grey: the old inputs do not
                                  reach it, the grey / black / white sources do
    a ragged last workgroup not written
                                  hw = 32 and 256 are multiples of 256 pixels: nothing ragged; at hw = 33 the last 65 pixels keep the
                                  buffer's fill"""
  rng = np.random.RandomState(4)
  real = N.resize_bilinear_tf1

  def unclamped(x, out_h, out_w):
    h, w = x.shape[:2]
    pad = np.zeros((h + 1, w + 1, x.shape[2]))
    pad[:h, :w] = x
    fy = np.arange(out_h, dtype=np.float32) * (np.float32(h) / np.float32(out_h))
    fx = np.arange(out_w, dtype=np.float32) * (np.float32(w) / np.float32(out_w))
    top, left = np.floor(fy).astype(int), np.floor(fx).astype(int)
    ly = (fy - top.astype(np.float32)).astype(np.float64)[:, None, None]
    lx = (fx - left.astype(np.float32)).astype(np.float64)[None, :, None]
    t = pad[top][:, left] + (pad[top][:, left + 1] - pad[top][:, left]) * lx
    b = pad[top + 1][:, left] + (pad[top + 1][:, left + 1] - pad[top + 1][:, left]) * lx
    return t + (b - t) * ly

  big, dot = rng.randint(0, 256, (48, 70, 3), dtype=np.uint8), rng.randint(1, 256, (1, 1, 3), dtype=np.uint8)
  want_big, want_dot = N.preprocess_image(big, 32, 'RESHAPE', False), N.preprocess_image(dot, 5, 'RESHAPE', False)
  monkeypatch.setattr(N, 'resize_bilinear_tf1', unclamped)
  assert np.abs(N.preprocess_image(big, 32, 'RESHAPE', False) - want_big).max() < 2e-6      # the old check passes
  got = N.preprocess_image(dot, 5, 'RESHAPE', False)
  monkeypatch.setattr(N, 'resize_bilinear_tf1', real)
  assert E.check_elementwise(got, want_dot, 3e-6, 'unclamped taps')[1] is not None
  # the flip
  for crop in (None, (0, 5, 6, 1)):
    kw = dict(saturation_first=False, delta=0.0, factor=1.0, crop=crop)
    want = N.preprocess_image(big, 5, 'RESHAPE', True, flip=True, **kw)
    got = N.preprocess_image(big[:, ::-1], 5, 'RESHAPE', True, flip=False, **kw)
    assert E.check_elementwise(got, want, 3e-6, 'flip of the source')[1] is not None
  want = N.preprocess_image(big, 32, 'RESHAPE', True, flip=True)
  assert np.abs(N.preprocess_image(big[:, ::-1], 32, 'RESHAPE', True, flip=False) - want).max() > 3e-6      # the old check fails too
  # saturate on s = 0
  def saturate_no_guard(c, factor):
    v = c.max(-1, keepdims=True)
    with np.errstate(invalid='ignore', divide='ignore'):
      s = (v - c.min(-1, keepdims=True)) / v
      return v - (v - c) * (np.minimum(s * factor, 1.0) / s)
  grey = np.repeat(rng.randint(0, 256, (4, 4, 1), dtype=np.uint8), 3, axis=2)
  for im, hit in ((big[:8, :8], False), (grey, True), (np.zeros((2, 2, 3), np.uint8), True), (np.full((2, 3, 3), 255, np.uint8), True)):
    x = N.preprocess_image(im, 4, 'RESHAPE', False)
    want = N.preprocess_image(im, 4, 'RESHAPE', True, factor=1.4)
    got = np.clip(saturate_no_guard(x, 1.4), 0.0, 1.0)
    assert (E.check_elementwise(got, want, 3e-6, 'saturate')[1] is not None) == hit
  # the ragged last workgroup
  for hw, hit in ((32, False), (33, True)):
    want = N.preprocess_image(big, hw, 'RESHAPE', False)
    got = np.full(hw * hw * 3, np.nan)
    full = (hw * hw // 256) * 256 * 3
    got[:full] = want.reshape(-1)[:full]
    assert (E.check_elementwise(got.reshape(want.shape), want, 3e-6, 'ragged workgroup')[1] is not None) == hit


# ------------------------------------------------------------------------------------------------ the gradient-penalty nodes
GP_ALPHA = float(np.float32(0.2))


def _gp_m(t):
  return np.where(t > 0, 1.0, GP_ALPHA)


def _gp_twice(ref, slope):
  u = E.unit_roundoff(torch.bfloat16)
  return (1 + u) * (u * np.abs(ref) + E.tiny(torch.bfloat16)) * (slope != 1.0)


@pytest.fixture(scope='module')
def gp_case():
  """The node outputs of tests/test_gpu_gp_nodes.py at n = 2, 32 x 32, 32 -> 64 in bf16, as clean rounded float64 references:
  independent random masks with planted +0.0 (every 7th element) and -0.0 (every 11th), vm = rnd(v m(x_act)),
      out   = dgrad(gy, w) m(x_act)                 MaskedDgradFn, first order            K = 9 64 + 1
      ggy   = conv(vm, w) m(out_act)                its d/dgy                             K = 9 32 + 1
      gw    = wgrad(vm, gy)                         its d/dw, fp32                        P = 2 32 32
      ggzp  = pool2(rnd(t m(z)))                    LReluPoolBwdFn's backward             the mean of four stored values"""
  n, hw, cin, cout = 2, 32, 32, 64
  rng = np.random.RandomState(77)

  def mask(shape):
    a = bf16(rng.randn(*shape))
    a.reshape(-1)[::7] = 0.0
    a.reshape(-1)[3::11] = -0.0
    return a
  gy, v, t = bf16(rng.randn(n, hw, hw, cout)), bf16(rng.randn(n, hw, hw, cin)), bf16(rng.randn(n, hw, hw, cout))
  w = bf16(rng.randn(3, 3, cin, cout) / np.sqrt(9 * cin))
  x_act, out_act = mask((n, hw, hw, cin)), mask((n, hw, hw, cout))
  xs, os_ = _gp_m(x_act), _gp_m(out_act)
  dg, dgmag = N.conv2d_bwd_data_gemm(gy, w, (hw, hw)), N.conv2d_bwd_data_gemm(np.abs(gy), np.abs(w), (hw, hw))
  vm = bf16((v * xs).astype(np.float32))
  lin, linmag = N.conv2d_gemm(vm, w), N.conv2d_gemm(np.abs(vm), np.abs(w))
  c = dict(n=n, hw=hw, cin=cin, cout=cout, gy=gy, v=v, w=w, x_act=x_act, out_act=out_act, xs=xs, os=os_, dg=dg, lin=lin, vm=vm)
  c['out'] = (dg * xs, E.conv_bound(dg * xs, dgmag * xs, 9 * cout + 1, torch.bfloat16, _gp_twice(dg * xs, xs)))
  c['ggy'] = (lin * os_, E.conv_bound(lin * os_, linmag * os_, 9 * cin + 1, torch.bfloat16, _gp_twice(lin * os_, os_)))
  gw = N.conv2d_bwd_weight_gemm(vm, gy, (3, 3))
  c['gw'] = (gw, E.wgrad_bound(gw, N.conv2d_bwd_weight_gemm(np.abs(vm), np.abs(gy), (3, 3)), n * hw * hw))
  tm = bf16((t * os_).astype(np.float32))                       # stored, then pooled: u |ref| of the mean of four
  pooled = tm.reshape(n, hw // 2, 2, hw // 2, 2, cout).mean(axis=(2, 4))
  c['ggzp'] = (pooled, E.rounded_bound(pooled, torch.bfloat16))
  c['t'] = t
  return c


def _gp_old_guard(got, clean, ref):
  """The two chain tests' thresholds (test_lrelu_fold_under_create_graph_matches_unfused,
  test_gradient_penalty_second_pass_masks_in_the_conv_epilogue), applied to the node's OWN tensor -- stricter than they ever
  were, those tests see it only through the layers that follow: rel-L2 < 3e-2 against the other route (the clean output
  stands for it) and < 6e-2 against float64."""
  return rel_l2(got, clean) < 3e-2 and rel_l2(got, ref) < 6e-2


def _gp_wrong_mask_on_a_tile(c, small):
  ref, _ = c['out']
  got = bf16(ref.astype(np.float32))
  zs = c['os'][..., :c['cin']]                                  # the OTHER mask of the node (z / out_act), its first cin channels
  h, w = (slice(8, 9), slice(16, 17)) if small else (slice(8, 16), slice(16, 24))      # small: the tile's corner pixel
  got[1, h, w, :] = bf16((c['dg'] * zs)[1, h, w, :].astype(np.float32))
  return 'out', got, dict(n=(1, 1), h=(8, h.stop - 1), w=(16, w.stop - 1))


def _gp_mask_twice_on_an_image(c, small):
  ref, _ = c['ggy']
  got = bf16(ref.astype(np.float32))
  rows = slice(31, 32) if small else slice(0, 32)               # small: the last row of that image
  got[1, rows] = bf16((ref[1, rows] * c['os'][1, rows]).astype(np.float32))
  return 'ggy', got, dict(n=(1, 1), h=(rows.start, 31), w=(0, 31))


def _gp_quarter_lost_on_the_last_pooled_row(c, small):
  ref, _ = c['ggzp']
  got = bf16(ref.astype(np.float32))
  sel = (0, 15, slice(15, 16), slice(63, 64)) if small else (0, 15, slice(0, 16), slice(0, 64))      # small: the row's last element
  got[sel] = bf16((4.0 * ref[sel]).astype(np.float32))
  return 'ggzp', got, dict(n=(0, 0), h=(15, 15), w=(sel[2].start, 15))


def _gp_filter_gradient_from_the_unmasked_cotangent(c, small):
  ref, _ = c['gw']
  got = ref.astype(np.float32).astype(np.float64)
  sel = (slice(2, 3), slice(2, 3), slice(31, 32), slice(16, 32)) if small else (slice(0, 3), slice(0, 3), slice(0, 32), slice(16, 32))
  got[sel] = N.conv2d_bwd_weight_gemm(c['v'], c['gy'], (3, 3))[sel].astype(np.float32)      # small: the block's last tap and input channel
  return 'gw', got, dict(c=(16, 31))      # a [kh, kw, cin, cout] tensor: the checker names its axes n, h, w, c


def _gp_negative_zero_taken_as_positive(c, small):
  ref, _ = c['out']
  pos = (c['x_act'] == 0) & np.signbit(c['x_act'])
  if small:                                                     # small: on four pixels of one row
    keep = np.zeros_like(pos)
    keep[1, 5, 8:12] = True
    pos &= keep
  got = bf16((c['dg'] * np.where(pos | (c['x_act'] > 0), 1.0, GP_ALPHA)).astype(np.float32))
  return 'out', got, (dict(n=(1, 1), h=(5, 5)) if small else dict(n=(0, 1), h=(0, 31), w=(0, 31), c=(0, 31)))


def test_clean_gp_node_outputs_pass(gp_case):
  for key in ('out', 'ggy', 'ggzp', 'gw'):
    ref, bound = gp_case[key]
    clean = ref.astype(np.float32).astype(np.float64) if key == 'gw' else bf16(ref.astype(np.float32))
    worst = E.assert_elementwise(clean, ref, bound, 'clean ' + key)
    print('clean gp node %s worst ratio %.3f' % (key, worst))
    assert worst <= 1.0 and _gp_old_guard(clean, clean, ref)


# fault, its extent -> does the old guard (on the node's own tensor, see _gp_old_guard) catch it?  Recorded from this test's own
# run.  At the extent the fault is named for, in a tensor of 2 x 32 x 32, rel-L2 sees all five (1.6e-1, 1.4e-1, 5.5e-1, 4.9e-1,
# 3.7e-1): the independent masks of these tests make a mask fault a factor of 5 on four elements in ten.  Confined to the
# smallest place a kernel could get it wrong (`small`) it is under both thresholds; the element-wise check rejects all ten
# and names the place
GP_FAULTS = [
    (_gp_wrong_mask_on_a_tile, 'm(z) for m(x_act) on one 8 x 8 tile', False, True),
    (_gp_wrong_mask_on_a_tile, 'm(z) for m(x_act) on one 8 x 8 tile', True, False),
    (_gp_mask_twice_on_an_image, 'the mask applied twice on one image', False, True),
    (_gp_mask_twice_on_an_image, 'the mask applied twice on one image', True, False),
    (_gp_quarter_lost_on_the_last_pooled_row, '0.25 missing on the last pooled row', False, True),
    (_gp_quarter_lost_on_the_last_pooled_row, '0.25 missing on the last pooled row', True, False),
    (_gp_filter_gradient_from_the_unmasked_cotangent, 'gw from the unmasked v for one 16-channel block', False, True),
    (_gp_filter_gradient_from_the_unmasked_cotangent, 'gw from the unmasked v for one 16-channel block', True, False),
    (_gp_negative_zero_taken_as_positive, '-0.0 taken as positive', False, True),
    (_gp_negative_zero_taken_as_positive, '-0.0 taken as positive', True, False),
]


@pytest.mark.parametrize('plant,name,small,old_catches', GP_FAULTS, ids=[f[0].__name__[4:] + ('-small' if f[2] else '') for f in GP_FAULTS])
def test_planted_gp_node_fault(gp_case, plant, name, small, old_catches):
  key, got, box = plant(gp_case, small)
  ref, bound = gp_case[key]
  clean = ref.astype(np.float32).astype(np.float64) if key == 'gw' else bf16(ref.astype(np.float32))
  print('%s%s: rel-L2 %.2e against the clean output, %.2e against float64' % (name, ' (small)' if small else '', rel_l2(got, clean), rel_l2(got, ref)))
  assert (not _gp_old_guard(got, clean, ref)) == old_catches, name          # half one: what the old thresholds make of it
  worst, msg = E.check_elementwise(got, ref, bound, name)
  assert msg is not None and worst > 10.0, (worst, msg)                     # half two: the element-wise check rejects it
  for axis, (lo, hi) in box.items():                                        # ... and says where
    assert '%s %d..%d' % (axis, lo, hi) in msg, (axis, lo, hi, msg)
