"""Kernel two-sample block sums on the device (include/twingan_hip_mmd.h, ops.mmd_block_sums, evaluate.KernelDistance,
evaluate_translation(latent=True)) against the float64 restatement tests/mmd_ref.py.  Also runs under TG_EMU=1 over the
emulated kernels.

Exact cases: rows in {-1, 0, 1}, d a power of two, gamma = 1 / d, coef0 = 1: the dot product is an integer, t = 1 + s / d is a
float32, every power is one correctly rounded float32 product (mmd_ref.pair_values(fp32_steps=True) takes the same), and the
fp64 sum of at most 2^17 float32 values of one binade's neighbourhood is exact in any order -- the block sums must EQUAL the
restatement's bit for bit.

Real-valued cases: Gaussian rows rounded to the dtype first; every block sum within mmd_ref.block_sum_bound, which is derived
from the inputs alone (its docstring: the fp32 chain's first-order error d 2^-24 sum|a_i b_i| on s, carried through gamma and
degree t^(degree - 1), plus the roundings of t and of the products, summed over the block's pairs)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guarded      # noqa: E402
import mmd_ref as R      # noqa: E402

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
DTYPES = {'fp32': torch.float32, 'bf16': torch.bfloat16, 'fp16': torch.float16}
SHAPES = [(33, 257), (70, 1000), (5, 515)]
REAL_SHAPES = [(33, 257, 24), (70, 1000, 130), (5, 515, 1031)]


def _signs(seed, m, n, d):
  rng = np.random.default_rng(seed)
  return rng.integers(-1, 2, size=(m, d)).astype(np.float32), rng.integers(-1, 2, size=(n, d)).astype(np.float32)


def _reals(seed, m, n, d, dt):
  """Gaussian rows rounded to the dtype: -> float32 arrays that hold exactly the rounded values."""
  g = torch.Generator().manual_seed(seed)
  return tuple(torch.randn(r, d, generator=g).to(dt).float().numpy() for r in (m, n))


def _dev(a, dt):
  return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(dt).contiguous()


def _sums(a, b, **kw):
  from twingan_amd import ops
  out = ops.mmd_block_sums(a, b, **kw)
  torch.cuda.synchronize()
  return out.cpu().numpy()


# ------------------------------------------------------------------------------------------------ exact
@pytest.fixture(scope='module')
def exact_inputs():
  return {(m, n, d): _signs(m + n + d, m, n, d) for (m, n) in SHAPES for d in (32, 64, 256)}


@pytest.mark.parametrize('dtype', list(DTYPES))
@pytest.mark.parametrize('d', [32, 64, 256])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'm%d_n%d' % s)
def test_exact_cases_equal_the_restatement_bit_for_bit(shape, d, dtype, exact_inputs):
  m, n = shape
  a, b = exact_inputs[(m, n, d)]
  ad, bd = _dev(a, DTYPES[dtype]), _dev(b, DTYPES[dtype])
  for block in (32, 128, 1024):      # 1024 >= m and >= n: one block
    want = R.block_sums(a, b, block, fp32_steps=True)
    got = _sums(ad, bd, block=block)
    assert got.shape == want.shape == (-(-m // block), -(-n // block)) and got.dtype == np.float64
    assert got.tobytes() == want.tobytes(), (block, np.abs(got - want).max())
  # b against itself without the diagonal, and row ranges that put the diagonal across block borders
  for block in (32, 128):
    want = R.block_sums(b, b, block, skip_same_index=True, fp32_steps=True)
    assert _sums(bd, bd, block=block, skip_same_index=True).tobytes() == want.tobytes(), block
    want = R.block_sums(b, b, block, a_index0=0, b_index0=40, skip_same_index=True, fp32_steps=True)      # pairs (j + 40, j)
    assert _sums(bd, bd, block=block, a_index0=0, b_index0=40, skip_same_index=True).tobytes() == want.tobytes(), block
  big = 1 << 33
  for a0, b0 in ((big + 40, big), (big, big + 7), (0, 31), (300, 0)):
    want = R.block_sums(a, b, 32, a_index0=a0, b_index0=b0, skip_same_index=True, fp32_steps=True)
    got = _sums(ad, bd, block=32, a_index0=a0, b_index0=b0, skip_same_index=True)
    assert got.tobytes() == want.tobytes(), (a0, b0)
    plain = R.block_sums(a, b, 32, fp32_steps=True)
    hit = max(0, min(m, n + b0 - a0) - max(0, b0 - a0))      # pairs on the moved diagonal
    assert int((want != plain).sum()) <= hit and (hit == 0) == np.array_equal(want, plain)


# ------------------------------------------------------------------------------------------------ real-valued
@pytest.mark.parametrize('dtype', list(DTYPES))
@pytest.mark.parametrize('shape', REAL_SHAPES, ids=lambda s: 'm%d_n%d_d%d' % s)
def test_real_valued_cases_within_the_derived_bounds(shape, dtype):
  m, n, d = shape
  a, b = _reals(7 + m, m, n, d, DTYPES[dtype])
  ad, bd = _dev(a, DTYPES[dtype]), _dev(b, DTYPES[dtype])
  worst = 0.0
  for degree in (1, 2, 3, 4):
    for kw in (dict(block=32), dict(block=128, gamma=0.05, coef0=0.5), dict(block=64, a_index0=3, b_index0=0, skip_same_index=True)):
      want, bound = R.block_sums(a, b, degree=degree, **kw), R.block_sum_bound(a, b, degree=degree, **kw)
      got = _sums(ad, bd, degree=degree, **kw)
      ratio = float((np.abs(got - want) / bound).max())
      worst = max(worst, ratio)
      print('[mmd %s %s degree %d %s] worst error / bound %.4f' % (dtype, shape, degree, kw, ratio))
      assert np.all(np.abs(got - want) <= bound), (degree, kw, ratio)
  print('[mmd %s %s] worst error / bound over all %.4f' % (dtype, shape, worst))


@pytest.fixture(scope='module')
def full_width():
  """1024 x 1024 x 4096: the rows (bf16-rounded) and the restatement with its bounds, computed once."""
  g = torch.Generator().manual_seed(77)
  x = torch.randn(1024, 4096, generator=g).to(torch.bfloat16)
  y = (torch.randn(1024, 4096, generator=g) * 1.05 + 0.02).to(torch.bfloat16)
  xf, yf = x.float().numpy(), y.float().numpy()
  return x, y, R.kernel_distance(xf, yf, subset_size=512), R.kernel_distance_bound(xf, yf, subset_size=512, with_max=True)


def test_full_width_bf16_estimates_within_the_implied_bound(full_width):
  from twingan_amd.evaluate import KernelDistance
  x, y, want, (b_mmd2, b_kid, b_max) = full_width
  kd = KernelDistance(4096, 1024, subset_size=512)
  kd.feed(x.to(DEV), y.to(DEV))
  got = kd.end()
  print('[mmd full width] mmd2 %.9e want %.9e bound %.3e (error / bound %.4f); kid_mean %.9e want %.9e bound %.3e (%.4f)'
        % (got['mmd2'], want['mmd2'], b_mmd2, abs(got['mmd2'] - want['mmd2']) / b_mmd2, got['kid_mean'], want['kid_mean'], b_kid,
           abs(got['kid_mean'] - want['kid_mean']) / b_kid))
  assert (got['m'], got['n'], got['num_subsets'], got['subset_size']) == (1024, 1024, 2, 512)
  assert abs(got['mmd2'] - want['mmd2']) <= b_mmd2
  assert abs(got['kid_mean'] - want['kid_mean']) <= b_kid
  assert abs(got['kid_std'] - want['kid_std']) <= b_max      # the standard deviation moves by at most the largest subset error


# ------------------------------------------------------------------------------------------------ determinism, position
@pytest.mark.parametrize('dtype', list(DTYPES))
def test_same_call_same_bits_and_the_pair_value_does_not_depend_on_position(dtype):
  m, n, d = 70, 333, 130
  a, b = _reals(3, m, n, d, DTYPES[dtype])
  ad, bd = _dev(a, DTYPES[dtype]), _dev(b, DTYPES[dtype])
  for block in (32, 128):
    assert _sums(ad, bd, block=block).tobytes() == _sums(ad, bd, block=block).tobytes()
  # one non-zero row among zero rows, whose pairs are exactly coef0 ** degree = 1 / 8: wherever the row sits, the two blocks
  # of its block row hold count / 8 plus what the row's pairs add, v_J = sum_j (p(row, b_j) - 1 / 8) over block J's columns,
  # and v_J is read off a launch of the row alone.  All of it exact: the p are float32 in [2^-7, 1], fewer than 2^11 a block
  row, cols = a[:1], b[:40]
  probe = _dev(cols, DTYPES[dtype])
  alone = [_sums(_dev(row, DTYPES[dtype]), _dev(cols[lo:hi], DTYPES[dtype]), block=32, coef0=0.5)[0, 0] for lo, hi in ((0, 32), (32, 40))]
  assert all(0.0 < v < 32.0 for v in alone)
  counts = np.outer([32, 32, 6], [32, 8]).astype(np.float64)
  for pos in (0, 31, 32, 69):
    z = np.zeros((m, d), dtype=np.float32)
    z[pos] = row[0]
    got = _sums(_dev(z, DTYPES[dtype]), probe, block=32, coef0=0.5)
    want = counts / 8
    want[pos // 32, 0] += alone[0] - 32 / 8
    want[pos // 32, 1] += alone[1] - 8 / 8
    assert got.tobytes() == want.tobytes(), (pos, got, want)


@pytest.mark.parametrize('dtype', list(DTYPES))
def test_nan_and_inf_rows_reach_exactly_their_own_blocks(dtype):
  m, n, d = 70, 333, 40
  a, b = _reals(19, m, n, d, DTYPES[dtype])
  ad, bd = _dev(a, DTYPES[dtype]), _dev(b, DTYPES[dtype])
  clean = _sums(ad, bd, block=32)
  a2, b2 = a.copy(), b.copy()
  a2[33, 5] = np.nan
  b2[200, 0] = np.inf
  got = _sums(_dev(a2, DTYPES[dtype]), _dev(b2, DTYPES[dtype]), block=32)
  hit = np.zeros_like(clean, dtype=bool)
  hit[33 // 32, :] = True
  hit[:, 200 // 32] = True
  assert got[~hit].tobytes() == clean[~hit].tobytes()
  assert not np.isfinite(got[hit]).any()
  assert np.isnan(got[1]).all()
  # the set against itself, a -inf row, the diagonal left out: rows and columns of its block
  b3 = b.copy()
  b3[100, 1] = -np.inf
  self_clean = _sums(bd, bd, block=64, skip_same_index=True)
  got = _sums(_dev(b3, DTYPES[dtype]), _dev(b3, DTYPES[dtype]), block=64, skip_same_index=True)
  hit = np.zeros_like(self_clean, dtype=bool)
  hit[1, :] = True
  hit[:, 1] = True
  assert got[~hit].tobytes() == self_clean[~hit].tobytes() and not np.isfinite(got[hit]).any()


# ------------------------------------------------------------------------------------------------ refusals, guard bands
def test_every_refusal_names_its_argument():
  from twingan_amd import _lib, ops
  a = torch.zeros(4, 16, dtype=torch.bfloat16, device=DEV)
  b = torch.zeros(10, 16, dtype=torch.bfloat16, device=DEV)
  sums = torch.zeros(1, 1, dtype=torch.float64, device=DEV)
  ws = torch.zeros(8, dtype=torch.float64, device=DEV)
  lib = _lib.load()
  assert lib.tg_mmd_workspace_bytes(4, 10, 16, 32) == 8 and lib.tg_mmd_workspace_bytes(33, 65, 16, 64) == 2 * 3 * 8
  assert lib.tg_mmd_workspace_bytes(0, 10, 16, 32) == 0 and lib.tg_mmd_workspace_bytes(4, 10, 16, 48) == 0

  def call(**over):
    v = dict(a=a.data_ptr(), m=4, b=b.data_ptr(), n=10, d=16, dtype=ops._dt(a), degree=3, gamma=1 / 16, coef0=1.0, block=32, a0=0, b0=0,
             skip=0, sums=sums.data_ptr(), ws=ws.data_ptr(), ws_bytes=8)
    v.update(over)
    _lib.call('tg_mmd_block_sums', v['a'], v['m'], v['b'], v['n'], v['d'], v['dtype'], v['degree'], v['gamma'], v['coef0'], v['block'],
              v['a0'], v['b0'], v['skip'], v['sums'], v['ws'], v['ws_bytes'], ops._stream())

  call()
  for over, text in ((dict(a=None), 'NULL'), (dict(b=None), 'NULL'), (dict(sums=None), 'NULL'), (dict(ws=None), 'NULL'),
                     (dict(m=0), 'm = 0'), (dict(n=0), 'n = 0'), (dict(n=(1 << 20) + 1), 'n = 1048577'), (dict(d=0), 'd = 0'),
                     (dict(dtype=7), 'dtype 7'), (dict(degree=0), 'degree = 0'), (dict(degree=5), 'degree = 5'),
                     (dict(block=0), 'block = 0'), (dict(block=48), 'block = 48'), (dict(block=-32), 'block = -32'),
                     (dict(a0=-1), 'a_index0'), (dict(b0=-1), 'b_index0'), (dict(ws_bytes=7), 'workspace of 7 bytes'),
                     (dict(ws=ws.data_ptr() + 4, ws_bytes=8), 'workspace not 8-byte aligned')):
    with pytest.raises(_lib.TgError, match=text):
      call(**over)
  # the wrapper: one dtype, one d, the shape of out
  with pytest.raises(_lib.TgError, match='float16'):
    ops.mmd_block_sums(a, b.to(torch.float16))
  with pytest.raises(_lib.TgError, match=r'\[., 8\]'):
    ops.mmd_block_sums(a, b[:, :8].contiguous())
  with pytest.raises(_lib.TgError, match='out must be fp64'):
    ops.mmd_block_sums(a, b, out=torch.zeros(2, 1, dtype=torch.float64, device=DEV))
  with pytest.raises(_lib.TgError, match='block = 40'):
    ops.mmd_block_sums(a, b, block=40)
  with pytest.raises(_lib.TgError, match='degree = 9'):
    ops.mmd_block_sums(a, b, degree=9)
  torch.cuda.synchronize()


@pytest.mark.parametrize('dtype', list(DTYPES))
@pytest.mark.parametrize('shape', [(1, 1, 1), (33, 257, 24), (70, 333, 27)], ids=lambda s: 'm%d_n%d_d%d' % s)
def test_guard_bands_and_poison_round_every_buffer(shape, dtype):
  """tests/guarded.py: the operands sit between NaN bytes and are unchanged afterwards, the sums and the workspace ops.py
  allocates sit between guard bytes that stay intact and start out as NaN, and the result equals the ordinary run's and the
  restatement's.  d = 27 and 24 take the scalar tail of the staging."""
  from twingan_amd import ops
  m, n, d = shape
  a, b = _signs(61, m, n, d)
  ad, bd = _dev(a, DTYPES[dtype]), _dev(b, DTYPES[dtype])
  for kw in (dict(block=32, gamma=0.25), dict(block=64, gamma=0.25, skip_same_index=True, a_index0=2)):
    served = []
    A, B = guarded.check(lambda x, y: ops.mmd_block_sums(x, y, **kw), [ad, bd], DEV, sync=torch.cuda.synchronize, served=served)
    assert len(served) >= 2, served      # sums, workspace
    want = R.block_sums(a, b, fp32_steps=True, **kw)      # gamma = 1 / 4: t is a multiple of 1 / 4, exact
    assert B.cpu().numpy().tobytes() == want.tobytes()
  out = torch.zeros(-(-m // 32), -(-n // 32), dtype=torch.float64, device=DEV)
  guarded.check(lambda x, y, o: ops.mmd_block_sums(x, y, gamma=0.25, out=o), [ad, bd, out], DEV, inout=(2,), sync=torch.cuda.synchronize)


# ------------------------------------------------------------------------------------------------ KernelDistance
def test_kernel_distance_does_not_depend_on_the_feeds_and_a_seed_fixes_it():
  from twingan_amd import _lib
  from twingan_amd.evaluate import KernelDistance
  m, n, d = 200, 170, 48
  x, y = _reals(29, m, n, d, torch.bfloat16)
  y = y + 0.25
  xd, yd = _dev(x, torch.bfloat16), _dev(y, torch.bfloat16)
  xf, yf = xd.float().cpu().numpy(), yd.float().cpu().numpy()
  kd = KernelDistance(d, 256, subset_size=64)
  kd.feed(xd, yd)
  one = kd.end()
  want, (b_mmd2, b_kid) = R.kernel_distance(xf, yf, subset_size=64), R.kernel_distance_bound(xf, yf, subset_size=64)
  assert (one['m'], one['n'], one['num_subsets'], one['subset_size']) == (m, n, 2, 64) == (want['m'], want['n'], want['num_subsets'], 64)
  assert abs(one['mmd2'] - want['mmd2']) <= b_mmd2 and abs(one['kid_mean'] - want['kid_mean']) <= b_kid
  assert one['mmd2'] > 10 * b_mmd2      # the shift is seen
  kd.begin()
  for lo in range(0, 200, 37):      # ragged, one-sided, interleaved feeds
    kd.feed(xd[lo:lo + 37], None)
    kd.feed(None, yd[lo:lo + 37] if lo < n else None)
  again = kd.end()
  assert again == one      # bitwise: floats compare by value, and every value is a float or an int
  # a seed fixes the permutation, and so the result; another seed cuts other subsets but leaves mmd2 to rounding
  seeded = [KernelDistance(d, 256, subset_size=64, shuffle_seed=s) for s in (5, 5, 6)]
  res = []
  for k in seeded:
    k.feed(xd, yd)
    res.append(k.end())
  assert res[0] == res[1] and res[0]['kid_mean'] != res[2]['kid_mean'] and res[0]['kid_mean'] != one['kid_mean']
  assert abs(res[0]['mmd2'] - one['mmd2']) <= 2 * b_mmd2 and abs(res[2]['mmd2'] - one['mmd2']) <= 2 * b_mmd2
  gen = torch.Generator().manual_seed(5)
  px, py = torch.randperm(m, generator=gen).numpy(), torch.randperm(n, generator=gen).numpy()
  want5 = R.kernel_distance(xf[px], yf[py], subset_size=64)
  assert abs(res[0]['kid_mean'] - want5['kid_mean']) <= R.kernel_distance_bound(xf[px], yf[py], subset_size=64)[1]
  # refusals: overflow, one-sided, fewer rows than a subset
  with pytest.raises(_lib.TgError, match='the buffers hold 256'):
    kd.feed(xd[:100], None)
  kd.begin()
  kd.feed(xd, None)
  with pytest.raises(_lib.TgError, match='at least 2 rows'):
    kd.end()
  kd.feed(None, yd[:1])
  with pytest.raises(_lib.TgError, match='at least 2 rows'):
    kd.end()
  kd.feed(None, yd[1:40])
  few = kd.end()
  assert (few['num_subsets'], few['kid_mean'], few['kid_std'], few['n']) == (0, None, None, 40) and np.isfinite(few['mmd2'])
  with pytest.raises(_lib.TgError, match='rows'):
    kd.feed(xd[:, :8], None)
  with pytest.raises(_lib.TgError, match='float32'):
    kd.feed(xd[:4].float(), None)
  torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ evaluate_translation
def _stand_ins(dtype):
  """translate_fn / encode_fn stand-ins that record what they return: a fixed random projection of the image per domain."""
  g = torch.Generator().manual_seed(91)
  proj = {dom: (torch.randn(16 * 16 * 3, 128, generator=g) / 16).to(DEV).to(dtype) for dom in 'st'}
  seen = []

  def translate_fn(x, to):
    return (x * 0.5 + 0.25 if to == 't' else x).contiguous()

  def encode_fn(x, domain):
    e = (x.reshape(x.shape[0], -1) @ proj[domain]).contiguous()
    seen.append((domain, e))
    return e
  return translate_fn, encode_fn, seen


def _images(seed, n, hw=16):
  g = torch.Generator().manual_seed(seed)
  return torch.rand(n, hw, hw, 3, generator=g).numpy()


def _check_latent(got, rows, subset):
  """got: out['latent']; rows: {'src', 'fake', 'tgt'} float32 arrays of the embeddings that were fed."""
  half = rows['tgt'].shape[0] // 2
  pairs = {'domains': (rows['src'], rows['tgt']), 'translation': (rows['fake'], rows['tgt']), 'floor': (rows['tgt'][:half], rows['tgt'][half:])}
  assert sorted(got) == sorted(pairs)
  for key, (x, y) in pairs.items():
    want, (b_mmd2, b_kid, b_max) = R.kernel_distance(x, y, subset_size=subset), R.kernel_distance_bound(x, y, subset_size=subset, with_max=True)
    res = got[key]
    print('[latent %s] mmd2 %.6e want %.6e bound %.2e, kid_mean %.6e want %.6e' % (key, res['mmd2'], want['mmd2'], b_mmd2, res['kid_mean'], want['kid_mean']))
    assert sorted(res) == ['kid_mean', 'kid_std', 'm', 'mmd2', 'n', 'num_subsets', 'subset_size']
    assert (res['m'], res['n'], res['num_subsets'], res['subset_size']) == (x.shape[0], y.shape[0], want['num_subsets'], subset)
    assert abs(res['mmd2'] - want['mmd2']) <= b_mmd2 and abs(res['kid_mean'] - want['kid_mean']) <= b_kid
    assert abs(res['kid_std'] - want['kid_std']) <= b_max


def test_evaluate_translation_latent_with_stand_ins():
  from twingan_amd import Config
  from twingan_amd.evaluate import evaluate_translation
  cfg = Config(hw=16, max_ch=8, precision='bf16')
  src, tgt = _images(9100, 64), _images(9150, 64)
  translate_fn, encode_fn, seen = _stand_ins(torch.bfloat16)
  got = evaluate_translation(cfg, None, src, to='t', batch=16, device=DEV, translate_fn=translate_fn, targets=tgt,
                             latent=dict(subset_size=32), encode_fn=encode_fn)
  assert sorted(got) == ['latent', 'ms_ssim_cycle', 'ms_ssim_diversity', 'swd_fake', 'swd_real', 'swd_resolutions']
  assert [dom for dom, _ in seen] == ['s', 't', 't'] * 4
  rows = {name: torch.cat([e for _, e in seen[k::3]]).float().cpu().numpy() for k, name in enumerate(('src', 'fake', 'tgt'))}
  assert rows['tgt'].shape == (64, 128)
  _check_latent(got['latent'], rows, 32)
  assert got['latent']['floor']['num_subsets'] == 1 and got['latent']['domains']['num_subsets'] == 2
  # without latent: key for key what it was, value for value
  plain = evaluate_translation(cfg, None, src, to='t', batch=16, device=DEV, translate_fn=translate_fn, targets=tgt)
  assert sorted(plain) == ['ms_ssim_cycle', 'ms_ssim_diversity', 'swd_fake', 'swd_real', 'swd_resolutions']
  assert all(plain[k] == got[k] for k in plain)
  assert sorted(evaluate_translation(cfg, None, src, batch=16, device=DEV, translate_fn=translate_fn)) == ['ms_ssim_cycle', 'ms_ssim_diversity']
  with pytest.raises(ValueError, match='targets'):
    evaluate_translation(cfg, None, src, batch=16, device=DEV, translate_fn=translate_fn, latent=True)


def test_evaluate_translation_latent_with_the_models_encoder():
  """The tiny stage of tests/golden/infer_hw16_c8_instance_norm (D = 16 * 8 = 128): the three dicts equal the restatement
  applied to the rows embed.ContentEncoder gives for the same images and twingan.translate's translations."""
  from twingan_amd import Config
  from twingan_amd.embed import ContentEncoder
  from twingan_amd.evaluate import evaluate_translation
  from twingan_amd.twingan import translate
  g = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'infer_hw16_c8_instance_norm.npz')))
  sd = {k[len('param/'):]: torch.from_numpy(v).float() for k, v in g.items() if k.startswith('param/')}
  cfg = Config(hw=16, max_ch=8, precision='fp32', generator_norm_type='instance_norm')
  src, tgt = _images(9200, 64), _images(9250, 64)
  got = evaluate_translation(cfg, sd, src, to='t', batch=16, device=DEV, targets=tgt, latent=dict(subset_size=32))
  plain = evaluate_translation(cfg, sd, src, to='t', batch=16, device=DEV, targets=tgt)
  assert sorted(got) == sorted(list(plain) + ['latent']) and all(plain[k] == got[k] for k in plain)
  enc = ContentEncoder(cfg, sd, DEV)
  rows = {'src': [], 'fake': [], 'tgt': []}
  with torch.cuda.device(enc.device), torch.no_grad():
    for i in range(0, 64, 16):
      x = torch.from_numpy(src[i:i + 16]).to(DEV).contiguous()
      t = torch.from_numpy(tgt[i:i + 16]).to(DEV).contiguous()
      y = translate(enc.store.P, x, cfg, 't', None).detach()
      for name, (img, dom) in (('src', (x, 's')), ('fake', (y, 't')), ('tgt', (t, 't'))):
        rows[name].append(enc.encode(img, dom).float().cpu().numpy())
  rows = {k: np.concatenate(v) for k, v in rows.items()}
  assert rows['src'].shape == (64, enc.dim) == (64, 128)
  _check_latent(got['latent'], rows, 32)
