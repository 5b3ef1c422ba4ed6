"""MS-SSIM on the GPU (ops.msssim: the fused per-level HIP kernel; twingan_amd/evaluate.py) against the reference's own
numbers (tests/golden/msssim_cases.npz, recorded from libs/ms_ssim.py by tools/make_msssim_golden.py) and the float64
restatement of its formulas (tests/msssim_np.py).

What is compared, and how tightly.  The per-level tables ssim[L, B] and cs[L, B] in every case, absolutely; the final score
where the clip at 0 does not bite (every clipped per-image factor of the case > 0.1 in the reference: all families but the
unrelated textures, and the test asserts that it holds).  The bound is not a constant: per case and per quantity,
  4 * max(|float32 restatement - float64|, |reference - float64|) + 1e-6
around the float64 value -- the factor 4 for a third float32 summation order (tiles, separable passes) next to the two
measured ones, 1e-6 = 16 ulp of fp32 at 1.0 so that the bound stays finite where both distances are 0."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import msssim_np as M      # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = M.load_golden()
TORCH_DT = {'fp32': torch.float32, 'bf16': torch.bfloat16, 'fp16': torch.float16}
DEV = 'cuda:0'
worst_ratio = {}      # dtype -> worst |kernel - f64| / bound seen (printed by the last test; the figures of DESIGN.md §4)


def _dev(x, dtype):
  return torch.from_numpy(np.ascontiguousarray(x)).to(DEV).to(TORCH_DT[dtype]).contiguous()


def _bounds(x1, x2, weights, ref=None):
  """-> {quantity: (float64 value, bound)} for the metric inputs x1, x2 (float32 arrays)."""
  e = dict(zip(('score', 'ssim', 'cs'), M.msssim_tables(x1, x2, weights=weights)))
  t = dict(zip(('score', 'ssim', 'cs'), M.msssim_tables(x1, x2, weights=weights, dtype=np.float32)))
  out = {}
  for k in e:
    d = np.abs(t[k] - e[k]).max()
    if ref is not None:
      d = max(d, np.abs(ref[k] - e[k]).max())
    out[k] = (e[k], 4.0 * d + 1e-6)
  return out


@pytest.mark.parametrize('name', [c['name'] for c in M.CASES])
def test_msssim_matches_reference(name):
  from twingan_amd import ops
  case, ref = M.CASE_BY_NAME[name], GOLD[name]
  d1, d2 = M.case_inputs(case)
  assert (M.checksum(d1), M.checksum(d2)) == (ref['crc1'], ref['crc2'])
  x1, x2 = M.metric_inputs(case, d1, d2)
  bounds = _bounds(x1, x2, case['weights'], ref)
  score, ssim, cs = ops.msssim(_dev(d1, case['dtype']), _dev(d2, case['dtype']), max_val=255., scale=case['scale'],
                               weights=case['weights'])
  got = dict(score=score.cpu().double().numpy(), ssim=ssim.cpu().double().numpy(), cs=cs.cpu().double().numpy())
  assert got['ssim'].shape == ref['ssim'].shape and got['score'].shape == (case['b'],)
  compared = ['ssim', 'cs']
  if case['family'] in M.SCORE_COMPARED:
    factors = np.concatenate([np.clip(ref['cs'][:-1], 0, None).ravel(), np.clip(ref['ssim'][-1], 0, None).ravel()])
    assert factors.min() > 0.1, factors.min()
    compared.append('score')
  else:      # the clip / no-NaN case: finite, and the product formula of the kernel's OWN tables (fp32 powf: a few ulp)
    assert np.isfinite(got['score']).all()
    own = M.score_from_tables(got['ssim'], got['cs'], case['weights'] or M.WEIGHTS)
    assert np.abs(got['score'] - own).max() <= 2e-6, np.abs(got['score'] - own).max()
  for k in compared:
    want, bound = bounds[k]
    err = np.abs(got[k] - want).max()
    print('%s %s: |kernel - f64| %.3e  bound %.3e  ratio %.3f' % (name, k, err, bound, err / bound))
    worst_ratio[case['dtype']] = max(worst_ratio.get(case['dtype'], 0.0), err / bound)
    assert err <= bound, (k, err, bound)
  if case['family'] == 'same':
    assert np.all(got['score'] == 1.0)


def _batch(seed, n, hw, families):
  a, b = zip(*[M.make_pair(seed + i, hw, hw, 3, families[i % len(families)]) for i in range(n)])
  return np.stack(a).astype(np.float32), np.stack(b).astype(np.float32)


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_msssim_is_bit_reproducible_and_batch_independent(dtype):
  from twingan_amd import ops
  a, b = _batch(7000, 5, 64, ('blend50', 'noise', 'roll', 'unrelated', 'flat'))
  da, db = _dev(a, dtype), _dev(b, dtype)
  first = [t.cpu() for t in ops.msssim(da, db, scale=255.)]
  again = [t.cpu() for t in ops.msssim(da, db, scale=255.)]
  for u, v in zip(first, again):
    assert torch.equal(u, v)
  for i in range(5):
    s, ss, cs = ops.msssim(da[i:i + 1].contiguous(), db[i:i + 1].contiguous(), scale=255.)
    assert torch.equal(s.cpu(), first[0][i:i + 1]) and torch.equal(ss.cpu(), first[1][:, i:i + 1])
    assert torch.equal(cs.cpu(), first[2][:, i:i + 1])


def test_msssim_accumulator_over_three_minibatches():
  from twingan_amd.evaluate import MsSsim
  acc = MsSsim(scale=255.)
  acc.begin()
  want, want32 = [], []
  for k, n in enumerate((4, 6, 2)):
    a, b = _batch(7100 + 10 * k, n // 2, 32, ('blend10', 'noise', 'roll'))
    mb = np.empty((n,) + a.shape[1:], np.float32)
    mb[0::2], mb[1::2] = a, b
    acc.feed(_dev(mb, 'fp32'))
    x1, x2 = a * np.float32(255.), b * np.float32(255.)
    want.append(M.msssim_tables(x1, x2)[0])
    want32.append(M.msssim_tables(x1, x2, dtype=np.float32)[0])
  want, want32 = np.concatenate(want), np.concatenate(want32)
  assert acc.num_pairs == 6
  got = acc.end()
  bound = 4.0 * np.abs(want32 - want).max() + 1e-6
  assert abs(got - want.mean()) <= bound, (got, want.mean(), bound)


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_evaluate_translation(precision):
  """Both metrics of a stage at the size of tests/golden/infer_hw16_c8_*: equal to the restatement applied to the very images
  twingan.translate produced (the model's dtype, scale 255)."""
  from twingan_amd import Config
  from twingan_amd.evaluate import evaluate_translation
  from twingan_amd.inference import ImageInferer
  from twingan_amd.twingan import translate
  g = dict(np.load(os.path.join(os.path.dirname(M.GOLDEN), 'infer_hw16_c8_instance_norm.npz')))
  sd = {k[len('param/'):]: torch.from_numpy(v).float() for k, v in g.items() if k.startswith('param/')}
  cfg = Config(hw=16, max_ch=8, precision=precision, generator_norm_type='instance_norm')
  src = np.stack([M.texture(np.random.RandomState(7200 + i), 16, 16, 3) for i in range(8)]).astype(np.float32)
  got = evaluate_translation(cfg, sd, src, to='t', batch=4, device=DEV)
  assert sorted(got) == ['ms_ssim_cycle', 'ms_ssim_diversity']

  inf = ImageInferer(cfg, sd, device=DEV)
  x = _dev(src, precision)
  with torch.cuda.device(inf.device):
    y = torch.cat([translate(inf.store.P, x[i:i + 4].contiguous(), cfg, 't', None) for i in (0, 4)])
    back = torch.cat([translate(inf.store.P, y[i:i + 4].contiguous(), cfg, 's', None) for i in (0, 4)])
  f = lambda t: t.float().cpu().numpy() * np.float32(255.)      # noqa: E731  (what the kernel forms on load)
  for key, (p, q) in (('ms_ssim_diversity', (f(y)[0::2], f(y)[1::2])), ('ms_ssim_cycle', (f(x), f(back)))):
    want = M.msssim_tables(p, q)[0]
    want32 = M.msssim_tables(p, q, dtype=np.float32)[0]
    bound = 4.0 * np.abs(want32 - want).max() + 1e-6
    print('%s %s: got %.9f want %.9f bound %.3e' % (precision, key, got[key], want.mean(), bound))
    assert abs(got[key] - want.mean()) <= bound, (key, got[key], want.mean(), bound)


def test_cycle_score_of_an_identity_stand_in_is_exactly_one():
  from twingan_amd import Config
  from twingan_amd.evaluate import evaluate_translation
  src = np.stack([M.texture(np.random.RandomState(7300 + i), 16, 16, 3) for i in range(6)]).astype(np.float32)
  got = evaluate_translation(Config(hw=16, max_ch=8, precision='bf16'), None, src, batch=4, device=DEV,
                             translate_fn=lambda x, to: x)
  assert got['ms_ssim_cycle'] == 1.0
  assert 0.0 < got['ms_ssim_diversity'] < 1.0


def test_msssim_errors_are_loud():
  from twingan_amd import ops
  from twingan_amd._lib import TgError
  a = torch.zeros(2, 40, 32, 3, device=DEV)
  with pytest.raises(TgError, match='divisible'):      # 40 = 8 * 5: not divisible by 2^(5-1)
    ops.msssim(a, a)
  ops.msssim(a, a, weights=(0.2, 0.3, 0.2, 0.3))       # ... but by 2^(4-1)
  with pytest.raises(TgError, match='same shape'):
    ops.msssim(a, torch.zeros(2, 32, 32, 3, device=DEV))
  with pytest.raises(TgError, match='1 <= c <= 4'):
    ops.msssim(torch.zeros(1, 16, 16, 5, device=DEV), torch.zeros(1, 16, 16, 5, device=DEV))
  with pytest.raises(TgError, match='dtype'):
    ops.msssim(a.double(), a.double())


def test_report_worst_ratios():
  """Not a check of its own: prints the worst |kernel - f64| / bound per dtype over the parity cases that ran."""
  for dt, r in sorted(worst_ratio.items()):
    print('worst ratio %s: %.3f' % (dt, r))
    assert r <= 1.0
