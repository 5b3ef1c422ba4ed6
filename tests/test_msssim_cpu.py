"""CPU checks of the MS-SSIM test infrastructure (tests/msssim_np.py) against tests/golden/msssim_cases.npz, which
tools/make_msssim_golden.py recorded from the reference's own libs/ms_ssim.py: the seeded input generator still produces the
inputs the reference was fed, and the float64 restatement of the formulas -- the yardstick of tests/test_gpu_metrics.py --
reproduces what the reference returned.  Where the reference checkout and SciPy are at hand the fixture is re-derived live."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import msssim_np as M      # noqa: E402

GOLD = M.load_golden()
# the restatement sums in float64, the reference in float32 maps behind an FFT: textured pairs agree to 1e-8 ... 2e-6, the
# near-flat pair (variances ~1e-6 of the squares they are differences of) to 5.9e-6 at its worst shape; the bound below is
# float32's: eps * max_val^2 / c2 = 1.2e-7 * 65025 / 58.5 = 1.3e-4 is what ONE map value can be off by
TOL = 1.3e-4


def test_fixture_covers_the_case_table():
  assert sorted(GOLD) == sorted(c['name'] for c in M.CASES)
  assert os.path.getsize(M.GOLDEN) < 256 * 1024


@pytest.mark.parametrize('shape', M.SHAPES, ids=lambda s: '%dx%d' % s)
def test_input_generator_reproduces_recorded_checksums(shape):
  for case in M.CASES:
    if (case['h'], case['w']) == shape or (shape == M.SHAPES[0] and (case['h'], case['w']) not in M.SHAPES):
      d1, d2 = M.case_inputs(case)
      assert (M.checksum(d1), M.checksum(d2)) == (GOLD[case['name']]['crc1'], GOLD[case['name']]['crc2']), case['name']


def _check(case, ref):
  d1, d2 = M.case_inputs(case)
  x1, x2 = M.metric_inputs(case, d1, d2)
  score, ssim, cs = M.msssim_tables(x1, x2, weights=case['weights'])
  assert np.abs(ssim - ref['ssim']).max() <= TOL, (case['name'], np.abs(ssim - ref['ssim']).max())
  assert np.abs(cs - ref['cs']).max() <= TOL, (case['name'], np.abs(cs - ref['cs']).max())
  if case['family'] in M.SCORE_COMPARED:      # elsewhere a clipped factor turns a sign flip at 1e-7 into 0.5 (x^0.0448)
    factors = np.concatenate([np.clip(ref['cs'][:-1], 0, None).ravel(), np.clip(ref['ssim'][-1], 0, None).ravel()])
    assert factors.min() > 0.1, (case['name'], factors.min())
    assert np.abs(score - ref['score']).max() <= TOL, (case['name'], np.abs(score - ref['score']).max())
    assert abs(score.mean() - ref['mean']) <= TOL
  if case['family'] == 'same':
    assert np.all(score == 1.0) and np.all(ssim == 1.0) and np.all(cs == 1.0)


@pytest.mark.parametrize('shape', M.SHAPES, ids=lambda s: '%dx%d' % s)
def test_float64_restatement_reproduces_fixture(shape):
  for case in M.CASES:
    if (case['h'], case['w']) == shape and case['dtype'] == 'fp32' or \
        (shape == M.SHAPES[0] and (case['h'], case['w']) not in M.SHAPES) or (case['c'] != 3 and case['h'] == shape[0]):
      _check(case, GOLD[case['name']])


def test_float64_restatement_reproduces_fixture_16_bit_inputs():
  for case in M.CASES:
    if case['dtype'] != 'fp32' and case['h'] <= 64:
      _check(case, GOLD[case['name']])


def test_float32_twin_stays_near_float64():
  for name in ('64x64-blend50-fp32-s1', '64x64-flat-fp32-s255'):
    case = M.CASE_BY_NAME[name]
    x1, x2 = M.metric_inputs(case, *M.case_inputs(case))
    a, b = M.msssim_tables(x1, x2), M.msssim_tables(x1, x2, dtype=np.float32)
    for u, v in zip(a, b):
      assert np.abs(u - v).max() <= TOL


def test_restatement_against_reference_live():
  """The fixture re-derived: the reference's module loaded in place and run on a few of the cases."""
  pytest.importorskip('scipy')
  sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
  try:
    import make_msssim_golden as T
  finally:
    sys.path.pop(0)
  try:
    ref = T.load_reference()
  except FileNotFoundError:
    pytest.skip('no reference checkout')
  for name in ('16x16-blend10-fp32-s1', '32x48-noise-bf16-s255', '64x64-flat-fp16-s1', '24x40-levels3-noise-bf16-s255'):
    case = M.CASE_BY_NAME[name]
    x1, x2 = M.metric_inputs(case, *M.case_inputs(case))
    score, ssim, cs, mean = T.reference_tables(ref, x1, x2, weights=case['weights'])
    g = GOLD[name]
    assert np.array_equal(ssim, g['ssim']) and np.array_equal(cs, g['cs']) and np.array_equal(score, g['score'])
    assert mean == g['mean']
