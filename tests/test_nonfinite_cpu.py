"""tests/nonfinite.py on the CPU: the helpers on hand-made arrays (each fault they exist to report IS reported), and every case
of the tables against the three case conditions over the float64 oracle alone -- no kernel runs here."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nonfinite as NF      # noqa: E402

TRIPLES = [t for c in NF.CASES for t in c.triples()]


def test_plant_writes_a_copy():
  x = np.zeros((2, 3), np.float32)
  y = NF.plant(x, (1, 2), 'nan')
  assert np.isnan(y[1, 2]) and np.isfinite(y).sum() == 5 and np.all(x == 0) and y.dtype == np.float32
  z = NF.plant(x.astype(np.float64), [(0, 0), (1, 1)], 'big')
  assert z[0, 0] == z[1, 1] == 60000.0 and z.sum() == 120000.0
  assert NF.plant(x, (0, 1), '-inf')[0, 1] == -np.inf and NF.plant(x, (0, 1), '+inf')[0, 1] == np.inf
  with pytest.raises(AssertionError):
    NF.plant(x, (2, 0), 'nan')
  with pytest.raises(AssertionError):
    NF.plant(x, (0, 0), 'huge')


def test_big_is_finite_in_every_storage_type_and_two_of_them_are_not_in_fp16():
  for d in NF.DNAMES:
    assert np.isfinite(NF.storage_round(NF.BIG, d))
  assert np.isinf(NF.storage_round(2 * NF.BIG, 'f16')) and np.isfinite(NF.storage_round(2 * NF.BIG, 'bf16'))
  assert NF.storage_round(65519.0, 'f16') == 65504.0 and np.isinf(NF.storage_round(65520.0, 'f16'))      # round to nearest even
  assert np.isnan(NF.storage_round(np.nan, 'f16')) and np.isnan(NF.storage_round(np.nan, 'bf16'))


def test_position_pickers():
  s = (3, 5, 7, 3)      # 315 elements
  assert NF.first(s) == (0, 0, 0, 0) and NF.last(s) == (2, 4, 6, 2)
  assert np.ravel_multi_index(NF.last_lane_of_vector(s, 'bf16'), s) == 7 and np.ravel_multi_index(NF.last_lane_of_vector(s, 'f32', 2), s) == 11
  assert np.ravel_multi_index(NF.behind_last_vector(s, 'f16'), s) == 312 and np.ravel_multi_index(NF.behind_last_vector(s, 'f32'), s) == 312
  assert NF.behind_last_vector((2, 8), 'bf16') is None
  # 3 images of 8 x 8: min_ppb 16 -> four blocks of 16 pixels in both passes; the pooled forward walks 16 2x2 blocks in one
  assert NF.norm_chunking(3, 64) == ((4, 16), (4, 16)) and NF.norm_chunking(3, 64, pool=True)[1] == (1, 16)
  assert NF.norm_chunking(1, 512 * 512) == ((1024, 256), (2048, 128)) and NF.norm_chunking(3, 65)[0] == (3, 32)
  assert NF.block_edge_pixels(8, 8, 16) == ((1, 7), (2, 0))
  with pytest.raises(AssertionError):
    NF.block_edge_pixels(4, 4, 16)
  assert NF.last_pixel(8, 6) == (7, 5) and NF.last_image(4) == 3 and NF.first_image_of_second_group(4, 1) == 1
  for h, w, k in ((8, 8, 3), (4, 4, 3), (5, 9, 3)):
    r, c = NF.interior_pixel(h, w, k)
    assert k // 2 <= r < h - k // 2 and k // 2 <= c < w - k // 2
  assert NF.corner_pixel(8, 8) == (0, 0) and NF.border_pixel(8, 8)[0] == 0 and 0 < NF.border_pixel(8, 8)[1] < 7


def _sets():
  ref = np.arange(12, dtype=np.float64).reshape(3, 4)
  ref[1, 2] = np.nan
  taint = ~np.isfinite(ref)
  return ref, taint


def test_a_correct_output_passes_both_routes():
  ref, taint = _sets()
  base = np.where(taint, 6.0, ref)
  NF.assert_propagates_and_contains(ref, base, taint, None, None, 'bit-equal route')
  inf = ref.copy()
  inf[1, 2] = -np.inf      # Inf for NaN: not compared
  NF.assert_propagates_and_contains(inf, None, taint, ref + 1e-9, 1e-6, 'bound route')


def test_a_swallowed_nan_is_reported():
  ref, taint = _sets()
  got = np.where(taint, 0.0, ref)
  with pytest.raises(AssertionError, match=r'1 of 1 taint elements are finite \(swallowed\), first at \(1, 2\)'):
    NF.assert_propagates_and_contains(got, got, taint, None, None, 'swallow')


def test_a_leaked_nan_is_reported():
  ref, taint = _sets()
  got = ref.copy()
  got[2, 3] = np.nan
  with pytest.raises(AssertionError, match=r'1 of 11 clean elements are non-finite \(leaked\), first at \(2, 3\)'):
    NF.assert_propagates_and_contains(got, np.where(taint, 6.0, ref), taint, None, None, 'leak')


def test_a_saturated_65504_in_fp16_is_reported():
  """The fp16 `big` case: the oracle's 120000 is stored as Inf, a store that clamps leaves the largest finite number."""
  sets = NF.expected_sets(lambda inp: dict(y=inp['x'].sum(axis=1)), dict(x=np.array([[NF.BIG, NF.BIG], [1.0, 2.0]])), 'f16')
  assert sets['y'].taint.tolist() == [True, False]
  assert not NF.expected_sets(lambda inp: dict(y=inp['x'].sum(axis=1)), dict(x=np.array([[NF.BIG, NF.BIG], [1.0, 2.0]])), 'bf16')['y'].taint.any()
  with pytest.raises(AssertionError, match='swallowed.*65504: a saturating store'):
    NF.assert_propagates_and_contains(np.array([65504.0, 3.0]), np.array([5.0, 3.0]), sets['y'].taint, None, None, 'saturate')
  NF.assert_propagates_and_contains(np.array([np.inf, 3.0]), np.array([5.0, 3.0]), sets['y'].taint, None, None, 'overflow')


def test_a_moved_bit_and_a_value_outside_its_bound_are_reported():
  ref, taint = _sets()
  base = np.where(taint, 6.0, ref)
  got = ref.copy()
  got[0, 0] = -0.0      # equal as a value, another bit pattern
  with pytest.raises(AssertionError, match=r'1 clean elements differ in bits from the unplanted launch, first at \(0, 0\)'):
    NF.assert_propagates_and_contains(got, base, taint, None, None, 'bits')
  got = ref.copy()
  got[2, 0] += 1e-3
  with pytest.raises(AssertionError, match=r'1 of 11 clean elements outside their bound, first at \(2, 0\)'):
    NF.assert_propagates_and_contains(got, None, taint, ref, 1e-6, 'bound')
  # a touched element is excused from bit-equality and held to the bound instead
  touched = np.zeros(taint.shape, bool)
  touched[2, 0] = True
  NF.assert_propagates_and_contains(got, base, taint, ref, 2e-3, 'touched', touched=touched)
  with pytest.raises(AssertionError, match='outside their bound'):
    NF.assert_propagates_and_contains(got, base, taint, ref, 1e-6, 'touched', touched=touched)
  with pytest.raises(AssertionError, match='need the oracle and its bound'):
    NF.assert_propagates_and_contains(got, None, taint, None, None, 'no bound given')


def test_cases_that_check_nothing_are_refused():
  t = np.zeros((3, 4), bool)
  mk = lambda taint: dict(y=NF.Sets(np.zeros(taint.shape), taint, np.zeros(taint.shape, bool)))
  with pytest.raises(AssertionError, match='no propagation'):
    NF.check_case(mk(t))
  with pytest.raises(AssertionError, match='clean set is empty'):
    NF.check_case(mk(~t))
  half = t.copy()
  half[:, :3] = True
  with pytest.raises(AssertionError, match='more than half'):
    NF.check_case(mk(half))
  col = t.copy()
  col[:, 0] = True      # every row holds a taint element: no whole clean unit along axis 0 ...
  with pytest.raises(AssertionError, match='no output keeps one whole clean unit'):
    NF.check_case(mk(col))
  assert NF.check_case(mk(col), units=dict(y=1)) == (3, 12)      # ... but three whole clean columns
  row = t.copy()
  row[1] = True
  assert NF.check_case(mk(row)) == (4, 12)


def test_case_ids_are_unique():
  ids = [c.id for c in NF.CASES]
  assert len(set(ids)) == len(ids), sorted(i for i in ids if ids.count(i) > 1)


@pytest.mark.parametrize('case,dname,what', TRIPLES, ids=['%s-%s-%s' % (c.id, d, w) for c, d, w in TRIPLES])
def test_every_case_meets_the_case_conditions_over_the_oracle_alone(case, dname, what):
  """taint and clean non-empty, one whole clean unit, taint at most half -- and the inputs as the kernels will get them: finite
  but for the plants, the plants where the table says."""
  inputs = case.make(dname)
  assert all(np.all(np.isfinite(v)) for v in inputs.values())
  planted = case.planted(inputs, dname, what)
  nplanted = sum(int((planted[k] != inputs[k]).sum()) for k in inputs)
  assert nplanted == sum(1 for _, idx in case.plants(inputs, dname) if idx is not None)
  sets = case.expected(inputs, planted, dname)
  nt, total = NF.check_case(sets, case.units)
  print('[case] %s %s %s: taint %d of %d, touched %d' % (case.id, dname, what, nt, total, sum(int(s.touched.sum()) for s in sets.values())))
  if any(s.touched.any() for s in sets.values()) or case.atomic:
    assert case.bound is not None, 'elements on the bound route need the bound of their family'
    b = case.bound(planted, sets, dname)
    for name, s in sets.items():
      need = s.touched | (s.clean if name in case.atomic else False)
      bb = np.broadcast_to(np.asarray(b[name], np.float64), s.ref.shape)
      assert np.all(np.isfinite(bb[need])) and np.all(bb[need] > 0), (name, 'the bound of an element on the bound route is not finite / positive')
