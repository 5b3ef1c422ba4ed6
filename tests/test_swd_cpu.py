"""CPU checks of the sliced Wasserstein test infrastructure (tests/swd_np.py: the float64 restatement the GPU tests hold the
kernels to).  No reference code exists to compare it with (image_generation.py:926-931), so the restatement is pinned by
properties that any correct statement of the algorithm has, and the kernels' own source is run over the emulation
(tests/hipemu) on the cases of tests/test_gpu_swd.py that are small enough for it."""
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import swd_np as S      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_summing_the_pyramid_back_up_recovers_the_image():
  for hw in (16, 32, 64):
    v = S.pixels(S.images(100 + hw, 2, hw), quantize=False).astype(np.float64)
    pyr = S.pyramid(v)
    assert [p.shape[1] for p in pyr] == S.resolutions(hw)
    assert np.abs(S.reconstruct(pyr) - v).max() <= 1e-9
  flat = S.pyramid(np.full((1, 64, 64, 3), 93.0))      # the filters keep a constant: band-pass levels vanish, borders included
  assert all(np.abs(p).max() <= 1e-12 for p in flat[:-1]) and np.abs(flat[-1] - 93.0).max() <= 1e-12


def test_polyphase_border_formulas_equal_literal_zero_insertion():
  rs = np.random.RandomState(1)
  for h in (2, 3, 16, 17):
    x = rs.randn(1, h, h, 3)
    want = S.up(x)
    rows = S.up_axis_polyphase(x[0])                                              # axis 0 of [h, w, c]
    got = S.up_axis_polyphase(rows.transpose(1, 0, 2)).transpose(1, 0, 2)      # then axis 1
    assert np.abs(got - want[0]).max() <= 1e-14, h
  x = np.arange(1., 6.)[None, :, None, None] * np.ones((1, 5, 5, 1))
  col = S.up(x)[0, :, 0, 0]
  assert np.allclose(col[[0, 8, 9]], [(6 * 1 + 2 * 2) / 8, (4 + 7 * 5) / 8, 5.0])      # the two borders differ


def test_identical_descriptor_sets_give_exactly_zero():
  d, dirs = S.dc_offset_set(2, 64), S.directions(3, 2, 8)
  assert S.distance(d, d.copy(), dirs)[0] == 0.0
  assert S.distance(d, d.copy(), dirs, np.float32)[0] == 0.0


def test_one_direction_one_channel_by_hand():
  rs = np.random.RandomState(4)
  a, b = np.zeros((40, S.K), np.float32), np.zeros((40, S.K), np.float32)
  a[:, :49], b[:, :49] = rs.randn(40, 49) * 3 + 10, rs.randn(40, 49) * 5 - 2
  dirs = np.zeros((1, S.K, 1), np.float32)
  dirs[0, 7, 0] = 1.0      # picks value 7 of channel 0; the flat channels 1 and 2 normalise to 0 (no NaN)

  def column(x):
    v = x[:, :49].astype(np.float64)
    return np.sort((v[:, 7] - v.mean()) / v.std())
  want = np.abs(column(a) - column(b)).mean()
  got, per = S.distance(a, b, dirs)
  assert np.isfinite(got) and abs(got - want) <= 1e-12 and per.shape == (1,)


def test_a_per_channel_affine_change_of_one_set_changes_nothing():
  a, b, dirs = S.dc_offset_set(5, 96), S.dc_offset_set(6, 96, mean=90., sigma=12.), S.directions(7, 2, 8)
  scale, shift = np.repeat([2.0, 0.5, 7.0], 49), np.repeat([-30.0, 4.0, 100.0], 49)
  moved = a.astype(np.float64) * scale + shift
  assert abs(S.distance(moved, b, dirs)[0] - S.distance(a, b, dirs)[0]) <= 1e-12


def test_descriptor_layout_and_statistics():
  level = np.arange(2 * 16 * 16 * 3, dtype=np.float64).reshape(2, 16, 16, 3)
  d = S.descriptors(level, np.array([[3, 3], [12, 5], [7, 7]]), per=2)      # rows 0, 1: image 0; row 2: image 1
  assert d.shape == (3, S.K)
  assert d[1, 2 * 49 + 6 * 7 + 0] == level[0, 12 + 3, 5 - 3, 2] and d[2, 0] == level[1, 4, 4, 0]
  mean, rstd = S.statistics(S.flat_channel_set(8, 10))
  assert rstd[1] == 0.0 and mean[1] == 37.25 and np.all(S.normalise(S.flat_channel_set(8, 10))[:, 49:98] == 0.0)


def test_write_swd_result_has_the_reference_layout(tmp_path):
  from twingan_amd.evaluate import write_swd_result
  res = {'resolutions': [32, 16], 'real': [1.5, 2.25], 'fake': [10.0, 20.5], 'average': (1.875, 15.25)}
  path = str(tmp_path / 'swd_eval_step_0_1024_images.txt')
  write_swd_result(path, res, 1024)
  assert open(path).read() == ('swd sliced wasserstein score evaluated on 1024 images.\n'
                               'res\treal\tfake\n'
                               '32\t1.500000\t10.000000\n'
                               '16\t2.250000\t20.500000\n'
                               'Average\t1.875000\t15.250000\n')


def test_swd_gpu_cases_pass_over_the_emulated_kernels():
  """The kernels' own source on the host: every case of tests/test_gpu_swd.py but the two that run the whole model."""
  env = dict(os.environ, TG_EMU='1')
  env.pop('TG_LIB_PATH', None)
  r = subprocess.run([sys.executable, '-m', 'pytest', '-m', 'gpu', '-q', '-x', '-p', 'no:cacheprovider', '--tb=short',
                      'tests/test_gpu_swd.py', '-k', 'not evaluate_translation'],
                     cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
  assert r.returncode == 0, r.stdout[-3000:]
  assert ' passed' in r.stdout and 'skipped' not in r.stdout.splitlines()[-1], r.stdout[-500:]
