"""CPU: the kernel two-sample distance's host side.  The guarantees of include/twingan_hip_mmd.h (exactly the documented
functions declared, bound one to one by _lib.MMD_SIGNATURES, exported by the built library and by the emulated one, the five
older tables still equal to their headers), the restatement tests/mmd_ref.py pinned by properties any correct statement of the
estimator has (no reference code exists for it), the host arithmetic of evaluate.KernelDistance.end() on block sums handed
in, the kernels' own source over the emulation on the cases of tests/test_gpu_mmd.py, and where the entry point reads and
writes: tests/hipemu/mmd_bounds_main.cpp, a stand-alone program compiled with AddressSanitizer and linked with the sanitized
emulated kernels, run case by case as child processes.  Nothing sanitized is loaded into python."""
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, 'tests', 'hipemu')
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mmd_ref as R      # noqa: E402

MMD_FUNCTIONS = ['tg_mmd_block_sums', 'tg_mmd_workspace_bytes']


def _emu_build():
  sys.path.insert(0, HERE)
  try:
    import build
  finally:
    sys.path.pop(0)
  return build


# ------------------------------------------------------------------------------------------------ the header
def _header(name):
  return re.sub(r'/\*.*?\*/', ' ', open(os.path.join(ROOT, 'include', name)).read(), flags=re.S)


def _declared(header):
  return sorted(set(re.findall(r'\b(tg_[a-z0-9_]+)\s*\(', _header(header))))


def _exported(lib):
  out = subprocess.run(['nm', '-D', '--defined-only', lib], stdout=subprocess.PIPE, text=True, check=True).stdout
  return {ln.split()[-1] for ln in out.splitlines() if ln.split()}


def test_mmd_header_is_exported_and_bound():
  from twingan_amd import _lib
  assert _declared('twingan_hip_mmd.h') == MMD_FUNCTIONS
  assert sorted(_lib.MMD_SIGNATURES) == MMD_FUNCTIONS
  if not os.path.exists(_lib.LIB_PATH):
    pytest.fail('%s is not built (build() compiles it)' % _lib.LIB_PATH)
  missing = [f for f in MMD_FUNCTIONS if f not in _exported(_lib.LIB_PATH)]
  assert not missing, missing
  # six disjoint tables, the five older ones still their headers
  older = {'twingan_hip.h': _lib.SIGNATURES, 'twingan_hip_optim.h': _lib.OPTIM_SIGNATURES, 'twingan_hip_summary.h': _lib.SUMMARY_SIGNATURES,
           'twingan_hip_knn.h': _lib.KNN_SIGNATURES, 'twingan_hip_syncnorm.h': _lib.SYNCNORM_SIGNATURES}
  for header, table in older.items():
    assert sorted(table) == _declared(header), header
    assert not set(table) & set(_lib.MMD_SIGNATURES), header
  assert sorted(f for f in os.listdir(os.path.join(ROOT, 'include')) if f.endswith('.h')) == sorted(list(older) + ['twingan_hip_mmd.h'])
  # argument counts and the constant follow the header
  text = _header('twingan_hip_mmd.h')
  for name, (_, args) in _lib.MMD_SIGNATURES.items():
    params = re.search(r'\b%s\s*\(([^)]*)\)' % name, text).group(1)
    assert len(args) == len([p for p in params.split(',') if p.strip()]), name
  consts = {k: int(v) for k, v in re.findall(r'#define (TG_MMD_[A-Z0-9_]+) (\d+)', text)}
  assert consts == {'TG_MMD_MAX_DEGREE': _lib.MMD_MAX_DEGREE} and _lib.MMD_MAX_DEGREE == 4


def test_emulated_library_exports_the_mmd_header():
  lib = _emu_build().build()
  assert not [f for f in MMD_FUNCTIONS if f not in _exported(lib)]


# ------------------------------------------------------------------------------------------------ the restatement
def _draw(seed, m, n, d, shift=0.0):
  rng = np.random.default_rng(seed)
  return rng.standard_normal((m, d)), rng.standard_normal((n, d)) + shift


def test_restatement_block_sums_give_the_double_loop_estimator():
  x, y = _draw(1, 37, 70, 9)
  for kernel in (dict(), dict(degree=2, gamma=0.3, coef0=0.5), dict(degree=1), dict(degree=4, gamma=0.01)):
    direct = R.estimate(R.pair_values(x, x, **kernel), R.pair_values(y, y, **kernel), R.pair_values(x, y, **kernel))
    assert abs(R.estimate_fast(x, y, **kernel) - direct) <= 1e-12 * max(1.0, abs(direct))
    for block in (32, 64):      # short last blocks on both sides
      got = R.kernel_distance(x, y, subset_size=64, block=block, **kernel)
      assert abs(got['mmd2'] - direct) <= 1e-12 * max(1.0, abs(direct)), (kernel, block)
      assert (got['m'], got['n'], got['num_subsets'], got['kid_mean'], got['kid_std']) == (37, 70, 0, None, None)
  # the masks: offsets move the excluded diagonal, and without skip nothing is excluded
  p = R.pair_values(x, y)
  assert R.block_sums(x, y, 32).sum() == pytest.approx(p.sum(), rel=1e-14)
  assert R.block_sums(x, y, 32, a_index0=5, b_index0=2, skip_same_index=True).sum() == pytest.approx(p.sum() - sum(p[i, i + 3] for i in range(37)), rel=1e-13)
  assert R.block_sums(x, y, 32).shape == (2, 3) and R.block_sums(x, y, 64).shape == (1, 2)


def test_restatement_subset_values_are_the_estimator_on_the_sliced_rows():
  x, y = _draw(2, 200, 170, 12)
  got = R.kernel_distance(x, y, subset_size=64, block=32)
  vals = [R.estimate_fast(x[k * 64:(k + 1) * 64], y[k * 64:(k + 1) * 64]) for k in range(2)]
  assert got['num_subsets'] == 2 and got['subset_size'] == 64
  assert abs(got['kid_mean'] - np.mean(vals)) <= 1e-13 and abs(got['kid_std'] - np.std(vals)) <= 1e-13
  one = R.kernel_distance(x[:64], y[:64], subset_size=64, block=64)
  assert one['num_subsets'] == 1 and one['kid_std'] == 0.0 and abs(one['kid_mean'] - vals[0]) <= 1e-13 and abs(one['mmd2'] - vals[0]) <= 1e-13


def test_restatement_a_set_against_a_copy_of_itself_is_the_closed_form():
  """X against X: sum_XY = sum_{i != j} k + sum_i k(x_i, x_i), so
  mmd2 = 2 S / (m (m - 1)) - 2 (S + T) / m^2 = 2 (S / (m - 1) - T) / m^2, S the off-diagonal sum and T the trace."""
  x, _ = _draw(3, 96, 1, 7)
  k = R.pair_values(x, x)
  T = np.trace(k)
  S = k.sum() - T
  want = 2.0 * (S / 95 - T) / 96 ** 2
  got = R.kernel_distance(x, x.copy(), subset_size=32)
  assert abs(got['mmd2'] - want) <= 1e-12 * abs(want) and got['mmd2'] < 0      # the diagonal dominates: below zero
  assert got['num_subsets'] == 3


def test_restatement_separates_a_shifted_distribution_from_a_second_sample():
  """Seeded, fixed draws: two samples of one distribution sit within a few kid_std of 0, a shifted one well above."""
  x, y = _draw(4, 1024, 1024, 32)
  same = R.kernel_distance(x, y, subset_size=128)
  assert same['num_subsets'] == 8 and abs(same['kid_mean']) <= 3 * same['kid_std'] / np.sqrt(8) + 1e-4
  assert abs(same['mmd2']) <= abs(same['kid_mean']) + 3 * same['kid_std']
  _, z = _draw(4, 1024, 1024, 32, shift=0.5)
  apart = R.kernel_distance(x, z, subset_size=128)
  assert apart['kid_mean'] > 10 * apart['kid_std'] and apart['kid_mean'] > 50 * abs(same['kid_mean']) and apart['mmd2'] > 0.5 * apart['kid_mean']


def test_restatement_fp32_steps_and_bound():
  a = np.array([[1.0, -1.0, 0.0, 1.0]])
  b = np.array([[1.0, 1.0, 1.0, 1.0], [0.0, 0.0, 0.0, 0.0]])
  p = R.pair_values(a, b, degree=3, gamma=0.25, coef0=1.0, fp32_steps=True)
  assert p.tolist() == [[1.25 ** 3, 1.0]]
  t = np.float32(1.0) + np.float32(267.0 / 256.0 - 1.0)      # 267 / 256: its cube needs 25 bits
  want = float(np.float32(np.float32(t * t) * t))
  got = R.pair_values(np.full((1, 256), 1.0), np.r_[np.ones(11), np.zeros(245)][None, :], degree=3, fp32_steps=True)[0, 0]
  assert got == want and got != (267.0 / 256.0) ** 3
  with pytest.raises(AssertionError):
    R.pair_values(np.array([[1.0]]), np.array([[1.0]]), gamma=0.1, fp32_steps=True)
  bound = R.block_sum_bound(a, b, 32, degree=1, gamma=0.25, coef0=1.0)
  e_s = 4 * R.U * np.array([3.0, 0.0])
  e_t = 0.25 * e_s + R.U * (np.array([1.25, 1.0]) + 0.25 * e_s)
  assert bound.shape == (1, 1) and abs(bound[0, 0] - (e_t.sum() + 2.0 ** -50 * (np.array([1.25, 1.0]) + e_t).sum())) <= 1e-20


# ------------------------------------------------------------------------------------------------ KernelDistance.end()
def test_kernel_distance_host_arithmetic_on_known_block_sums():
  from twingan_amd.evaluate import KernelDistance, kernel_distance_from_sums
  # m = 70, n = 100 in blocks of 32: 3 and 4 blocks, the last ones short; subsets of 32: two
  xx, yy, xy = np.arange(9.0).reshape(3, 3) + 1, np.arange(16.0).reshape(4, 4) * 2, np.arange(12.0).reshape(3, 4) - 3
  got = kernel_distance_from_sums(xx, yy, xy, 70, 100, 32, 32)
  assert got['mmd2'] == xx.sum() / (70 * 69) + yy.sum() / (100 * 99) - 2 * xy.sum() / (70 * 100)
  vals = [xx[k, k] / (32 * 31) + yy[k, k] / (32 * 31) - 2 * xy[k, k] / (32 * 32) for k in range(2)]
  assert got['num_subsets'] == 2 and got['kid_mean'] == np.mean(vals) and got['kid_std'] == np.std(vals)
  assert sorted(got) == ['kid_mean', 'kid_std', 'm', 'mmd2', 'n', 'num_subsets', 'subset_size'] and (got['m'], got['n'], got['subset_size']) == (70, 100, 32)
  assert got == R.from_sums(xx, yy, xy, 70, 100, 32, 32)
  # subsets of 64 = two blocks a side: one subset, the 2 x 2 corner
  got = kernel_distance_from_sums(xx, yy, xy, 70, 100, 32, 64)
  assert got['num_subsets'] == 1 and got['kid_std'] == 0.0
  assert got['kid_mean'] == xx[:2, :2].sum() / (64 * 63) + yy[:2, :2].sum() / (64 * 63) - 2 * xy[:2, :2].sum() / (64 * 64)
  # fewer rows than a subset on one side
  got = kernel_distance_from_sums(xx[:1, :1], yy, xy[:1], 20, 100, 32, 32)
  assert (got['num_subsets'], got['kid_mean'], got['kid_std']) == (0, None, None) and got['mmd2'] == 1.0 / (20 * 19) + yy.sum() / 9900 - 2 * xy[0].sum() / 2000
  # refusals
  for args, text in (((xx[:1, :1], yy, xy[:1], 1, 100, 32, 32), 'at least 2 rows'), ((xx, yy[:1, :1], xy[:, :1], 70, 1, 32, 32), 'at least 2 rows'),
                     ((xx, yy, xy, 70, 100, 32, 48), 'multiple'), ((xx, yy, xy, 70, 100, 48, 96), 'multiple'), ((xx, yy, xy, 70, 100, 32, 16), 'multiple'),
                     ((xx, yy, xy, 170, 100, 32, 32), 'do not belong'), ((xx, yy, xy.T, 70, 100, 32, 32), 'do not belong')):
    with pytest.raises(ValueError, match=text):
      kernel_distance_from_sums(*args)
  for kw, text in ((dict(subset_size=48), 'multiple'), (dict(block=16, subset_size=64), 'multiple'), (dict(degree=5), 'degree'), (dict(degree=0), 'degree')):
    with pytest.raises(ValueError, match=text):
      KernelDistance(8, 64, **kw)
  with pytest.raises(ValueError, match='capacity'):
    KernelDistance(8, 1)


# ------------------------------------------------------------------------------------------------ the emulated kernels
def test_mmd_gpu_cases_pass_over_the_emulated_kernels():
  """The kernels' own source on the host: the cases of tests/test_gpu_mmd.py but those that only cost time there -- the
  full-width one (4 G multiply-adds a launch through the emulated MFMA), the two largest of the other shapes, whose paths the
  smaller ones take too, and evaluate_translation (the model and the SWD kernels, which have emulated runs of their own)."""
  env = dict(os.environ, TG_EMU='1')
  env.pop('TG_LIB_PATH', None)
  r = subprocess.run([sys.executable, '-m', 'pytest', '-m', 'gpu', '-q', '-x', '-p', 'no:cacheprovider', '--tb=short',
                      'tests/test_gpu_mmd.py', '-k', 'not full_width and not evaluate_translation and not d1031 and not n1000-256'],
                     cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
  assert r.returncode == 0, r.stdout[-3000:]
  assert ' passed' in r.stdout and 'skipped' not in r.stdout.splitlines()[-1], r.stdout[-500:]


# ------------------------------------------------------------------------------------------------ bounds
WORKERS = 16
CASE_TIMEOUT = 120


def _build_driver():
  """Compiles mmd_bounds_main.cpp with the flags of build_bounds() and links it with that build's objects but bounds_main.o."""
  build = _emu_build()
  build.build_bounds()
  src = os.path.join(HERE, 'mmd_bounds_main.cpp')
  obj = os.path.join(build.OUT_ASAN, 'mmd_bounds_main.o')
  exe = os.path.join(build.OUT_ASAN, 'mmd_bounds')
  objs = [os.path.join(build.OUT_ASAN, n + '.o') for n in build.SOURCES + ['emu']]
  deps = [src, os.path.join(ROOT, 'include', 'twingan_hip_mmd.h'), os.path.join(ROOT, 'include', 'twingan_hip.h')]
  if build.stale(obj, deps):
    subprocess.check_call([build.CXX] + build.FLAGS + build.ASAN_FLAGS + ['-c', src, '-o', obj])
  if build.stale(exe, [obj] + objs):
    tmp = exe + '.tmp%d' % os.getpid()
    subprocess.check_call([build.CXX] + build.ASAN_FLAGS + [obj] + objs + ['-ldl', '-o', tmp])
    os.replace(tmp, exe)
  return exe


def _run_case(binary, name):
  try:
    r = subprocess.run([binary, '--case', name], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=CASE_TIMEOUT,
                       env=dict(os.environ, ASAN_OPTIONS='detect_leaks=0:abort_on_error=0'))
    return name, r.returncode, r.stdout, r.stderr
  except subprocess.TimeoutExpired:
    return name, -1, '', 'FAIL %s: no result within %d s' % (name, CASE_TIMEOUT)


@pytest.fixture(scope='module')
def driver():
  binary = _build_driver()
  names = subprocess.run([binary, '--list'], stdout=subprocess.PIPE, text=True, check=True).stdout.split()
  with ThreadPoolExecutor(max_workers=WORKERS) as ex:
    results = list(ex.map(lambda n: _run_case(binary, n), names))
  return names, results


def test_mmd_bounds_cases_run_clean_under_the_sanitizer(driver):
  names, results = driver
  dts = ('f32', 'bf16', 'f16')
  shapes = ('m1_n1_d1_b32_p1', 'm3_n5_d16_b32_p2', 'm33_n257_d24_b32_p3', 'm70_n300_d27_b64_p4', 'm70_n333_d40_b128_p3')
  want = {'tg_mmd_block_sums_%s_%s_%s' % (d, s, o) for d in dts for s in shapes for o in 'ao'}
  want |= {'tg_mmd_block_sums_%s_self' % d for d in dts} | {'tg_mmd_block_sums_refusals'}
  assert set(names) == want and len(names) == len(want) == 34
  bad = [(n, rc, (err + out)[-1500:]) for n, rc, out, err in results if rc != 0 or ('ok ' + n) not in out]
  assert not bad, '\n\n'.join('%s (exit %s)\n%s' % b for b in bad[:6])


def test_every_function_of_the_mmd_header_has_a_case(driver):
  names, _ = driver
  src = re.sub(r'//[^\n]*', ' ', open(os.path.join(HERE, 'mmd_bounds_main.cpp')).read())
  called = set(re.findall(r'\b(tg_[a-z0-9_]+)\s*\(', src))
  sized = {'tg_mmd_workspace_bytes': 'tg_mmd_block_sums'}      # the size query is exercised by the case of what it sizes
  for f in MMD_FUNCTIONS:
    assert f in called, f
    assert any(n.startswith(sized.get(f, f) + '_') for n in names), f
