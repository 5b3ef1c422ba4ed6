"""CPU: the --optimizer rules' float64 reference (tests/optim_ref.py) against torch.optim where the definitions coincide and
against hand-computed steps where they do not; Config's validation; the guarantees of include/twingan_hip_optim.h (every
declared name exported, bound one to one by _lib.OPTIM_SIGNATURES); and where tg_optim_step reads and writes:
tests/hipemu/optim_bounds_main.cpp, a stand-alone program compiled with AddressSanitizer and linked with the sanitized
emulated kernels, run case by case as child processes.  Nothing sanitized is loaded into python."""
import math
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, 'tests', 'hipemu')
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optim_ref as R      # noqa: E402


# ------------------------------------------------------------------------------------------------ the reference
def _run_ref(rule, h, th, grads):
  slots = [x.astype(np.float64) for x in R.slot_init(rule, th.size)]
  for g in grads:
    out, _ = R.step(rule, th, g, slots, h, 1.0, f32_scalars=False)
    th, slots = out[0], out[1:]
  return th


@pytest.mark.parametrize('rule', ['sgd', 'momentum', 'adadelta'])
def test_reference_matches_torch_optim(rule):
  """20 steps on 1000 random elements in float64: 1e-12 relative."""
  gen = torch.Generator().manual_seed(3)
  th0 = torch.randn(1000, generator=gen, dtype=torch.float64)
  grads = [torch.randn(1000, generator=gen, dtype=torch.float64) for _ in range(20)]
  h = R.Hyper(lr=0.05, momentum=0.9, decay_or_rho=0.95, eps=1e-6, lr_power=-0.5, l1=0.0, l2=0.0)
  p = th0.clone().requires_grad_(True)
  opt = {'sgd': lambda: torch.optim.SGD([p], lr=h.lr), 'momentum': lambda: torch.optim.SGD([p], lr=h.lr, momentum=h.momentum),
         'adadelta': lambda: torch.optim.Adadelta([p], lr=h.lr, rho=h.decay_or_rho, eps=h.eps)}[rule]()
  for g in grads:
    p.grad = g.clone()
    opt.step()
  want = p.detach().numpy()
  got = _run_ref(rule, h, th0.numpy(), [g.numpy() for g in grads])
  assert np.abs(got - th0.numpy()).max() > 1e-3
  assert np.all(np.abs(got - want) <= 1e-12 * np.abs(want)), float(np.abs(got / want - 1).max())


def test_rmsprop_by_hand():
  """One scalar step, written out: ms starts at 1, epsilon sits inside the root."""
  h = R.Hyper(lr=0.1, momentum=0.5, decay_or_rho=0.9, eps=0.01, lr_power=-0.5, l1=0.0, l2=0.0)
  th, g, ms, mom = 2.0, 3.0, 1.0, 0.25
  ms1 = 1.0 + (9.0 - 1.0) * 0.1                       # ms += (g^2 - ms)(1 - decay) = 1.8
  mom1 = 0.5 * 0.25 + 0.1 * 3.0 / math.sqrt(1.8 + 0.01)      # momentum mom + lr g / sqrt(ms + eps)
  th1 = 2.0 - mom1
  (t, a, b), _ = R.step('rmsprop', np.array([th]), np.array([g]), [np.array([ms]), np.array([mom])], h, 1.0, f32_scalars=False)
  assert abs(a[0] - ms1) < 1e-15 and abs(a[0] - 1.8) < 1e-15
  assert abs(b[0] - mom1) < 1e-15 and abs(b[0] - (0.125 + 0.3 / math.sqrt(1.81))) < 1e-15
  assert abs(t[0] - th1) < 1e-15
  # epsilon outside the root would give another number: this is TF's form, not torch's
  assert abs(b[0] - (0.125 + 0.3 / (math.sqrt(1.8) + 0.01))) > 1e-4


def test_ftrl_by_hand():
  """One scalar step with lr_power = -0.5, l1 and l2 set, written out; then the zeroing: |linear| <= l1 writes 0."""
  h = R.Hyper(lr=0.5, momentum=0.0, decay_or_rho=0.0, eps=0.0, lr_power=-0.5, l1=0.25, l2=0.125)
  th, g, accum, linear = 1.0, 3.0, 16.0, -1.0
  n = 16.0 + 9.0                                      # accum + g^2 = 25
  sigma = (5.0 - 4.0) / 0.5                           # (sqrt(n) - sqrt(accum)) / lr = 2
  lin = -1.0 + 3.0 - 2.0 * 1.0                        # linear + g - sigma theta = 0: the zeroing case first
  (t, a, b), _ = R.step('ftrl', np.array([th]), np.array([g]), [np.array([accum]), np.array([linear])], h, 1.0, f32_scalars=False)
  assert a[0] == n == 25.0 and b[0] == lin == 0.0 and sigma == 2.0
  assert t[0] == 0.0                                  # |linear| = 0 <= l1: theta = 0, TF's rule
  th = 0.5
  lin = -1.0 + 3.0 - 2.0 * 0.5                        # = 1
  q = 5.0 / 0.5 + 2.0 * 0.125                         # sqrt(n) / lr + 2 l2 = 10.25
  want = (0.25 - 1.0) / q                             # (sign(linear) l1 - linear) / q
  (t, a, b), _ = R.step('ftrl', np.array([th]), np.array([g]), [np.array([accum]), np.array([linear])], h, 1.0, f32_scalars=False)
  assert b[0] == 1.0 and a[0] == 25.0 and abs(t[0] - want) < 1e-15 and abs(t[0] + 0.75 / 10.25) < 1e-15
  # a general power: n^-p with p = -0.25
  h2 = h._replace(lr_power=-0.25)
  (t, a, b), _ = R.step('ftrl', np.array([th]), np.array([g]), [np.array([16.0]), np.array([linear])], h2, 1.0, f32_scalars=False)
  sigma = (25.0 ** 0.25 - 2.0) / 0.5
  lin = -1.0 + 3.0 - sigma * 0.5
  assert abs(b[0] - lin) < 1e-15 and abs(t[0] - (0.25 - lin) / (25.0 ** 0.25 / 0.5 + 0.25)) < 1e-15


def test_adagrad_has_no_epsilon_and_bounds_are_positive():
  h = R.default_hyper('adagrad', lr=0.5)
  (t, a), (bt, ba) = R.step('adagrad', np.array([1.0]), np.array([2.0]), [np.array([0.1])], h, 1.0, f32_scalars=False)
  assert abs(a[0] - 4.1) < 1e-15 and abs(t[0] - (1.0 - 0.5 * 2.0 / math.sqrt(4.1))) < 1e-15
  assert 0 < bt[0] < 1e-5 and 0 < ba[0] < 1e-5
  for rule in R.RULES:      # a bound is finite and never zero (the 2^-126 floor), whatever the magnitudes
    th, g = np.array([0.0, 1.0, -3.0]), np.array([0.0, 1e4, 1e-20])
    refs, bounds = R.step(rule, th, g, [x.astype(np.float64) for x in R.slot_init(rule, 3)], R.default_hyper(rule), 1.0)
    for r, b in zip(refs, bounds):
      assert np.all(np.isfinite(r)) and np.all(np.isfinite(b)) and np.all(b >= R.TINY), (rule, r, b)


# ------------------------------------------------------------------------------------------------ Config
def test_config_defaults_are_the_reference_flags():
  from twingan_amd import Config
  c = Config()
  assert (c.optimizer, c.adadelta_rho, c.adagrad_initial_accumulator_value, c.ftrl_learning_rate_power, c.ftrl_initial_accumulator_value,
          c.ftrl_l1, c.ftrl_l2, c.momentum, c.rmsprop_momentum, c.rmsprop_decay) == ('adam', 0.95, 0.1, -0.5, 0.1, 0.0, 0.0, 0.9, 0.9, 0.9)
  for name in ('adadelta', 'adagrad', 'adam', 'ftrl', 'momentum', 'rmsprop', 'sgd'):
    assert Config(optimizer=name).optimizer == name
  Config(ftrl_learning_rate_power=0.0, momentum=0.0, rmsprop_decay=0.0, adadelta_rho=0.0, rmsprop_momentum=0.0)


@pytest.mark.parametrize('field,value', [
    ('optimizer', 'adamw'), ('optimizer', 'Adam'), ('optimizer', ''),
    ('ftrl_learning_rate_power', 0.5), ('ftrl_learning_rate_power', 1e-9),
    ('ftrl_l1', -0.1), ('ftrl_l2', -1e-9),
    ('adagrad_initial_accumulator_value', 0.0), ('adagrad_initial_accumulator_value', -0.1),
    ('ftrl_initial_accumulator_value', 0.0), ('ftrl_initial_accumulator_value', -1.0),
    ('adadelta_rho', 1.0), ('adadelta_rho', -0.1), ('rmsprop_decay', 1.0), ('rmsprop_decay', -0.5),
    ('momentum', 1.0), ('momentum', -0.1), ('rmsprop_momentum', 1.5), ('rmsprop_momentum', -0.1)])
def test_config_rejects(field, value):
  from twingan_amd import Config
  with pytest.raises(ValueError) as e:
    Config(**{field: value})
  assert field in str(e.value) and repr(value) in str(e.value), str(e.value)


def test_slot_table_matches_the_reference_names():
  from twingan_amd.params import OPTIM_SLOTS
  for rule in R.RULES:
    assert tuple(s for s, _ in OPTIM_SLOTS[rule]) == R.SLOT_NAMES[rule]
  assert OPTIM_SLOTS['rmsprop'][0][1] == 1.0 and OPTIM_SLOTS['adam'] == (('Adam', 0.0), ('Adam_1', 0.0))


# ------------------------------------------------------------------------------------------------ the header
def _declared(header):
  text = open(os.path.join(ROOT, 'include', header)).read()
  text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
  return sorted(set(re.findall(r'\b(tg_[a-z0-9_]+)\s*\(', text)))


def _exported(lib):
  out = subprocess.run(['nm', '-D', '--defined-only', lib], stdout=subprocess.PIPE, text=True, check=True).stdout
  return {ln.split()[-1] for ln in out.splitlines() if ln.split()}


def test_optim_header_is_exported_and_bound():
  from twingan_amd import _lib
  fns = _declared('twingan_hip_optim.h')
  assert fns == ['tg_optim_slot_count', 'tg_optim_step']
  assert sorted(_lib.OPTIM_SIGNATURES) == fns
  if not os.path.exists(_lib.LIB_PATH):
    pytest.fail('%s is not built (build() compiles it)' % _lib.LIB_PATH)
  missing = [f for f in fns if f not in _exported(_lib.LIB_PATH)]
  assert not missing, missing
  # the main header and its table still agree with each other, and the two tables do not overlap
  assert sorted(_lib.SIGNATURES) == _declared('twingan_hip.h')
  assert not set(_lib.SIGNATURES) & set(_lib.OPTIM_SIGNATURES)
  # the struct and the constants follow the header
  text = open(os.path.join(ROOT, 'include', 'twingan_hip_optim.h')).read()
  m = re.search(r'typedef struct TgOptimHyper \{\s*float ([^;]+);', text)
  assert [f.strip() for f in m.group(1).split(',')] == [f for f, _ in _lib.TgOptimHyper._fields_] == list(R.Hyper._fields)
  consts = dict(re.findall(r'\b(TG_OPT_[A-Z]+) = (\d+)', text))
  assert {k: int(v) for k, v in consts.items()} == {'TG_OPT_' + r.upper(): i for r, i in R.RULE_ID.items()}
  assert _lib.OPTIM_RULES == R.RULE_ID


def test_emulated_library_exports_the_optim_header():
  sys.path.insert(0, HERE)
  try:
    import build
  finally:
    sys.path.pop(0)
  lib = build.build()
  assert not [f for f in _declared('twingan_hip_optim.h') if f not in _exported(lib)]


# ------------------------------------------------------------------------------------------------ bounds
WORKERS = 16
CASE_TIMEOUT = 120


def _build_driver():
  """Compiles optim_bounds_main.cpp with the flags of build_bounds() and links it with that build's objects but bounds_main.o."""
  sys.path.insert(0, HERE)
  try:
    import build
  finally:
    sys.path.pop(0)
  build.build_bounds()
  src = os.path.join(HERE, 'optim_bounds_main.cpp')
  obj = os.path.join(build.OUT_ASAN, 'optim_bounds_main.o')
  exe = os.path.join(build.OUT_ASAN, 'optim_bounds')
  objs = [os.path.join(build.OUT_ASAN, n + '.o') for n in build.SOURCES + ['emu']]
  deps = [src, os.path.join(ROOT, 'include', 'twingan_hip_optim.h'), os.path.join(ROOT, 'include', 'twingan_hip.h')]
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


def test_optim_bounds_cases_run_clean_under_the_sanitizer(driver):
  names, results = driver
  want = {'tg_optim_step_%s_%s_n%d_%s' % (r, m, n, o) for r in R.RULES for m in ('plain', 'ema', 'skip', 'apply') for n in (1, 1027)
          for o in 'ao'}
  assert set(names) == want and len(names) == len(want) == 96
  bad = [(n, rc, (err + out)[-1500:]) for n, rc, out, err in results if rc != 0 or ('ok ' + n) not in out]
  assert not bad, '\n\n'.join('%s (exit %s)\n%s' % b for b in bad[:6])


def test_every_function_of_the_optim_header_has_a_case(driver):
  names, _ = driver
  src = re.sub(r'//[^\n]*', ' ', open(os.path.join(HERE, 'optim_bounds_main.cpp')).read())
  called = set(re.findall(r'\b(tg_[a-z0-9_]+)\s*\(', src))
  exempt = {'tg_optim_slot_count'}      # pure query
  for f in _declared('twingan_hip_optim.h'):
    if f in exempt:
      continue
    assert f in called and any(n.startswith(f + '_') for n in names), f

