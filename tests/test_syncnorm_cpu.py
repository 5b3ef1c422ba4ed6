"""CPU: the host side of the cross-replica batch statistics (Config.cross_replica_norm).  The guarantees of
include/twingan_hip_syncnorm.h (exactly the documented functions declared, bound one to one by _lib.SYNCNORM_SIGNATURES, exported
by the built library and by the emulated one, the four older tables still equal to their headers); where the entry points read
and write: tests/hipemu/syncnorm_bounds_main.cpp, a stand-alone program compiled with AddressSanitizer and linked with the
sanitized emulated kernels, run case by case as child processes (nothing sanitized is loaded into python); the merge rule
restated in float64 against numpy on the concatenation; Config's and the Trainer's refusals; dp.ReplicaGather over gloo in two
CPU processes."""
import os
import re
import socket
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, 'tests', 'hipemu')

SYNCNORM_FUNCTIONS = ['tg_norm_act_bwd_apply', 'tg_norm_act_bwd_sums', 'tg_norm_moments', 'tg_norm_moments_merge']


def _emu_build():
  sys.path.insert(0, HERE)
  try:
    import build
  finally:
    sys.path.pop(0)
  return build


# ------------------------------------------------------------------------------------------------ the header
def _declared(header):
  text = open(os.path.join(ROOT, 'include', header)).read()
  text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
  return sorted(set(re.findall(r'\b(tg_[a-z0-9_]+)\s*\(', text)))


def _exported(lib):
  out = subprocess.run(['nm', '-D', '--defined-only', lib], stdout=subprocess.PIPE, text=True, check=True).stdout
  return {ln.split()[-1] for ln in out.splitlines() if ln.split()}


def test_syncnorm_header_is_exported_and_bound():
  from twingan_amd import _lib
  assert _declared('twingan_hip_syncnorm.h') == SYNCNORM_FUNCTIONS
  assert sorted(_lib.SYNCNORM_SIGNATURES) == SYNCNORM_FUNCTIONS
  if not os.path.exists(_lib.LIB_PATH):
    pytest.fail('%s is not built (build() compiles it)' % _lib.LIB_PATH)
  missing = [f for f in SYNCNORM_FUNCTIONS if f not in _exported(_lib.LIB_PATH)]
  assert not missing, missing
  # five disjoint tables, the four older ones still their headers
  older = {'twingan_hip.h': _lib.SIGNATURES, 'twingan_hip_optim.h': _lib.OPTIM_SIGNATURES, 'twingan_hip_summary.h': _lib.SUMMARY_SIGNATURES,
           'twingan_hip_knn.h': _lib.KNN_SIGNATURES}
  for header, table in older.items():
    assert sorted(table) == _declared(header), header
    assert not set(table) & set(_lib.SYNCNORM_SIGNATURES), header
  # argument counts follow the header
  text = re.sub(r'/\*.*?\*/', ' ', open(os.path.join(ROOT, 'include', 'twingan_hip_syncnorm.h')).read(), flags=re.S)
  for name, (_, args) in _lib.SYNCNORM_SIGNATURES.items():
    params = re.search(r'\b%s\s*\(([^)]*)\)' % name, text).group(1)
    assert len(args) == len([p for p in params.split(',') if p.strip()]), name


def test_emulated_library_exports_the_syncnorm_header():
  lib = _emu_build().build()
  assert not [f for f in SYNCNORM_FUNCTIONS if f not in _exported(lib)]


# ------------------------------------------------------------------------------------------------ the merge rule
def _moments64(x):
  """x [pixels, c] float64 -> (mean, M2) of one replica."""
  m = x.mean(axis=0)
  return m, ((x - m) ** 2).sum(axis=0)


def _merge64(rows, count):
  """include/twingan_hip_syncnorm.h tg_norm_moments_merge in float64: rows = [(mean_r, M2_r)] of equal count, rank order."""
  R = len(rows)
  mean = sum(m for m, _ in rows) / R
  m2 = sum(q for _, q in rows) + count * sum((m - mean) ** 2 for m, _ in rows)
  return mean, m2 / (R * count)


@pytest.mark.parametrize('R', [1, 2, 3, 8])
def test_merge_rule_equals_numpy_on_the_concatenation(R):
  rng = np.random.default_rng(R)
  for count, c, mu, sd in ((16, 5, 0.7, 1.5), (260, 3, 300.0, 0.05), (4096, 8, 8.0, 0.25)):
    x = mu + sd * rng.standard_normal((R, count, c)) + rng.standard_normal((R, 1, c)) * sd      # replicas with their own means
    mean, var = _merge64([_moments64(x[r]) for r in range(R)], count)
    cat = x.reshape(R * count, c)
    assert np.abs(mean - cat.mean(axis=0)).max() <= 1e-13 * max(1.0, abs(mu))
    assert np.abs(var - cat.var(axis=0)).max() <= 1e-11 * cat.var(axis=0).max()
    # what the rule is there to avoid: raw sums and sums of squares at this offset lose the variance in float32
    if mu == 300.0:
      s1 = x.astype(np.float32).sum(axis=(0, 1), dtype=np.float32)
      s2 = (x.astype(np.float32) ** 2).sum(axis=(0, 1), dtype=np.float32)
      raw = s2 / np.float32(R * count) - (s1 / np.float32(R * count)) ** 2
      assert np.abs(raw - cat.var(axis=0)).max() > 0.1 * cat.var(axis=0).max()


# ------------------------------------------------------------------------------------------------ validation
def test_config_flag_needs_a_batch_normaliser():
  from twingan_amd import Config
  assert Config().cross_replica_norm is False
  for nt in ('batch_norm', 'batch_renorm', 'batch_renorm_native'):
    assert Config(generator_norm_type=nt, cross_replica_norm=True).cross_replica_norm is True
  for nt in ('instance_norm', 'layer_norm_native', 'none'):
    assert Config(generator_norm_type=nt).cross_replica_norm is False
    with pytest.raises(ValueError, match='cross_replica_norm needs a batch normaliser'):
      Config(generator_norm_type=nt, cross_replica_norm=True)


def test_trainer_refuses_graph_capture_with_cross_replica_statistics():
  from twingan_amd import Config
  from twingan_amd.twingan import Trainer
  cfg = Config(hw=16, max_ch=8, precision='fp32', generator_norm_type='batch_renorm', cross_replica_norm=True)
  with pytest.raises(ValueError, match='runs the eager step'):
    Trainer(cfg, device='cpu', world_size=2, use_graph=True)


def test_parameter_dict_has_no_replicas_by_default():
  from twingan_amd import pggan
  from twingan_amd.params import _ParamDict
  assert _ParamDict().replicas is None and pggan._replicas(_ParamDict()) is None and pggan._replicas({}) is None


# ------------------------------------------------------------------------------------------------ ReplicaGather over gloo
def _gather_worker(rank, world, port, q):
  import datetime
  import torch.distributed as dist
  os.environ['MASTER_ADDR'] = '127.0.0.1'
  os.environ['MASTER_PORT'] = str(port)
  dist.init_process_group('gloo', rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
  try:
    from twingan_amd.dp import ReplicaGather
    rep = ReplicaGather(world, None)
    assert (rep.size, rep.rank) == (world, rank) and rep.stats() == dict(gather_bytes=0, collectives=0)
    a = rep.gather(torch.full((2, 3, 5), float(rank + 1)))
    b = rep.gather(torch.arange(4, dtype=torch.float32) + 10 * rank)      # a second one, another shape: program order
    with pytest.raises(ValueError):
      rep.gather(torch.zeros(3, dtype=torch.float64))
    q.put((rank, a.numpy(), b.numpy(), rep.stats()))
    dist.barrier()
  finally:
    dist.destroy_process_group()


def test_replica_gather_rows_in_rank_order_world2():
  import torch.multiprocessing as mp
  sk = socket.socket()
  sk.bind(('127.0.0.1', 0))
  port = sk.getsockname()[1]
  sk.close()
  ctx = mp.get_context('spawn')
  q = ctx.Queue()
  procs = [ctx.Process(target=_gather_worker, args=(r, 2, port, q)) for r in range(2)]
  try:
    for p in procs:
      p.start()
    got = {}
    for _ in range(2):
      r, a, b, stats = q.get(timeout=300)
      got[r] = (a, b, stats)
    for p in procs:
      p.join(timeout=120)
      assert p.exitcode == 0
  finally:
    for p in procs:
      if p.is_alive():
        p.terminate()
        p.join(timeout=30)
  for r in (0, 1):
    a, b, stats = got[r]
    assert a.shape == (2, 2, 3, 5) and np.all(a[0] == 1.0) and np.all(a[1] == 2.0)
    assert b.tolist() == [[0, 1, 2, 3], [10, 11, 12, 13]]
    assert stats == dict(gather_bytes=4 * (2 * 30 + 2 * 4), collectives=2)
  assert got[0][0].tobytes() == got[1][0].tobytes() and got[0][1].tobytes() == got[1][1].tobytes()


def test_replica_gather_single_clone_is_a_copy():
  from twingan_amd.dp import ReplicaGather
  rep = ReplicaGather(1)
  t = torch.arange(6, dtype=torch.float32).view(2, 3)
  out = rep.gather(t)
  assert out.shape == (1, 2, 3) and torch.equal(out[0], t) and out.data_ptr() != t.data_ptr()
  assert rep.stats() == dict(gather_bytes=0, collectives=0)


# ------------------------------------------------------------------------------------------------ bounds
WORKERS = 16
CASE_TIMEOUT = 120


def _build_driver():
  """Compiles syncnorm_bounds_main.cpp with the flags of build_bounds() and links it with that build's objects but bounds_main.o."""
  build = _emu_build()
  build.build_bounds()
  src = os.path.join(HERE, 'syncnorm_bounds_main.cpp')
  obj = os.path.join(build.OUT_ASAN, 'syncnorm_bounds_main.o')
  exe = os.path.join(build.OUT_ASAN, 'syncnorm_bounds')
  objs = [os.path.join(build.OUT_ASAN, n + '.o') for n in build.SOURCES + ['emu']]
  deps = [src, os.path.join(ROOT, 'include', 'twingan_hip_syncnorm.h'), os.path.join(ROOT, 'include', 'twingan_hip.h')]
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


def test_syncnorm_bounds_cases_run_clean_under_the_sanitizer(driver):
  names, results = driver
  dts = ('f32', 'bf16', 'f16')
  shapes = ('n1_4x4_c8', 'n3_10x26_c3', 'n2_10x26_c32', 'n2_64x16_c24')
  want = {'tg_norm_moments_%s_%s' % (d, s) for d in dts for s in shapes}
  want |= {'tg_norm_act_bwd_%s_%s_%s_v%d' % (k, d, s, v) for k in ('sums', 'apply') for d in dts for s in shapes for v in range(3)}
  want |= {'tg_norm_moments_merge_r%d_%s' % (r, s) for r in (1, 2, 8) for s in shapes}
  assert set(names) == want and len(names) == len(want) == 96
  bad = [(n, rc, (err + out)[-1500:]) for n, rc, out, err in results if rc != 0 or ('ok ' + n) not in out]
  assert not bad, '\n\n'.join('%s (exit %s)\n%s' % b for b in bad[:6])


def test_every_function_of_the_syncnorm_header_has_a_case(driver):
  names, _ = driver
  src = re.sub(r'//[^\n]*', ' ', open(os.path.join(HERE, 'syncnorm_bounds_main.cpp')).read())
  called = set(re.findall(r'\b(tg_[a-z0-9_]+)\s*\(', src))
  for f in SYNCNORM_FUNCTIONS:
    assert f in called, f
    # tg_norm_moments is a prefix of tg_norm_moments_merge: the case names of the former go on with a dtype
    assert any(re.match(r'%s_(f32|bf16|f16|r\d)' % f, n) for n in names), f
