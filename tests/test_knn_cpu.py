"""CPU: the nearest-neighbour search's host side.  The guarantees of include/twingan_hip_knn.h (exactly the documented functions
declared, bound one to one by _lib.KNN_SIGNATURES, exported by the built library and by the emulated one, the three older
tables still equal to their headers), the embedding CSV (bytes against a csv.writer restatement, append, float32 round trip),
the restatement tests/knn_ref.py itself (tie rule, filler, NaN and +inf), and where the entry points read and write:
tests/hipemu/knn_bounds_main.cpp, a stand-alone program compiled with AddressSanitizer and linked with the sanitized emulated
kernels, run case by case as child processes.  Nothing sanitized is loaded into python."""
import csv
import io
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
import knn_ref as R      # noqa: E402

KNN_FUNCTIONS = ['tg_knn_plan', 'tg_knn_sqnorm', 'tg_knn_topk', 'tg_knn_workspace_bytes']


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


def test_knn_header_is_exported_and_bound():
  from twingan_amd import _lib
  assert _declared('twingan_hip_knn.h') == KNN_FUNCTIONS
  assert sorted(_lib.KNN_SIGNATURES) == KNN_FUNCTIONS
  if not os.path.exists(_lib.LIB_PATH):
    pytest.fail('%s is not built (build() compiles it)' % _lib.LIB_PATH)
  missing = [f for f in KNN_FUNCTIONS if f not in _exported(_lib.LIB_PATH)]
  assert not missing, missing
  # four disjoint tables, the three older ones still their headers
  older = {'twingan_hip.h': _lib.SIGNATURES, 'twingan_hip_optim.h': _lib.OPTIM_SIGNATURES, 'twingan_hip_summary.h': _lib.SUMMARY_SIGNATURES}
  for header, table in older.items():
    assert sorted(table) == _declared(header), header
    assert not set(table) & set(_lib.KNN_SIGNATURES), header
  # argument counts and the constants follow the header
  text = re.sub(r'/\*.*?\*/', ' ', open(os.path.join(ROOT, 'include', 'twingan_hip_knn.h')).read(), flags=re.S)
  for name, (_, args) in _lib.KNN_SIGNATURES.items():
    params = re.search(r'\b%s\s*\(([^)]*)\)' % name, text).group(1)
    assert len(args) == len([p for p in params.split(',') if p.strip()]), name
  consts = {k: int(v) for k, v in re.findall(r'#define (TG_KNN_[A-Z0-9_]+) (\d+)', text)}
  assert consts == {'TG_KNN_MAX_K': _lib.KNN_MAX_K, 'TG_KNN_L2': _lib.KNN_METRICS['l2'], 'TG_KNN_COSINE': _lib.KNN_METRICS['cosine']}


def test_emulated_library_exports_the_knn_header():
  lib = _emu_build().build()
  assert not [f for f in KNN_FUNCTIONS if f not in _exported(lib)]


# ------------------------------------------------------------------------------------------------ the restatement
def test_restatement_tie_rule_and_filler():
  dist = np.array([[3, 1, 1, 7, 1], [5, 5, 5, 5, 5]], dtype=np.int64)
  d, i = R.topk(dist, 3)
  assert i.tolist() == [[1, 2, 4], [0, 1, 2]] and d.tolist() == [[1, 1, 1], [5, 5, 5]]
  d, i = R.topk(dist, 7)      # n < k: the filler
  assert i[0].tolist() == [1, 2, 4, 0, 3, -1, -1] and np.isposinf(d[:, 5:]).all() and (d[0, :5] == [1, 1, 1, 3, 7]).all()
  # a running table, an offset, the excluded self match: the lower index wins across chunks too
  d1, i1 = R.topk(dist[:, :2], 3, index_offset=10)
  d2, i2 = R.topk(dist[:, 2:], 3, index_offset=12, prior=(d1, i1))
  da, ia = R.topk(dist, 3, index_offset=10)
  assert np.array_equal(i2, ia) and np.array_equal(d2, da)
  d, i = R.topk(dist, 3, index_offset=10, query_ids=[11, 10])
  assert i.tolist() == [[12, 14, 10], [11, 12, 13]]
  # NaN is never selected, +inf never displaces the filler
  d, i = R.topk(np.array([[np.nan, 2.0, np.inf, 1.0]]), 3)
  assert i.tolist() == [[3, 1, -1]] and d[0, :2].tolist() == [1.0, 2.0] and np.isposinf(d[0, 2])


def test_restatement_distances_and_bounds():
  q = np.array([[1.0, 2.0, -2.0], [0.0, 0.0, 0.0]])
  g = np.array([[1.0, 2.0, -2.0], [-1.0, -2.0, 2.0], [0.0, 0.0, 0.0], [3.0, 0.0, 0.0]])
  assert R.sq_l2(q, g).tolist() == [[0, 36, 9, 12], [9, 9, 0, 9]] and np.array_equal(R.sq_l2_int(q, g), R.sq_l2(q, g).astype(np.int64))
  c = R.cosine(q, g)
  assert c[0, 0] == 0.0 and c[0, 1] == 2.0 and c[0, 2] == 1.0 and np.all(c[1] == 1.0) and abs(c[0, 3] - (1 - 1 / 3)) < 1e-15
  assert np.all(R.sq_l2_bound(q, g) >= 0) and R.sq_l2_bound(q, g)[0, 1] == R.gamma(6) * (9 + 9 + 2 * 9)
  assert abs(R.cosine_bound(q, g)[0, 0] - R.gamma(11) * 3.0) < 1e-18      # S = 1, |cos| = 1, + 1
  with np.errstate(all='ignore'):
    assert np.isnan(R.sq_l2(np.array([[np.nan]]), np.array([[1.0]]))[0, 0])


# ------------------------------------------------------------------------------------------------ the CSV
class _FakeEncoder:
  """encode() of twingan_amd.embed.ContentEncoder without a device: the embedding is handed in."""

  def encode(self, images, domain):
    import torch
    return torch.from_numpy(np.asarray(images, dtype=np.float32))


def test_csv_bytes_append_and_round_trip(tmp_path):
  from twingan_amd import embed
  rng = np.random.default_rng(4)
  emb = rng.standard_normal((7, 12)).astype(np.float32)
  emb[0, :6] = [0.0, -0.0, 1.0, 1e-30, 3.4028235e38, 1.17549435e-38]
  emb[1, 0] = np.float32(1.0) + np.finfo(np.float32).eps      # needs all nine digits
  names = ['a.png', 'dir/b c.jpg', 'with,comma.png', 'quote".png', 'e', 'f', 'g']
  path = str(tmp_path / 'out.csv')
  assert embed.export_embeddings(_FakeEncoder(), [(names[:3], emb[:3])], 's', path) == 3
  assert embed.export_embeddings(_FakeEncoder(), [(names[3:5], emb[3:5]), ([n.encode() for n in names[5:]], emb[5:])], 's', path) == 4
  # the reference's _write_outputs: csv.writer over [name] + embedding.tolist()
  want = io.StringIO(newline='')
  w = csv.writer(want)
  for name, e in zip(names, emb):
    w.writerow([name] + e.tolist())
  assert open(path, newline='').read() == want.getvalue()
  assert embed.embedding_row('x', emb[1])[1] == float(emb[1, 0]) and repr(embed.embedding_row('x', emb[1])[1]) == repr(emb[1].tolist()[0])
  got_names, got = embed.read_embeddings(path)
  assert got_names == names and got.dtype == np.float32 and got.tobytes() == emb.tobytes()
  with pytest.raises(ValueError, match='names'):
    embed.export_embeddings(_FakeEncoder(), [(names[:2], emb[:3])], 's', path)
  (tmp_path / 'ragged.csv').write_text('a,1.0,2.0\nb,1.0\n')
  with pytest.raises(ValueError, match='different lengths'):
    embed.read_embeddings(str(tmp_path / 'ragged.csv'))


# ------------------------------------------------------------------------------------------------ bounds
WORKERS = 16
CASE_TIMEOUT = 120


def _build_driver():
  """Compiles knn_bounds_main.cpp with the flags of build_bounds() and links it with that build's objects but bounds_main.o."""
  build = _emu_build()
  build.build_bounds()
  src = os.path.join(HERE, 'knn_bounds_main.cpp')
  obj = os.path.join(build.OUT_ASAN, 'knn_bounds_main.o')
  exe = os.path.join(build.OUT_ASAN, 'knn_bounds')
  objs = [os.path.join(build.OUT_ASAN, n + '.o') for n in build.SOURCES + ['emu']]
  deps = [src, os.path.join(ROOT, 'include', 'twingan_hip_knn.h'), os.path.join(ROOT, 'include', 'twingan_hip.h')]
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


def test_knn_bounds_cases_run_clean_under_the_sanitizer(driver):
  names, results = driver
  dts = ('f32', 'bf16', 'f16')
  shapes = ('q1_n1_d1_k1', 'q3_n5_d16_k8', 'q33_n257_d24_k8', 'q70_n300_d27_k32')
  want = {'tg_knn_topk_%s_%s_%s' % (d, s, o) for d in dts for s in shapes for o in 'ao'}
  want |= {'tg_knn_topk_%s_%s' % (d, v) for d in dts for v in ('cosine', 'query_ids', 'cosine_query_ids')}
  want |= {'tg_knn_sqnorm_%s_r%d_%s' % (d, r, o) for d in dts for r in (1, 131) for o in 'ao'} | {'tg_knn_plan_rule'}
  assert set(names) == want and len(names) == len(want) == 46
  bad = [(n, rc, (err + out)[-1500:]) for n, rc, out, err in results if rc != 0 or ('ok ' + n) not in out]
  assert not bad, '\n\n'.join('%s (exit %s)\n%s' % b for b in bad[:6])


def test_every_function_of_the_knn_header_has_a_case(driver):
  names, _ = driver
  src = re.sub(r'//[^\n]*', ' ', open(os.path.join(HERE, 'knn_bounds_main.cpp')).read())
  called = set(re.findall(r'\b(tg_[a-z0-9_]+)\s*\(', src))
  sized = {'tg_knn_workspace_bytes': 'tg_knn_topk'}      # the size query is exercised by the case of what it sizes
  for f in KNN_FUNCTIONS:
    assert f in called, f
    assert any(n.startswith(sized.get(f, f) + '_') for n in names), f
