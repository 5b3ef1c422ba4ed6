"""CPU: the training summaries' host side.  The TensorFlow histogram limits (tests/summary_ref.py restates them; the ABI's
host function must return exactly those doubles and their float round-ups), the event file (wire bytes by hand, round trip,
checksums), the PNG writer, the guarantees of include/twingan_hip_summary.h (every declared name exported, bound one to one by
_lib.SUMMARY_SIGNATURES, exported by the emulated library too), and where its entry points read and write:
tests/hipemu/summary_bounds_main.cpp, a stand-alone program compiled with AddressSanitizer and linked with the sanitized
emulated kernels, run case by case as child processes.  Nothing sanitized is loaded into python."""
import ctypes
import os
import re
import struct
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, 'tests', 'hipemu')
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import summary_ref as R      # noqa: E402


def _emu_build():
  sys.path.insert(0, HERE)
  try:
    import build
  finally:
    sys.path.pop(0)
  return build


# ------------------------------------------------------------------------------------------------ limits
def test_limits_of_the_restatement():
  pos = R.positive_limits()
  assert pos.size == 774 and pos[0] == 1e-12 and pos[-1] < 1e20 <= pos[-1] * 1.1
  lim = R.limits()
  assert lim.size == 1551 and np.all(np.diff(lim) > 0)
  assert lim[775] == 0.0 and lim[776] == 1e-12 and lim[0] == -R.DBL_MAX and lim[-1] == R.DBL_MAX
  # limits are exclusive upper edges: both zeros and every 0 <= v < 1e-12 in the bucket whose limit is 1e-12; -1e-13 in 0.0's
  idx = np.searchsorted(lim, np.array([0.0, -0.0, 9e-13, -1e-13, 1e-12]), side='right')
  assert idx.tolist() == [776, 776, 776, 775, 777]
  up = R.round_up_f32(pos)
  assert np.unique(up).size == 774 and np.all(up.astype(np.float64) >= pos)
  # v < L exactly when v < roundup(L), for the floats next to every limit
  for f in (np.nextafter(up, np.float32(0)), up, np.nextafter(up, np.float32(np.inf))):
    assert np.array_equal(f.astype(np.float64) < pos, f < up)


def test_abi_limits_are_the_restatement():
  """tg_summary_limits of the emulated library (plain host code): the same doubles, and floats that are the round-ups."""
  lib = ctypes.CDLL(_emu_build().build())
  lim = (ctypes.c_double * 1551)()
  pos = (ctypes.c_float * 774)()
  lib.tg_summary_limits.argtypes = [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_float)]
  assert lib.tg_summary_limits(lim, pos) == 0
  assert np.array_equal(np.array(lim, dtype=np.float64), R.limits())
  assert np.array_equal(np.array(pos, dtype=np.float32), R.round_up_f32(R.positive_limits()))
  assert lib.tg_summary_limits(None, None) == 0


def test_collapse_rule():
  from twingan_amd import summary
  lim = R.limits()
  rng = np.random.default_rng(5)
  for trial in range(6):
    b = np.zeros(1551)
    if trial:
      b[rng.integers(0, 1551, size=trial * 7)] = rng.integers(1, 100, size=trial * 7)
    if trial == 2:
      b[0] = b[-1] = 3
    got = summary.collapse_buckets(lim, b)
    want = R.collapse(lim, b)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert got[1].sum() == b.sum()
  # a run of empty buckets is one entry with the run's last limit
  l, c = summary.collapse_buckets([1., 2., 3., 4., 5.], [0, 0, 7, 0, 0])
  assert l.tolist() == [2., 3., 5.] and c.tolist() == [0., 7., 0.]
  l, c = summary.collapse_buckets([], [])
  assert l.tolist() == [R.DBL_MAX] and c.tolist() == [0.0]


# ------------------------------------------------------------------------------------------------ event file
def _varint(v):
  out = b''
  while v >= 0x80:
    out += bytes([(v & 0x7f) | 0x80])
    v >>= 7
  return out + bytes([v])


def test_scalar_event_bytes_by_hand(tmp_path):
  """Event{wall_time = 1: double, step = 2: varint, summary = 5{value = 1{tag = 1, simple_value = 2: float}}} inside
  uint64 length | masked crc | data | masked crc, written out here from the wire rules."""
  from twingan_amd import checkpoint, summary
  tag = b'generator_loss'
  value = b'\x0a' + _varint(len(tag)) + tag + b'\x15' + struct.pack('<f', 0.75)          # field 1 wire 2, field 2 wire 5
  summ = b'\x0a' + _varint(len(value)) + value                                            # Summary.value = 1
  ev = b'\x09' + struct.pack('<d', 1234.5) + b'\x10' + _varint(300) + b'\x2a' + _varint(len(summ)) + summ
  head = struct.pack('<Q', len(ev))
  rec = (head + struct.pack('<I', checkpoint.mask_crc(checkpoint.crc32c(head))) + ev +
         struct.pack('<I', checkpoint.mask_crc(checkpoint.crc32c(ev))))
  w = summary.EventWriter(str(tmp_path), wall_time=1000.25, host='box')
  w.add(300, [summary.scalar_value('generator_loss', 0.75)], wall_time=1234.5)
  w.close()
  assert os.path.basename(w.path) == 'events.out.tfevents.0000001000.box'
  data = open(w.path, 'rb').read()
  ver = b'\x09' + struct.pack('<d', 1000.25) + b'\x1a' + _varint(13) + b'brain.Event:2'
  first = struct.pack('<Q', len(ver))
  first += struct.pack('<I', checkpoint.mask_crc(checkpoint.crc32c(first))) + ver + struct.pack('<I', checkpoint.mask_crc(checkpoint.crc32c(ver)))
  assert data == first + rec
  assert checkpoint.crc32c(b'123456789') == 0xe3069283      # the CRC-32C check value


def test_event_round_trip_and_checksum(tmp_path):
  from twingan_amd import summary
  rng = np.random.default_rng(1)
  v = (rng.standard_normal(5000) * 0.02).astype(np.float32)
  v[:17] = 0
  want = R.summarize(v)
  lim = R.limits()
  w = summary.EventWriter(str(tmp_path), wall_time=5.0, host='h')
  proto = summary.histogram_proto(want['min'], want['max'], want['num'], want['sum'], want['sum_squares'], lim, want['bucket'])
  empty = summary.histogram_proto(0.0, 0.0, 0, 0.0, 0.0, lim, np.zeros(1551))
  w.add(0, [summary.scalar_value('learning_rate', 1e-4)], wall_time=6.0)
  w.add(7, [summary.scalar_value('losses/l_cyc_s', -2.5), summary.histogram_value('generator/w', proto),
            summary.histogram_value('empty', empty)], wall_time=7.0)
  w.close()
  evs = summary.read_events(w.path)
  assert [e['step'] for e in evs] == [0, 0, 7] and evs[0]['file_version'] == 'brain.Event:2' and evs[0]['wall_time'] == 5.0
  assert evs[1]['values'] == {'learning_rate': float(np.float32(1e-4))} and evs[1]['file_version'] is None
  got = evs[2]['values']
  assert got['losses/l_cyc_s'] == -2.5 and evs[2]['wall_time'] == 7.0
  h = got['generator/w']
  assert (h['min'], h['max'], h['num'], h['sum'], h['sum_squares']) == (float(want['min']), float(want['max']), float(want['num']),
                                                                       want['sum'], want['sum_squares'])
  wl, wb = R.collapse(lim, want['bucket'])
  assert np.array_equal(h['bucket_limit'], wl) and np.array_equal(h['bucket'], wb) and h['bucket'].sum() == 5000
  e = got['empty']
  assert (e['num'], e['min'], e['max']) == (0.0, R.DBL_MAX, -R.DBL_MAX) and e['bucket_limit'].tolist() == [R.DBL_MAX]
  assert summary.find_event_files(str(tmp_path)) == [w.path]
  # a flipped byte: in the data of the last record, then in a length
  data = bytearray(open(w.path, 'rb').read())
  for pos in (len(data) - 40, 3):
    bad = bytearray(data)
    bad[pos] ^= 0x10
    p = tmp_path / ('bad%d' % pos)
    p.write_bytes(bytes(bad))
    with pytest.raises(ValueError, match='checksum'):
      summary.read_events(str(p))
  (tmp_path / 'cut').write_bytes(bytes(data[:-3]))
  with pytest.raises(ValueError, match='cut off'):
    summary.read_events(str(tmp_path / 'cut'))


# ------------------------------------------------------------------------------------------------ PNG
@pytest.mark.parametrize('shape', [(8, 12, 3), (1, 1, 3)])
def test_png_decodes_to_the_grid(shape, tmp_path):
  from twingan_amd import monitor
  img = np.random.default_rng(2).integers(0, 256, size=shape, dtype=np.uint8)
  assert np.array_equal(R.decode_png(monitor.png_bytes(img)), img)
  monitor.write_png(str(tmp_path / 'a.png'), img)
  assert np.array_equal(R.decode_png((tmp_path / 'a.png').read_bytes()), img)


def test_grid_byte_rule_of_the_restatement():
  x = np.array([0.0, 1.0, 0.5, -0.5, 1.5, np.nan, np.inf, -np.inf, 1e30, -1e30, 254.999 / 255], dtype=np.float32)
  assert R.grid_bytes(x).tolist() == [0, 255, 127, 0, 255, 0, 255, 0, 255, 0, 254]
  # where numpy's own rule is defined (|x * 255| < 2^31) the two agree
  y = np.random.default_rng(3).uniform(-2, 3, 4096).astype(np.float32)
  assert np.array_equal(R.grid_bytes(y), np.clip((y * np.float32(255.0)).astype(np.int32), 0, 255).astype(np.uint8))


# ------------------------------------------------------------------------------------------------ the header
def _declared(header):
  text = open(os.path.join(ROOT, 'include', header)).read()
  text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
  return sorted(set(re.findall(r'\b(tg_[a-z0-9_]+)\s*\(', text)))


def _exported(lib):
  out = subprocess.run(['nm', '-D', '--defined-only', lib], stdout=subprocess.PIPE, text=True, check=True).stdout
  return {ln.split()[-1] for ln in out.splitlines() if ln.split()}


def test_summary_header_is_exported_and_bound():
  from twingan_amd import _lib
  fns = _declared('twingan_hip_summary.h')
  assert fns == ['tg_image_grid_table_bytes', 'tg_image_grid_table_fill', 'tg_image_grid_u8', 'tg_summary_limits', 'tg_summary_multi',
                 'tg_summary_table_bytes', 'tg_summary_table_fill', 'tg_summary_workspace_bytes']
  assert sorted(_lib.SUMMARY_SIGNATURES) == fns
  if not os.path.exists(_lib.LIB_PATH):
    pytest.fail('%s is not built (build() compiles it)' % _lib.LIB_PATH)
  missing = [f for f in fns if f not in _exported(_lib.LIB_PATH)]
  assert not missing, missing
  # the three tables do not overlap, and the other two still follow their headers
  assert sorted(_lib.SIGNATURES) == _declared('twingan_hip.h') and sorted(_lib.OPTIM_SIGNATURES) == _declared('twingan_hip_optim.h')
  assert not set(_lib.SUMMARY_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.OPTIM_SIGNATURES))
  # the struct and the constants follow the header
  text = open(os.path.join(ROOT, 'include', 'twingan_hip_summary.h')).read()
  body = re.sub(r'/\*.*?\*/', ' ', re.search(r'typedef struct TgSummaryStats \{(.*?)\} TgSummaryStats;', text, flags=re.S).group(1), flags=re.S)
  fields = [(t, n.strip()) for t, names in re.findall(r'(double|float|uint32_t)\s+([^;]+);', body) for n in names.split(',')]
  ctype = {'double': ctypes.c_double, 'float': ctypes.c_float, 'uint32_t': ctypes.c_uint32}
  assert [(n, ctype[t]) for t, n in fields] == list(_lib.TgSummaryStats._fields_)
  assert ctypes.sizeof(_lib.TgSummaryStats) == 40
  consts = {k: int(v) for k, v in re.findall(r'#define (TG_SUMMARY_[A-Z_]+) (\d+)', text)}
  assert consts == {'TG_SUMMARY_POS_LIMITS': _lib.SUMMARY_POS_LIMITS, 'TG_SUMMARY_BUCKETS': _lib.SUMMARY_BUCKETS}
  assert _lib.SUMMARY_BUCKETS == 2 * _lib.SUMMARY_POS_LIMITS + 3 == R.limits().size


def test_emulated_library_exports_the_summary_header():
  lib = _emu_build().build()
  assert not [f for f in _declared('twingan_hip_summary.h') if f not in _exported(lib)]


# ------------------------------------------------------------------------------------------------ bounds
WORKERS = 16
CASE_TIMEOUT = 120


def _build_driver():
  """Compiles summary_bounds_main.cpp with the flags of build_bounds() and links it with that build's objects but bounds_main.o."""
  build = _emu_build()
  build.build_bounds()
  src = os.path.join(HERE, 'summary_bounds_main.cpp')
  obj = os.path.join(build.OUT_ASAN, 'summary_bounds_main.o')
  exe = os.path.join(build.OUT_ASAN, 'summary_bounds')
  objs = [os.path.join(build.OUT_ASAN, n + '.o') for n in build.SOURCES + ['emu']]
  deps = [src, os.path.join(ROOT, 'include', 'twingan_hip_summary.h'), os.path.join(ROOT, 'include', 'twingan_hip.h')]
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


def test_summary_bounds_cases_run_clean_under_the_sanitizer(driver):
  names, results = driver
  dts = ('f32', 'bf16', 'f16')
  want = {'tg_summary_multi_%s_n%d_%s' % (d, n, o) for d in dts for n in (1, 1027) for o in 'ao'}
  want |= {'tg_summary_multi_%s_strided_%s' % (d, o) for d in dts for o in 'ao'}
  want |= {'tg_summary_multi_f32_n1027_scale%d' % m for m in (1, 2, 3)} | {'tg_summary_multi_mixed_table'}
  want |= {'tg_image_grid_u8_%s_%s_c%d' % (d, g, c) for d in dts for g in ('1x1', '3x2') for c in (1, 3)}
  want |= {'tg_summary_limits_exact', 'tg_summary_table_fill_exact', 'tg_image_grid_table_fill_exact'}
  assert set(names) == want and len(names) == len(want) == 37
  bad = [(n, rc, (err + out)[-1500:]) for n, rc, out, err in results if rc != 0 or ('ok ' + n) not in out]
  assert not bad, '\n\n'.join('%s (exit %s)\n%s' % b for b in bad[:6])


def test_every_function_of_the_summary_header_has_a_case(driver):
  names, _ = driver
  src = re.sub(r'//[^\n]*', ' ', open(os.path.join(HERE, 'summary_bounds_main.cpp')).read())
  called = set(re.findall(r'\b(tg_[a-z0-9_]+)\s*\(', src))
  sized = {'tg_summary_table_bytes': 'tg_summary_table_fill', 'tg_summary_workspace_bytes': 'tg_summary_multi',
           'tg_image_grid_table_bytes': 'tg_image_grid_table_fill'}      # a size query is exercised by the case of what it sizes
  for f in _declared('twingan_hip_summary.h'):
    assert f in called, f
    assert any(n.startswith(sized.get(f, f) + '_') for n in names), f
