"""CPU: where the kernels read and write.  tests/hipemu/bounds_main.cpp is a stand-alone program (its own main, linked with
the emulated kernels, everything compiled with AddressSanitizer) that hands every entry point of include/twingan_hip.h heap
buffers of exactly the documented sizes: a store or load one byte outside any of them is a sanitizer report that names the
kernel's line.  After a clean return each case also checks that inputs are untouched, that no element of an output still
holds the pre-fill and that float outputs are finite.  The cases run here as child processes, 16 at a time; nothing loads
the program into python.

  python tests/test_bounds_cpu.py [substring]     runs the cases by hand and prints the time of each
"""
import json
import os
import re
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, 'tests', 'hipemu')
CASE_TIMEOUT = 600          # seconds per case; the whole run stays inside the 1500 s tests/test_emu_kernels.py allows itself
TOTAL_BUDGET = 1500
WORKERS = 16

# Entry points of the header that no driver case names, each with its reason.
EXEMPT = {
    'tg_version': 'version getter',
    'tg_last_error': 'error getter',
    'tg_last_kernel': 'getter (the driver prints it after every conv case)',
    'tg_set_deterministic': 'process-wide switch',
    'tg_get_deterministic': 'process-wide switch',
    'tg_conv2d_upcat_supported': 'pure query',
    'tg_flash_attention_supported': 'pure query',
    'tg_loss_scale_state_bytes': 'pure query',
    'tg_comm_unique_id_bytes': 'comm: stubbed by the emulator',
    'tg_comm_unique_id': 'comm: stubbed by the emulator',
    'tg_comm_init': 'comm: stubbed by the emulator',
    'tg_allreduce': 'comm: stubbed by the emulator',
    'tg_comm_destroy': 'comm: stubbed by the emulator',
}

# Rows of tests/golden/dispatch_edge_kernels.json that the driver does not have to reach in full.  Measured here, 8 cores,
# one case alone over the sanitized emulation: a 128x128 row of EDGE_CASES 30-50 s (bwd_weight_bias tile_wres16 n15: 29 s), a
# grouped 128x128 row 22 s (fwd g2_tile_n16), the 264-channel minibatch-stddev row 52 s (fwd g2_mbstd_c264_n264).  Each fits
# the per-case limit; together they do not fit the run: the driver as it stands (with the six EDGE_CASES rows' forward and
# backward-data kernels in both types and their masked / statistics / pool / sign / unpool kernels in bf16, 156 cases that
# take up to 259 s each with 16 running at once) needs 717 s of the 1500, and the ~280 cases left (the f16 forms of those
# variants, the filter gradients, the 4 grouped tile rows, the 264-channel row and the 6 upsample-concat rows, both sides, both
# types) would add some 1200 s.  Every symbol of these rows that the driver does not print is asserted on the device through
# tg_last_kernel() at its recorded batch: tests/test_gpu_bounds.py test_edge_rows_*.
DEVICE_ROWS = ('tile_', 'g2_tile', 'g3_tile', 'upcat_', 'g2_mbstd')


def _build():
  sys.path.insert(0, HERE)
  try:
    import build
  finally:
    sys.path.pop(0)
  return build.build_bounds()


def _first_report(text):
  """The sanitizer's first report, shortened: the ERROR line, the access, the top frames, the 'located' line."""
  lines = text.splitlines()
  out, frames = [], 0
  for i, ln in enumerate(lines):
    if 'ERROR: AddressSanitizer' in ln:
      for ln2 in lines[i:]:
        s = ln2.strip()
        if s.startswith('#'):
          frames += 1
          if frames <= 6:
            out.append(ln2)
        elif 'ERROR:' in ln2 or s.startswith(('READ of', 'WRITE of')) or 'located' in ln2:
          out.append(ln2)
        if 'located' in ln2:
          break
      break
  fails = [ln for ln in lines if ln.startswith('FAIL ')]
  return '\n'.join(fails + out) or text[-1500:]


def _run_case(binary, name):
  t0 = time.time()
  try:
    r = subprocess.run([binary, '--case', name], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=CASE_TIMEOUT,
                       env=dict(os.environ, ASAN_OPTIONS='detect_leaks=0:abort_on_error=0'))
    rc, out, err = r.returncode, r.stdout, r.stderr
  except subprocess.TimeoutExpired as e:
    rc, out, err = -1, '', 'FAIL %s: no result within %d s' % (name, CASE_TIMEOUT)
  return name, rc, out, err, time.time() - t0


def run_all(select=None):
  binary = _build()
  names = subprocess.run([binary, '--list'], stdout=subprocess.PIPE, text=True, check=True).stdout.split()
  if select:
    names = [n for n in names if select in n]
  t0 = time.time()
  with ThreadPoolExecutor(max_workers=WORKERS) as ex:
    results = list(ex.map(lambda n: _run_case(binary, n), names))
  return names, results, time.time() - t0


@pytest.fixture(scope='module')
def driver_run():
  return run_all()


def test_every_case_runs_clean_under_the_sanitizer(driver_run):
  names, results, total = driver_run
  assert len(names) == len(set(names)) and len(names) > 100, len(names)
  bad = [(n, rc, _first_report(err + out)) for n, rc, out, err, _ in results if rc != 0 or ('ok ' + n) not in out]
  slow = sorted(results, key=lambda r: -r[4])[:5]
  print('bounds driver: %d cases in %.0f s; slowest: %s' % (len(names), total, ', '.join('%s %.0f s' % (r[0], r[4]) for r in slow)))
  assert not bad, '\n\n'.join('%s (exit %s)\n%s' % b for b in bad[:8])
  assert total < TOTAL_BUDGET, total


def _header_functions():
  text = open(os.path.join(ROOT, 'include', 'twingan_hip.h')).read()
  text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
  return sorted(set(re.findall(r'\b(tg_[a-z0-9_]+)\s*\(', text)))


def test_every_entry_point_of_the_header_has_a_case_or_a_reason():
  fns = _header_functions()
  assert len(fns) > 120, len(fns)
  src = open(os.path.join(HERE, 'bounds_cases.inc')).read()
  src = re.sub(r'//[^\n]*', ' ', src)
  called = set(re.findall(r'\b(tg_[a-z0-9_]+)\s*\(', src))
  missing = [f for f in fns if f not in called and f not in EXEMPT]
  assert not missing, ('entry points without a bounds case', missing)
  stale = [f for f in EXEMPT if f not in fns]
  assert not stale, ('exemptions for functions the header no longer has', stale)
  assert len(EXEMPT) <= 16 and all(EXEMPT.values())


def _symbols(node, out):
  if isinstance(node, dict):
    for v in node.values():
      _symbols(v, out)
  elif isinstance(node, str):
    out.add(node)


def test_driver_reaches_the_recorded_dispatch_symbols(driver_run):
  names, results, _ = driver_run
  reached = set()
  for _, rc, out, _, _ in results:
    reached.update(ln[len('kernel: '):].strip() for ln in out.splitlines() if ln.startswith('kernel: ') and ln[8:].strip())
  table = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'dispatch_edge_kernels.json')))
  want, device_only = set(), set()
  for row, rec in table.items():
    _symbols(rec, device_only if row.startswith(DEVICE_ROWS) else want)
  device_only -= reached
  print('kernel symbols reached by the driver (%d): %s' % (len(reached), ', '.join(sorted(reached))))
  print('recorded for the rows left to the device and not reached here (%d): %s' % (len(device_only), ', '.join(sorted(device_only))))
  missing = sorted(want - reached)
  assert not missing, ('recorded symbols of rows cheap enough for the driver that no case reached', missing)


if __name__ == '__main__':
  names, results, total = run_all(sys.argv[1] if len(sys.argv) > 1 else None)
  for n, rc, out, err, dt in sorted(results, key=lambda r: r[4]):
    print('%-6s %6.1f s  %s' % ('ok' if rc == 0 else 'FAIL', dt, n))
    if rc != 0:
      print(_first_report(err + out))
  print('%d cases, %d failed, %.0f s' % (len(names), sum(1 for r in results if r[1] != 0), total))
