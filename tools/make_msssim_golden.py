#!/usr/bin/env python
"""Generates tests/golden/msssim_cases.npz: what the REFERENCE's own MS-SSIM code (libs/ms_ssim.py, NumPy / SciPy) returns
for the seeded inputs of tests/msssim_np.py.  The module is loaded in place from the reference checkout (TG_REFERENCE_DIR,
default /root/reference, as oracle/tf_shim/loader.py does for the TF sources); nothing of it is copied.  Recorded per case:
the per-level (ssim, cs) of _SSIMForMultiScale over the _HoxDownsample pyramid, msssim() of every pair alone and of the
batch, and a CRC-32 of each input batch -- results, names and checksums only.

Needs the reference checkout and SciPy, i.e. runs where the fixtures are made; the tests read the committed file.
Run:  python tools/make_msssim_golden.py      (rewrites the file; deterministic)
"""
import importlib.util
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import msssim_np as M      # noqa: E402


def load_reference(root=None):
  root = root or os.environ.get('TG_REFERENCE_DIR', '/root/reference')
  path = os.path.join(root, 'libs', 'ms_ssim.py')
  if not os.path.exists(path):
    raise FileNotFoundError(path)
  spec = importlib.util.spec_from_file_location('_reference_ms_ssim', path)
  mod = importlib.util.module_from_spec(spec)
  with warnings.catch_warnings():
    warnings.simplefilter('ignore')      # scipy.ndimage.filters is a deprecated alias
    spec.loader.exec_module(mod)
  return mod


def reference_tables(ref, x1, x2, max_val=255., weights=None, k1=0.01, k2=0.03):
  """-> (score[B], ssim[L, B], cs[L, B], mean): the reference's functions called as its msssim() calls them."""
  weights = list(weights) if weights is not None else None
  levels = len(weights) if weights else 5
  a, b = x1.astype(np.float32), x2.astype(np.float32)
  ssim, cs = [], []
  for _ in range(levels):
    s, c = ref._SSIMForMultiScale(a, b, max_val=max_val, k1=k1, k2=k2)
    ssim.append(s)
    cs.append(c)
    a, b = ref._HoxDownsample(a), ref._HoxDownsample(b)
  score = [ref.msssim(x1[i:i + 1], x2[i:i + 1], max_val=max_val, k1=k1, k2=k2, weights=weights) for i in range(x1.shape[0])]
  mean = ref.msssim(x1, x2, max_val=max_val, k1=k1, k2=k2, weights=weights)
  return np.asarray(score, np.float64), np.asarray(ssim, np.float64), np.asarray(cs, np.float64), float(mean)


def main():
  ref = load_reference()
  n, lmax, bmax = len(M.CASES), 5, max(c['b'] for c in M.CASES)
  score, mean = np.zeros((n, bmax)), np.zeros(n)
  ssim, cs = np.zeros((n, lmax, bmax)), np.zeros((n, lmax, bmax))
  crc1, crc2, levels = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int32)
  for i, case in enumerate(M.CASES):
    d1, d2 = M.case_inputs(case)
    x1, x2 = M.metric_inputs(case, d1, d2)
    s, ss, c, m = reference_tables(ref, x1, x2, weights=case['weights'])
    L = ss.shape[0]
    score[i], mean[i], ssim[i, :L], cs[i, :L], levels[i] = s, m, ss, c, L
    crc1[i], crc2[i] = M.checksum(d1), M.checksum(d2)
    print('%-36s mean %.9f' % (case['name'], m), flush=True)
  np.savez_compressed(M.GOLDEN, names=np.array([c['name'] for c in M.CASES]), levels=levels, score=score, mean=mean, ssim=ssim,
                      cs=cs, crc1=crc1, crc2=crc2)
  print('wrote %s (%d bytes)' % (M.GOLDEN, os.path.getsize(M.GOLDEN)))


if __name__ == '__main__':
  main()
