#!/usr/bin/env python
"""Times evaluate.KernelDistance.end() (three ops.mmd_block_sums launches and one device-to-host copy,
include/twingan_hip_mmd.h) on the GPU against the same block sums composed from torch ops, at two sizes:

  python tools/mmd_bench.py [--d 4096] [--reps 20] [--warmup 2] [--out profiles/mmd_bench.json]

  evaluation   m = n = 8192 rows a side, D = 4096 (the 256 x 256 model's 4 * 4 * 256), bf16, block 32, the cubic kernel
  subset       m = n = 1024, the rest the same: one KID subset

Both paths start from resident rows and end with the block sums of X against X, Y against Y (their diagonals left out) and X
against Y on the host, between two HIP events (the copy is the synchronisation of both).  After --warmup untimed runs of each,
the two are timed ALTERNATELY, --reps times each, so that what else the machine does falls on both; the median, the least and
the greatest of each go to the JSON, and the spread (max - min) of the runs of the same code says what a difference between
the two means.  fused: KernelDistance.end().  composed: per Gram matrix, row chunks of --chunk rows -- matmul with fp32 output
where this torch offers it (else a bf16 product widened afterwards; the JSON says which), ((x @ y.T) * gamma + 1) ** 3 in fp32,
summed per block into fp64, the diagonal's values subtracted from the diagonal blocks -- so it writes and reads every chunk of
the Gram matrix that the fused kernel never writes.  Next to each time: the operations (2 D pairs, three matrices) over it and
the time the dense bf16 MFMA peak allows.  The two paths' mmd2 are compared.

Every timed part runs under a time limit of its own (--limit seconds, a watchdog that ends the process)."""
import argparse
import json
import os
import sys
import threading

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from twingan_amd.evaluate import KernelDistance, kernel_distance_from_sums      # noqa: E402

MFMA_BF16_PEAK = 2.5e15      # dense bf16 FLOP / s, the MI355X's specified matrix peak


def limited(what, seconds, fn):
  def expire():
    sys.stderr.write('mmd_bench: %s exceeded its limit of %d s\n' % (what, seconds))
    sys.stderr.flush()
    os._exit(124)
  t = threading.Timer(seconds, expire)
  t.daemon = True
  t.start()
  try:
    return fn()
  finally:
    t.cancel()


def timed_alternating_ms(fns, reps):
  """Every fn of ``fns`` (label -> callable) once per round, ``reps`` rounds -> {label: sorted times}, {label: last result}."""
  evs = {k: [] for k in fns}
  res = {}
  for _ in range(reps):
    for k, fn in fns.items():
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      e0.record()
      res[k] = fn()
      e1.record()
      evs[k].append((e0, e1))
  torch.cuda.synchronize()
  return {k: sorted(e0.elapsed_time(e1) for e0, e1 in v) for k, v in evs.items()}, res


def make_composed(x, y, block, chunk):
  """-> (fn -> the dict KernelDistance.end() returns, how the products are formed)."""
  how = 'mm(out_dtype=float32)'
  try:
    torch.mm(x[:1], y[:8].t(), out_dtype=torch.float32)
    dots = lambda a, b: torch.mm(a, b.t(), out_dtype=torch.float32)
  except (TypeError, RuntimeError):
    how = 'bf16 matmul, widened afterwards'
    dots = lambda a, b: torch.matmul(a, b.t()).float()
  gamma = float(torch.tensor(1.0, dtype=torch.float32) / x.shape[1])

  def gram_sums(a, b, skip_diagonal):
    m, n = a.shape[0], b.shape[0]
    rows = []
    for lo in range(0, m, chunk):
      p = (dots(a[lo:lo + chunk], b) * gamma + 1.0) ** 3
      rows.append(p.reshape(-1, block, n // block, block).sum(dim=(1, 3), dtype=torch.float64))
    sums = torch.cat(rows)
    if skip_diagonal:
      diag = (torch.linalg.vector_norm(a, dim=1, dtype=torch.float32).square_() * gamma + 1.0) ** 3
      sums.diagonal().sub_(diag.reshape(-1, block).sum(dim=1, dtype=torch.float64))
    return sums

  def run():
    xx, yy, xy = gram_sums(x, x, True), gram_sums(y, y, True), gram_sums(x, y, False)
    host = torch.cat([xx.reshape(-1), yy.reshape(-1), xy.reshape(-1)]).cpu().numpy()      # the one copy
    a, b = xx.numel(), xx.numel() + yy.numel()
    return kernel_distance_from_sums(host[:a].reshape(xx.shape), host[a:b].reshape(yy.shape), host[b:].reshape(xy.shape), x.shape[0],
                                     y.shape[0], block, 1024)
  return run, how


def case(name, x, y, block, chunk, reps, warmup, limit):
  m, d = x.shape
  n = y.shape[0]
  kd = KernelDistance(d, max(m, n), block=block)
  kd.feed(x, y)
  composed, how = make_composed(x, y, block, min(chunk, m))
  fns = {'fused': kd.end, 'composed': composed}

  def go():
    for _ in range(warmup):
      for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    return timed_alternating_ms(fns, reps)
  times, results = limited(name, limit, go)
  flops = 2.0 * d * (m * m + n * n + m * n)
  row = dict(case=name, m=m, n=n, d=d, block=block, dtype=str(x.dtype), flops=flops, gram_bytes_fp32=4.0 * (m * m + n * n + m * n),
             composed_products=how, composed_chunk=min(chunk, m), reps=reps, warmup=warmup, order='alternating',
             mfma_bound_ms=flops / MFMA_BF16_PEAK * 1e3)
  for label in ('fused', 'composed'):
    ms = times[label]
    med = ms[len(ms) // 2]
    row[label] = dict(ms=med, ms_min=ms[0], ms_max=ms[-1], spread_ms=ms[-1] - ms[0], tflops=flops / med * 1e-9, share_of_bound=row['mfma_bound_ms'] / med,
                      mmd2=results[label]['mmd2'], kid_mean=results[label]['kid_mean'])
  row['fused_over_composed'] = row['fused']['ms'] / row['composed']['ms']
  row['mmd2_difference'] = abs(row['fused']['mmd2'] - row['composed']['mmd2'])
  return row


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--rows', type=int, default=8192)
  ap.add_argument('--subset', type=int, default=1024)
  ap.add_argument('--d', type=int, default=4096)
  ap.add_argument('--block', type=int, default=32)
  ap.add_argument('--chunk', type=int, default=2048)
  ap.add_argument('--reps', type=int, default=20)
  ap.add_argument('--warmup', type=int, default=2)
  ap.add_argument('--limit', type=int, default=240)
  ap.add_argument('--out', default=os.path.join('profiles', 'mmd_bench.json'))
  args = ap.parse_args()
  if not torch.cuda.is_available():
    sys.exit('mmd_bench: no GPU visible (there is no CPU path to time)')
  dev = 'cuda:0'
  gen = torch.Generator(device=dev).manual_seed(0)
  x = torch.randn(args.rows, args.d, generator=gen, device=dev, dtype=torch.float32).to(torch.bfloat16)
  y = (torch.randn(args.rows, args.d, generator=gen, device=dev, dtype=torch.float32) * 1.05 + 0.02).to(torch.bfloat16)
  rows = [case('evaluation', x, y, args.block, args.chunk, args.reps, args.warmup, args.limit),
          case('subset', x[:args.subset].contiguous(), y[:args.subset].contiguous(), args.block, args.chunk, args.reps, args.warmup, args.limit)]
  result = dict(tool='tools/mmd_bench.py', device=torch.cuda.get_device_name(0), torch=torch.__version__, cases=rows)
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'w') as fh:
    json.dump(result, fh, indent=1)
    fh.write('\n')
  for r in rows:
    print('%-10s %5d x %5d x %4d  fused %9.3f ms (spread %.3f; %6.1f TFLOP/s)  composed %9.3f ms (spread %.3f; %6.1f TFLOP/s)  fused / composed %.2f  '
          '|mmd2 difference| %.2e' % (r['case'], r['m'], r['n'], r['d'], r['fused']['ms'], r['fused']['spread_ms'], r['fused']['tflops'], r['composed']['ms'],
                                      r['composed']['spread_ms'], r['composed']['tflops'], r['fused_over_composed'], r['mmd2_difference']))


if __name__ == '__main__':
  main()
