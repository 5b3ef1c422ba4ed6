#!/usr/bin/env python
"""Times the fused nearest-neighbour search (ops.knn_topk, include/twingan_hip_knn.h) on the GPU against the same search
composed from torch ops, at one search size and one latency size:

  python tools/knn_bench.py [--q 1024] [--n 131072] [--d 4096] [--k 8] [--reps 30] [--warmup 2] [--out profiles/knn_bench.json]

  search    Q = 1024 queries, N = 131072 gallery rows, D = 4096 (the 256 x 256 model's 4 * 4 * 256), k = 8, bf16, squared L2
  latency   Q = 1, the rest the same

Both paths run the whole search on resident tensors between two HIP events.  After --warmup untimed runs of each, the two are
timed ALTERNATELY, --reps times each (fused, composed, fused, ...), so that what else the machine does falls on both; the
median, the least and the greatest of each go to the JSON with --reps and --warmup, and the spread (max - min) of the runs of
the same code says what a difference between the two means.  fused: one ops.knn_topk call (norms, tile kernel, merge).
composed: the gallery in chunks of --chunk rows -- matmul with fp32 output where this torch offers it (else a bf16 product
widened afterwards; the JSON says which), squared row norms in ONE pass over the 16-bit rows with fp32 accumulation
(torch.linalg.vector_norm(dtype=float32): no fp32 copy of the chunk is written), |q|^2 + |g|^2 - 2 q.g clamped at 0, topk, and
a topk over the running table and the chunk's.
Next to each time: the operations (2 Q N D) over it, and its two bounds (operations over the dense bf16 MFMA peak, gallery
bytes over the HBM peak) with the name of the one that applies.  The indices of the two paths are compared (they may differ
where bf16 products tie or where the composed path rounded its products): the fraction of equal entries is reported.

Every timed part runs under a time limit of its own (--limit seconds, a watchdog that ends the process)."""
import argparse
import json
import os
import sys
import threading

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from twingan_amd import ops      # noqa: E402

HBM_PEAK = 8.0e12        # bytes / s, the MI355X's specified HBM3E bandwidth
MFMA_BF16_PEAK = 2.5e15      # dense bf16 FLOP / s, the MI355X's specified matrix peak


def limited(what, seconds, fn):
  def expire():
    sys.stderr.write('knn_bench: %s exceeded its limit of %d s\n' % (what, seconds))
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


def make_composed(q, g, k, chunk):
  """-> (fn, how the products are formed)."""
  how = 'mm(out_dtype=float32)'
  try:
    torch.mm(q[:1], g[:8].t(), out_dtype=torch.float32)
    dots = lambda gc: torch.mm(q, gc.t(), out_dtype=torch.float32)
  except (TypeError, RuntimeError):
    how = 'bf16 matmul, widened afterwards'
    dots = lambda gc: torch.matmul(q, gc.t()).float()
  sqnorm = lambda x: torch.linalg.vector_norm(x, dim=1, dtype=torch.float32).square_()      # one pass, fp32 accumulation

  def run():
    qq = sqnorm(q)[:, None]
    best_d = best_i = None
    for lo in range(0, g.shape[0], chunk):
      gc = g[lo:lo + chunk]
      d2 = (qq + sqnorm(gc)[None, :] - 2.0 * dots(gc)).clamp_min_(0.0)
      cd, ci = torch.topk(d2, min(k, gc.shape[0]), dim=1, largest=False)
      ci = ci + lo
      if best_d is not None:
        cd, ci = torch.cat([best_d, cd], 1), torch.cat([best_i, ci], 1)
        cd, sel = torch.topk(cd, k, dim=1, largest=False)
        ci = torch.gather(ci, 1, sel)
      best_d, best_i = cd, ci
    return best_d, best_i
  return run, how


def case(name, q, g, k, chunk, reps, warmup, limit):
  nq, d = q.shape
  n = g.shape[0]
  fused = lambda: ops.knn_topk(q, g, k)
  composed, how = make_composed(q, g, k, chunk)
  fns = {'fused': fused, 'composed': composed}

  def go():
    for _ in range(warmup):
      for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    return timed_alternating_ms(fns, reps)
  times, results = limited(name, limit, go)
  flops, nbytes = 2.0 * nq * n * d, float(n + nq) * d * q.element_size()
  row = dict(case=name, q=nq, n=n, d=d, k=k, dtype=str(q.dtype), flops=flops, gallery_bytes=nbytes, composed_products=how, composed_chunk=chunk,
             composed_norms='linalg.vector_norm(dtype=float32), one pass', reps=reps, warmup=warmup, order='alternating',
             mfma_bound_ms=flops / MFMA_BF16_PEAK * 1e3, hbm_bound_ms=nbytes / HBM_PEAK * 1e3)
  row['bound_by'] = 'bf16 MFMA peak' if row['mfma_bound_ms'] > row['hbm_bound_ms'] else 'HBM bandwidth'
  for label in ('fused', 'composed'):
    ms = times[label]
    med = ms[len(ms) // 2]
    row[label] = dict(ms=med, ms_min=ms[0], ms_max=ms[-1], spread_ms=ms[-1] - ms[0], tflops=flops / med * 1e-9, share_of_bound=max(row['mfma_bound_ms'], row['hbm_bound_ms']) / med)
  row['fused_over_composed'] = row['fused']['ms'] / row['composed']['ms']
  fi, ci = results['fused'][1], results['composed'][1]
  row['idx_equal_fraction'] = float((fi == ci).float().mean().item())
  row['idx_first_equal_fraction'] = float((fi[:, 0] == ci[:, 0]).float().mean().item())
  return row


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--q', type=int, default=1024)
  ap.add_argument('--n', type=int, default=131072)
  ap.add_argument('--d', type=int, default=4096)
  ap.add_argument('--k', type=int, default=8)
  ap.add_argument('--chunk', type=int, default=16384)
  ap.add_argument('--reps', type=int, default=30)
  ap.add_argument('--warmup', type=int, default=2)
  ap.add_argument('--limit', type=int, default=240)
  ap.add_argument('--out', default=os.path.join('profiles', 'knn_bench.json'))
  args = ap.parse_args()
  if not torch.cuda.is_available():
    sys.exit('knn_bench: no GPU visible (there is no CPU path to time)')
  dev = 'cuda:0'
  gen = torch.Generator(device=dev).manual_seed(0)
  g = torch.randn(args.n, args.d, generator=gen, device=dev, dtype=torch.float32).to(torch.bfloat16)
  q = (g[torch.randint(0, args.n, (args.q,), generator=gen, device=dev)].float() +
       0.5 * torch.randn(args.q, args.d, generator=gen, device=dev)).to(torch.bfloat16)      # noisy copies: neighbours that mean something
  rows = [case('search', q, g, args.k, args.chunk, args.reps, args.warmup, args.limit),
          case('latency', q[:1].contiguous(), g, args.k, args.chunk, args.reps, args.warmup, args.limit)]
  result = dict(tool='tools/knn_bench.py', device=torch.cuda.get_device_name(0), torch=torch.__version__, splits=[ops.knn_plan(r['q'], r['n'], r['d'], r['k'])[0] for r in rows],
                cases=rows)
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'w') as fh:
    json.dump(result, fh, indent=1)
    fh.write('\n')
  for r in rows:
    print('%-8s Q %5d  fused %10.3f ms (%7.1f TFLOP/s)  composed %10.3f ms (%7.1f TFLOP/s)  fused / composed %.2f  idx equal %.4f'
          % (r['case'], r['q'], r['fused']['ms'], r['fused']['tflops'], r['composed']['ms'], r['composed']['tflops'], r['fused_over_composed'],
             r['idx_equal_fraction']))


if __name__ == '__main__':
  main()
