#!/usr/bin/env python
"""Times ops.msssim (the fused MS-SSIM kernel) on the GPU: HIP events around warm calls, median of --calls.

  python tools/msssim_bench.py [--calls 30] [--out FILE.json]

Per shape it prints the whole five-level call, a one-level call (the level-0 launch + the two small kernels: an upper bound
of the level-0 launch; the launch alone is what `rocprofv3 --kernel-trace --stats -- python tools/msssim_bench.py` lists
under msssim_level_kernel<bf16 / f16>, the instantiation only level 0 uses) and the level-0 launch's algorithmic bytes
(both images read once in the storage type, the pooled pair written once in fp32) over that time against the 8 TB/s peak."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from twingan_amd import ops      # noqa: E402

PEAK_BYTES_PER_S = 8.0e12


def median_us(fn, calls, warmup=5):
  for _ in range(warmup):
    fn()
  torch.cuda.synchronize()
  ts = []
  for _ in range(calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    ts.append(e0.elapsed_time(e1) * 1e3)
  ts.sort()
  return ts[len(ts) // 2], ts[0], ts[-1]


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--calls', type=int, default=30)
  ap.add_argument('--out', default=None)
  args = ap.parse_args()
  assert torch.cuda.is_available(), 'needs a GPU'
  rows = []
  for (b, h, w, c), dt in (((64, 256, 256, 3), torch.bfloat16), ((64, 64, 64, 3), torch.bfloat16), ((64, 256, 256, 3), torch.float32),
                           ((64, 64, 64, 3), torch.float32)):
    g = torch.Generator(device='cuda').manual_seed(0)
    x = torch.rand(b, h, w, c, device='cuda', generator=g)
    y = (0.9 * x + 0.1 * torch.rand(b, h, w, c, device='cuda', generator=g)).to(dt)
    x = x.to(dt)
    full = median_us(lambda: ops.msssim(x, y, scale=255.), args.calls)
    one = median_us(lambda: ops.msssim(x, y, scale=255., weights=(1.0,)), args.calls)
    bytes0 = 2 * x.numel() * x.element_size() + 2 * (x.numel() // 4) * 4
    rows.append(dict(shape=[b, h, w, c], dtype=str(dt).split('.')[-1], calls=args.calls,
                     five_level_call_us=dict(median=full[0], min=full[1], max=full[2]),
                     one_level_call_us=dict(median=one[0], min=one[1], max=one[2]),
                     level0_algorithmic_bytes=bytes0, level0_bytes_per_s_upper_bound_time=bytes0 / (one[0] * 1e-6),
                     share_of_8TBps=bytes0 / (one[0] * 1e-6) / PEAK_BYTES_PER_S))
    print(json.dumps(rows[-1]), flush=True)
  if args.out:
    with open(args.out, 'w') as f:
      json.dump(rows, f, indent=1)


if __name__ == '__main__':
  main()
