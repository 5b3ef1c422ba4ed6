#!/usr/bin/env python
"""Times the sliced Wasserstein evaluation (evaluate.SlicedWasserstein over the ops.swd_* kernels) on the GPU against the
model that produces the images it scores: HIP events around warm calls, median of --calls.

  python tools/swd_bench.py [--hw 256] [--images 1024] [--batch 16] [--calls 5] [--out FILE.json]

Measured, all on one device in one process:
  feed            one minibatch of reals and fakes (two pyramids, two gathers per level), median over the feeds of a pass
  end             the whole read-out (both columns, every level), and per level its stages on the `fake` column: projection of
                  both sets (statistics included), column sort of both, mean |difference|
  translate       twingan.translate for the same number of images in the same batches (what produces the fakes)
  framework_end   the same read-out composed from torch.matmul + torch.sort (normalised descriptors written out)
The condition DESIGN.md section 4 states: feeds + end <= translate, i.e. the evaluation stays bound by the model.  Every timed
step runs under a time limit of its own (--limit seconds, a watchdog that ends the process)."""
import argparse
import json
import os
import sys
import threading

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from twingan_amd import Config, ops      # noqa: E402
from twingan_amd.evaluate import SlicedWasserstein      # noqa: E402
from twingan_amd.params import ParamStore, declare_twingan      # noqa: E402
from twingan_amd.twingan import translate      # noqa: E402


def limited(what, seconds, fn):
  """Runs fn(); a step that has not come back after `seconds` ends the process (exit status 124) instead of hanging it."""
  def expire():
    sys.stderr.write('swd_bench: %s exceeded its limit of %d s\n' % (what, seconds))
    sys.stderr.flush()
    os._exit(124)
  t = threading.Timer(seconds, expire)
  t.daemon = True
  t.start()
  try:
    return fn()
  finally:
    t.cancel()


def timed_ms(fn):
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  e0.record()
  out = fn()
  e1.record()
  e1.synchronize()
  return e0.elapsed_time(e1), out


def median(ts):
  ts = sorted(ts)
  return ts[len(ts) // 2]


def framework_distance(a, b, dirs):
  def keys(x):
    v = x.view(-1, 3, 49)
    std, mean = torch.std_mean(v.double(), dim=(0, 2), unbiased=False)
    xn = ((v - mean.float().view(1, 3, 1)) / std.float().view(1, 3, 1)).view(-1, ops.SWD_K)
    return torch.sort(torch.matmul(xn, dirs), dim=1).values      # [R, N, D] sorted over N
  return (keys(a) - keys(b)).abs().mean()


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--hw', type=int, default=256)
  ap.add_argument('--images', type=int, default=1024)
  ap.add_argument('--batch', type=int, default=16)
  ap.add_argument('--max-ch', type=int, default=256)
  ap.add_argument('--calls', type=int, default=5)
  ap.add_argument('--limit', type=int, default=120)
  ap.add_argument('--out', default=None)
  args = ap.parse_args()
  assert torch.cuda.is_available(), 'needs a GPU'
  dev, dt = torch.device('cuda:0'), torch.bfloat16
  g = torch.Generator(device='cuda').manual_seed(0)
  nb = args.images // args.batch
  reals = [torch.rand(args.batch, args.hw, args.hw, 3, device=dev, generator=g).to(dt) for _ in range(2)]
  acc = SlicedWasserstein(args.hw, args.images)

  def one_pass():
    acc.begin()
    return [timed_ms(lambda: acc.feed(reals[i % 2], reals[(i + 1) % 2]))[0] for i in range(nb)]
  limited('feed warm-up', args.limit, one_pass)
  feeds = [t for _ in range(args.calls) for t in limited('feed', args.limit, one_pass)]

  dirs = [d.to(dev) for d in acc.draw_dirs()]
  limited('end warm-up', args.limit, lambda: acc.distances(dirs))
  torch.cuda.synchronize()
  end = [limited('end', args.limit, lambda: timed_ms(lambda: acc.distances(dirs))[0]) for _ in range(args.calls)]
  n = acc.count * acc.per
  levels = []
  for l, (dr, df) in enumerate(acc.desc):
    row = dict(resolution=acc.resolutions[l], descriptors=n)
    for _ in range(2):      # the second round is the warm one
      row['project_ms'], (pa, pb) = limited('project', args.limit, lambda: timed_ms(
          lambda: (ops.swd_project(dr[:n], dirs[l])[0], ops.swd_project(df[:n], dirs[l])[0])))
      row['sort_ms'], _ = limited('sort', args.limit, lambda: timed_ms(lambda: (ops.swd_sort_columns(pa), ops.swd_sort_columns(pb))))
      row['diff_ms'], _ = limited('diff', args.limit, lambda: timed_ms(lambda: ops.swd_mean_abs_diff(pa, pb, n, acc.repeats)))
    del pa, pb
    levels.append(row)

  def framework_end():
    out = []
    for l, (dr, df) in enumerate(acc.desc):
      out.append(framework_distance(dr[:n], df[:n], dirs[l]))
      out.append(framework_distance(dr[:n // 2], dr[n // 2:n], dirs[l]))
    return out
  limited('framework warm-up', args.limit, framework_end)
  torch.cuda.synchronize()
  fw = [limited('framework end', args.limit, lambda: timed_ms(framework_end)[0]) for _ in range(args.calls)]
  ours = [float(t) for pair in acc.distances(dirs) for t in pair]
  theirs = [float(t) for t in framework_end()]
  fw_sort = [limited('framework sort', args.limit, lambda: timed_ms(
      lambda: torch.sort(torch.empty(acc.repeats * acc.dirs, ops.swd_npad(n), device=dev).normal_(), dim=1))[0]) for _ in range(3)]

  cfg = Config(hw=args.hw, max_ch=args.max_ch, precision='bf16')
  store = declare_twingan(ParamStore(dev), cfg).build(0)

  def translate_all():
    with torch.no_grad():
      for i in range(nb):
        translate(store.P, reals[i % 2], cfg, 't', None)
  limited('translate warm-up', args.limit, lambda: (translate_all(), torch.cuda.synchronize()))
  tr = [limited('translate', args.limit, lambda: timed_ms(translate_all)[0]) for _ in range(args.calls)]
  store.close()

  feed_ms, end_ms, tr_ms, fw_ms = median(feeds), median(end), median(tr), median(fw)
  res = dict(hw=args.hw, images=args.images, batch=args.batch, dtype='bf16', per=acc.per, repeats=acc.repeats, dirs=acc.dirs,
             calls=args.calls, sort_block=ops.SWD_SORT_BLOCK, feed_ms_per_minibatch=feed_ms, feeds_ms_total=feed_ms * nb,
             end_ms=end_ms, end_levels=levels, translate_ms_total=tr_ms, evaluation_over_translate=(feed_ms * nb + end_ms) / tr_ms,
             stays_model_bound=bool(feed_ms * nb + end_ms <= tr_ms), framework_end_ms=fw_ms, end_over_framework_end=end_ms / fw_ms,
             framework_sort_one_set_ms=median(fw_sort), distances_x1e3=[v * 1e3 for v in ours],
             framework_distances_x1e3=[v * 1e3 for v in theirs])
  print(json.dumps(res), flush=True)
  if args.out:
    with open(args.out, 'w') as f:
      json.dump(res, f, indent=1)


if __name__ == '__main__':
  main()
