#!/usr/bin/env python
"""Times the --optimizer apply kernels (Config.optimizer; tg_optim_step) on the GPU next to Adam's at the same sizes:

  python tools/optim_bench.py [--launches 30] [--warmup 5] [--rounds 3] [--out profiles/optim_bench.json]
                              [--train adam,rmsprop,sgd] [--bench-line NAME=FILE ...]

  every rule x {plain, ema, guarded+ema}   on flat fp32 buffers of the largest optimiser group of BASELINE configs[3]
                                           (256x256, max_ch 256) and of one small size (65 536 elements)
  tg_adam_step, tg_adam_ema_step, tg_adam_ema_step_guarded   at the same sizes: the yardstick

Bytes per element: sgd 12, momentum / adagrad 20, rmsprop / adadelta / ftrl / adam 28, 8 more with the average.  HIP events
around every launch; successive launches of a case rotate through four copies of its buffers, so none is cache-resident.
--warmup untimed launches per case, then --rounds rounds that alternate the cases with --launches timed launches each: the
median per case and the spread of the per-round medians.  Per rule and form the achieved bytes/s is held against Adam's of
the same form and size minus the spread Adam's own rounds show (`verdicts`).  --train: ms per G+D step of configs[3] (bf16,
batch 16, hipGraph replay) with the named optimisers, the median of three timed regions -- a sanity figure, not a pass/fail.
--bench-line: the JSON result line(s) of a bench.py run kept in FILE, stored under `bench_lines`.  Every timed case runs under
a time limit of its own (--limit seconds, a watchdog that ends the process)."""
import argparse
import ctypes
import json
import os
import sys
import threading
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from twingan_amd import Config, _lib      # noqa: E402
from twingan_amd._lib import OPTIM_RULES, TgLossScaleState, TgOptimHyper, call      # noqa: E402
from twingan_amd.params import OPTIM_SLOTS, ParamStore, declare_twingan      # noqa: E402

HBM_PEAK = 8.0e12      # bytes / s, the MI355X's specified HBM3E bandwidth
SETS = 4                # copies of a case's buffers that successive launches rotate through
SMALL = 65536
FORMS = ('plain', 'ema', 'guarded_ema')


def largest_group():
  """-> (group, flat elements) of the largest optimiser group of configs[3], from the declarations alone (a CPU store)."""
  s3 = declare_twingan(ParamStore(torch.device('cpu')), Config(hw=256, max_ch=256)).build(0)
  flat = {g: s3.flat[g].numel() for g in s3.GROUPS}
  s3.close()
  g = max(flat, key=flat.get)
  return g, flat[g]


def limited(what, seconds, fn):
  def expire():
    sys.stderr.write('optim_bench: %s exceeded its limit of %d s\n' % (what, seconds))
    sys.stderr.flush()
    os._exit(124)
  t = threading.Timer(seconds, expire)
  t.daemon = True
  t.start()
  try:
    return fn()
  finally:
    t.cancel()


def median(ts):
  ts = sorted(ts)
  return ts[len(ts) // 2]


def timed_us(fn, launches):
  evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
  for e0, e1 in evs:
    e0.record()
    fn()
    e1.record()
  torch.cuda.synchronize()
  return [e0.elapsed_time(e1) * 1e3 for e0, e1 in evs]


def train_ms_per_step(rule, steps, warmup, regions=3):
  """configs[3] as bench.py runs it (bf16, batch 16, hipGraph replay, inputs in the static buffers) with Config.optimizer."""
  from twingan_amd.twingan import Trainer
  os.environ.setdefault('TG_STRICT_DISPATCH', '1')
  tr = Trainer(Config(hw=256, max_ch=256, precision='bf16', optimizer=rule), device='cuda:0', seed=0, use_graph=True)
  ga, gb = torch.Generator().manual_seed(1234), torch.Generator().manual_seed(4321)
  a = torch.rand(16, 256, 256, 3, generator=ga).to('cuda:0').to(torch.bfloat16).contiguous()
  b = torch.rand(16, 256, 256, 3, generator=gb).to('cuda:0').to(torch.bfloat16).contiguous()
  for _ in range(max(warmup, 1)):
    tr.run(a, b)
    tr.run(a, b)
  assert tr.use_graph, tr.graph_fallback_reason
  sa, sb = tr.static_inputs()
  sa.copy_(a)
  sb.copy_(b)
  out = []
  for _ in range(regions):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
      tr.run(sa, sb)
      tr.run(sa, sb)
    torch.cuda.synchronize()
    out.append(1e3 * (time.perf_counter() - t0) / steps)
  tr.close()
  del tr
  torch.cuda.empty_cache()
  return dict(optimizer=rule, ms_per_step=round(median(out), 3), ms_per_step_regions=[round(x, 3) for x in sorted(out)], steps=steps)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--launches', type=int, default=30)
  ap.add_argument('--warmup', type=int, default=5)
  ap.add_argument('--rounds', type=int, default=3)
  ap.add_argument('--limit', type=int, default=60)
  ap.add_argument('--train', default='', help='comma-separated optimisers to time a configs[3] step with')
  ap.add_argument('--train-steps', type=int, default=6)
  ap.add_argument('--bench-line', action='append', default=[], metavar='NAME=FILE')
  ap.add_argument('--out', default=None)
  args = ap.parse_args()
  assert args.launches >= 20, 'at least 20 timed launches per case'
  group, big = largest_group()
  assert torch.cuda.is_available(), 'needs a GPU'
  dev = torch.device('cuda:0')
  st = torch.cuda.current_stream().cuda_stream
  lr = torch.full((1,), 1e-4, dtype=torch.float32, device=dev)
  w = torch.full((1,), 1e-3, dtype=torch.float32, device=dev)
  state = TgLossScaleState(scale=1.0, seed=1.0, inv_scale=1.0, found=0, skip=0, good_steps=0, skipped=0)
  guard = torch.frombuffer(bytearray(bytes(state)), dtype=torch.int32).to(dev)
  hyper = {r: TgOptimHyper(lr=1e-4, momentum=0.9, decay_or_rho=0.95 if r == 'adadelta' else 0.9, eps=1e-8, lr_power=-0.5, l1=0.0,
                           l2=0.0) for r in OPTIM_RULES}
  cases = []      # (rule, form, numel, algorithmic bytes, launch)
  turn = [0]

  def rotate(sets, launch):
    def fn():
      turn[0] += 1
      launch(sets[turn[0] % len(sets)])
    return fn
  for n in (big, SMALL):
    sets = []
    for _ in range(SETS):      # theta, grad, two slots (positive: every rule's accumulators are), the average
      th, gr, s0, s1, avg = (torch.randn(n, device=dev) * 0.02 for _ in range(5))
      s0.abs_().add_(0.1)
      s1.abs_()
      sets.append([t.data_ptr() for t in (th, gr, s0, s1, avg)] + [(th, gr, s0, s1, avg)])
    g, lp, wp = guard.data_ptr(), lr.data_ptr(), w.data_ptr()
    cases.append(('adam', 'plain', n, 28 * n, rotate(sets, lambda p, n=n: call(
        'tg_adam_step', p[0], p[1], p[2], p[3], None, n, 0.0, lp, 0.5, 0.99, 1e-8, 1.0, st))))
    cases.append(('adam', 'ema', n, 36 * n, rotate(sets, lambda p, n=n: call(
        'tg_adam_ema_step', p[0], p[1], p[2], p[3], p[4], n, lp, 0.5, 0.99, 1e-8, 1.0, wp, st))))
    cases.append(('adam', 'guarded_ema', n, 36 * n, rotate(sets, lambda p, n=n: call(
        'tg_adam_ema_step_guarded', p[0], p[1], p[2], p[3], p[4], n, lp, 0.5, 0.99, 1e-8, g, wp, st))))
    for rule, rid in OPTIM_RULES.items():
      ns = len(OPTIM_SLOTS[rule])
      per = 12 + 8 * ns
      hp = ctypes.byref(hyper[rule])

      def launch(p, form, n=n, rid=rid, ns=ns, hp=hp):
        call('tg_optim_step', rid, p[0], p[1], p[2] if ns >= 1 else None, p[3] if ns >= 2 else None,
             p[4] if form != 'plain' else None, n, hp, 1.0, g if form == 'guarded_ema' else None, wp if form != 'plain' else None, st)
      for form in FORMS:
        cases.append((rule, form, n, (per + (0 if form == 'plain' else 8)) * n, rotate(sets, lambda p, form=form, launch=launch: launch(p, form))))

  name = lambda c: '%s:%s:%d' % c[:3]
  for c in cases:
    limited(name(c) + ' warm-up', args.limit, lambda fn=c[4]: ([fn() for _ in range(args.warmup)], torch.cuda.synchronize()))
  rounds = {name(c): [] for c in cases}
  for _ in range(args.rounds):      # the cases alternate: what drifts on a shared box drifts for all of them
    for c in cases:
      rounds[name(c)].append(median(limited(name(c), args.limit, lambda fn=c[4]: timed_us(fn, args.launches))))
  rows = {}
  for c in cases:
    r = rounds[name(c)]
    us = median(r)
    rows[name(c)] = dict(case=name(c), rule=c[0], form=c[1], numel=c[2], bytes=c[3], bytes_per_element=c[3] // c[2], us=us, us_rounds=r,
                         spread=(max(r) - min(r)) / us, gb_per_s=c[3] / us * 1e-3, gb_per_s_rounds=[c[3] / x * 1e-3 for x in r],
                         hbm_peak_fraction=c[3] / (us * 1e-6) / HBM_PEAK)
  verdicts = []
  for c in cases:
    if c[0] == 'adam':
      continue
    mine, adam = rows[name(c)], rows['adam:%s:%d' % (c[1], c[2])]
    floor = adam['gb_per_s'] - (max(adam['gb_per_s_rounds']) - min(adam['gb_per_s_rounds']))
    verdicts.append(dict(case=name(c), gb_per_s=mine['gb_per_s'], adam_gb_per_s=adam['gb_per_s'], adam_minus_spread=floor,
                         at_least_adam=mine['gb_per_s'] >= floor, us=mine['us'], adam_us=adam['us']))
  res = dict(device=torch.cuda.get_device_name(0), launches=args.launches, rounds=args.rounds, largest_group=group, numel=[big, SMALL],
             cases=list(rows.values()), verdicts=verdicts)
  del cases, sets
  torch.cuda.empty_cache()
  if args.train:
    res['train_config3'] = [limited('train ' + r, 600, lambda r=r: train_ms_per_step(r, args.train_steps, 2)) for r in args.train.split(',')]
  for item in args.bench_line:
    key, path = item.split('=', 1)
    res.setdefault('bench_lines', {})[key] = [json.loads(ln) for ln in open(path) if ln.startswith('{')]
  print(json.dumps(res), flush=True)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
      json.dump(res, f, indent=1)


if __name__ == '__main__':
  main()
