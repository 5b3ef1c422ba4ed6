#!/usr/bin/env python
"""Times the moving-average kernels (Config.moving_average_decay) on the GPU at the sizes the trainer launches them with:

  python tools/ema_bench.py [--launches 30] [--warmup 5] [--rounds 3] [--out FILE.json]

  tg_adam_step, tg_adam_ema_step, tg_ema_update   on flat fp32 buffers of the `g` and `d` groups of BASELINE configs[3]
                                                  (256x256, max_ch 256): 28, 36 and 12 bytes per element
  tg_ema_update_multi                             on the state table of configs[2] with batch renorm (128x128, max_ch 256):
                                                  separately allocated tensors, 12 bytes per element

HIP events around every launch; successive launches of a case rotate through four copies of its buffers, so none is
cache-resident.  --warmup untimed launches per case, then --rounds rounds that alternate the cases with --launches timed
launches each: the median per case, and the spread of the per-round medians (what a difference between two cases has to
exceed).  Reported per case: microseconds, achieved GB/s from the algorithmic bytes, the fraction of the 8 TB/s
HBM peak, and fused / (adam + ema) -- the fused kernel is kept for the applied group only if that ratio is below 1.
Every timed case runs under a time limit of its own (--limit seconds, a watchdog that ends the process)."""
import argparse
import ctypes
import json
import os
import sys
import threading

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from twingan_amd import Config, _lib      # noqa: E402
from twingan_amd._lib import call      # noqa: E402
from twingan_amd.params import ParamStore, declare_twingan, is_model_variable      # noqa: E402

HBM_PEAK = 8.0e12      # bytes / s, the MI355X's specified HBM3E bandwidth
SETS = 4                # copies of a group's buffers that successive launches rotate through


def sizes():
  """-> ({group: flat elements} of configs[3], [state variable elements] of configs[2] under batch renorm), from the
  declarations alone (CPU stores)."""
  s3 = declare_twingan(ParamStore(torch.device('cpu')), Config(hw=256, max_ch=256)).build(0)
  flat = {g: s3.flat[g].numel() for g in s3.GROUPS}
  s3.close()
  s2 = declare_twingan(ParamStore(torch.device('cpu')), Config(hw=128, max_ch=256, generator_norm_type='batch_renorm'))
  state = [int(torch.Size((n,) if isinstance(n, int) else n).numel()) for k, (n, _) in s2.state_specs.items() if is_model_variable(k)]
  return flat, state


def limited(what, seconds, fn):
  def expire():
    sys.stderr.write('ema_bench: %s exceeded its limit of %d s\n' % (what, seconds))
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


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--launches', type=int, default=30)
  ap.add_argument('--warmup', type=int, default=5)
  ap.add_argument('--rounds', type=int, default=3)
  ap.add_argument('--limit', type=int, default=60)
  ap.add_argument('--out', default=None)
  args = ap.parse_args()
  assert args.launches >= 20, 'at least 20 timed launches per case'
  flat, state = sizes()
  assert torch.cuda.is_available(), 'needs a GPU'
  dev = torch.device('cuda:0')
  st = torch.cuda.current_stream().cuda_stream
  lr = torch.full((1,), 1e-4, dtype=torch.float32, device=dev)
  w = torch.full((1,), 1e-3, dtype=torch.float32, device=dev)
  cases = []      # (name, algorithmic bytes, launch)
  turn = [0]

  def rotate(sets, launch):
    """Successive launches of a case go round SETS copies of its buffers, so that a launch finds none of its 140-180 MB in
    the 256 MB Infinity Cache -- as in a training step, where gigabytes stream between two applies."""
    def fn():
      turn[0] += 1
      launch(sets[turn[0] % len(sets)])
    return fn
  for g, n in flat.items():
    sets = []
    for _ in range(SETS):
      th, gr, m, v, avg = (torch.randn(n, device=dev) * 0.02 for _ in range(5))
      v.abs_()
      sets.append([t.data_ptr() for t in (th, gr, m, v, avg)] + [(th, gr, m, v, avg)])
    cases.append(('adam_step:%s:%d' % (g, n), 28 * n, rotate(sets, lambda p, n=n: call(
        'tg_adam_step', p[0], p[1], p[2], p[3], None, n, 0.0, lr.data_ptr(), 0.5, 0.99, 1e-8, 1.0, st))))
    cases.append(('adam_ema_step:%s:%d' % (g, n), 36 * n, rotate(sets, lambda p, n=n: call(
        'tg_adam_ema_step', p[0], p[1], p[2], p[3], p[4], n, lr.data_ptr(), 0.5, 0.99, 1e-8, 1.0, w.data_ptr(), st))))
    cases.append(('ema_update:%s:%d' % (g, n), 12 * n, rotate(sets, lambda p, n=n: call(
        'tg_ema_update', p[4], p[0], n, w.data_ptr(), st))))
  pairs = [(torch.randn(n, device=dev), torch.randn(n, device=dev)) for n in state]
  host = ctypes.create_string_buffer(_lib.load().tg_ema_table_bytes(len(pairs)))
  blocks = ctypes.c_int32(0)
  for j, (a, x) in enumerate(pairs):
    call('tg_ema_table_fill', a.data_ptr(), x.data_ptr(), a.numel(), j, ctypes.addressof(host), ctypes.byref(blocks))
  tab = torch.frombuffer(bytearray(host.raw), dtype=torch.uint8).to(dev)
  cases.append(('ema_update_multi:%djobs:%d' % (len(pairs), sum(state)), 12 * sum(state), lambda: call(
      'tg_ema_update_multi', tab.data_ptr(), len(pairs), blocks.value, w.data_ptr(), st)))

  for name, _, fn in cases:
    limited(name + ' warm-up', args.limit, lambda fn=fn: ([fn() for _ in range(args.warmup)], torch.cuda.synchronize()))
  rounds = {name: [] for name, _, _ in cases}
  for _ in range(args.rounds):      # the cases alternate: what drifts on a shared box drifts for all of them
    for name, _, fn in cases:
      rounds[name].append(median(limited(name, args.limit, lambda fn=fn: timed_us(fn, args.launches))))
  rows = []
  for name, nbytes, _ in cases:
    us = median(rounds[name])
    rows.append(dict(case=name, bytes=nbytes, us=us, us_rounds=rounds[name], spread=(max(rounds[name]) - min(rounds[name])) / us,
                     gb_per_s=nbytes / us * 1e-3, hbm_peak_fraction=nbytes / (us * 1e-6) / HBM_PEAK))
  by = {r['case'].split(':')[0] + ':' + r['case'].split(':')[1]: r for r in rows}
  ratios = {}
  for g in flat:
    a, f, e = by['adam_step:' + g]['us'], by['adam_ema_step:' + g]['us'], by['ema_update:' + g]['us']
    ratios[g] = dict(fused_over_adam=f / a, expected_from_bytes=36.0 / 28.0, fused_over_adam_plus_ema=f / (a + e))
  # a G run applies g (fused) and averages d and the state; a D run the other way round; against two plain Adam applies
  added = sum(by['adam_ema_step:' + g]['us'] - by['adam_step:' + g]['us'] + by['ema_update:' + g]['us'] for g in flat)
  res = dict(device=torch.cuda.get_device_name(0), launches=args.launches, rounds=args.rounds, cases=rows, ratios=ratios,
             added_us_per_g_plus_d_step_flat=added, state_us_per_run=rows[-1]['us'],
             added_us_per_g_plus_d_step=added + 2 * rows[-1]['us'])
  print(json.dumps(res), flush=True)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
      json.dump(res, f, indent=1)


if __name__ == '__main__':
  main()
