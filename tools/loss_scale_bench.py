#!/usr/bin/env python
"""Times the optimiser tail with and without dynamic loss scaling (Config.dynamic_loss_scale) on the GPU, on flat fp32 buffers of
the sizes of the `g` and `d` groups of BASELINE configs[3] (256x256, max_ch 256) and configs[4] (+ self-attention at 64,
spectrally normalised discriminators):

  python tools/loss_scale_bench.py [--launches 30] [--warmup 5] [--rounds 3] [--out FILE.json]

  static            tg_adam_tick + tg_adam_step                                        28 bytes per element
  dynamic           tg_nonfinite_check + tg_loss_scale_tick + tg_adam_step_guarded     4 + 28
  dynamic_skipped   the same with an inf in the gradient: the apply stores nothing     4
  fused_*           the three again with the fused average (tg_adam_ema_step[_guarded]) 36, 4 + 36, 4 + 12
  check, ema        tg_nonfinite_check and tg_ema_update alone: the two streaming kernels' rates side by side (4 and 12)

HIP events around every case (its two or three launches together, boundaries included: what an apply costs the step);
successive launches of a case rotate through four copies of its buffers, so none is cache-resident.  --warmup untimed
launches per case, then --rounds rounds that alternate the cases with --launches timed launches each: the median per case and
the spread of the per-round medians.  Reported per case: microseconds, GB/s of algorithmic bytes, the fraction of the 8 TB/s
HBM peak; per group dynamic / static against the (4 + 28) / 28 and (4 + 36) / 36 the byte counts predict.  Every timed case
runs under a time limit of its own (--limit seconds, a watchdog that ends the process)."""
import argparse
import json
import os
import sys
import threading

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from twingan_amd import Config      # noqa: E402
from twingan_amd._lib import TgLossScaleState, call      # noqa: E402
from twingan_amd.params import ParamStore, declare_twingan      # noqa: E402

HBM_PEAK = 8.0e12      # bytes / s, the MI355X's specified HBM3E bandwidth
SETS = 4                # copies of a group's buffers that successive launches rotate through
B1, B2, EPS, LR = 0.5, 0.99, 1e-8, 1e-4
CONFIGS = {'c3': dict(), 'c4': dict(do_self_attention=True, self_attention_hw=64, spectral_norm=True)}


def sizes():
  """-> {'c3:g': flat elements, ...} from the declarations alone (CPU stores)."""
  out = {}
  for name, kw in CONFIGS.items():
    s = declare_twingan(ParamStore(torch.device('cpu')), Config(hw=256, max_ch=256, **kw)).build(0)
    out.update({'%s:%s' % (name, g): s.flat[g].numel() for g in s.GROUPS})
    s.close()
  return out


def limited(what, seconds, fn):
  def expire():
    sys.stderr.write('loss_scale_bench: %s exceeded its limit of %d s\n' % (what, seconds))
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
  flat = sizes()
  assert torch.cuda.is_available(), 'needs a GPU'
  dev = torch.device('cuda:0')
  st = torch.cuda.current_stream().cuda_stream
  w = torch.full((1,), 1e-3, dtype=torch.float32, device=dev)
  cases = []      # (name, algorithmic bytes, launch)
  turn = [0]
  keep = []

  def scalars():
    """A step counter, a rate and a loss-scale state (S = 128, an interval no run reaches) of a case's own."""
    step, lr = torch.zeros(1, dtype=torch.int64, device=dev), torch.full((1,), LR, dtype=torch.float32, device=dev)
    ls = torch.frombuffer(bytearray(bytes(TgLossScaleState(scale=128.0, seed=128.0, inv_scale=1.0 / 128.0))), dtype=torch.int32).to(dev)
    keep.extend((step, lr, ls))
    return step.data_ptr(), lr.data_ptr(), ls.data_ptr()

  def rotate(sets, launch):
    def fn():
      turn[0] += 1
      launch(sets[turn[0] % len(sets)])
    return fn

  def static(n, fused):
    step, lr, _ = scalars()

    def launch(p):
      call('tg_adam_tick', step, lr, LR, B1, B2, st)
      if fused:
        call('tg_adam_ema_step', p[0], p[1], p[2], p[3], p[4], n, lr, B1, B2, EPS, 1.0 / 128.0, w.data_ptr(), st)
      else:
        call('tg_adam_step', p[0], p[1], p[2], p[3], None, n, 0.0, lr, B1, B2, EPS, 1.0 / 128.0, st)
    return launch

  def dynamic(n, fused, grad):
    step, lr, ls = scalars()

    def launch(p):
      call('tg_nonfinite_check', p[grad], n, ls, st)
      call('tg_loss_scale_tick', ls, step, lr, LR, B1, B2, 1 << 30, 2.0 ** 24, 1, st)
      if fused:
        call('tg_adam_ema_step_guarded', p[0], p[grad], p[2], p[3], p[4], n, lr, B1, B2, EPS, ls, w.data_ptr(), st)
      else:
        call('tg_adam_step_guarded', p[0], p[grad], p[2], p[3], n, lr, B1, B2, EPS, ls, st)
    return launch
  for g, n in flat.items():
    sets = []
    for _ in range(SETS):
      th, gr, m, v, avg, bad = (torch.randn(n, device=dev) * 0.02 for _ in range(6))
      v.abs_()
      gr.mul_(128.0)
      bad[n // 2] = float('inf')      # the gradient of the skipped cases
      sets.append([t.data_ptr() for t in (th, gr, m, v, avg, bad)] + [(th, gr, m, v, avg, bad)])
    _, _, ls = scalars()
    for fused, tag, nb in ((False, '', 28), (True, 'fused_', 36)):
      cases.append(('%sstatic:%s:%d' % (tag, g, n), nb * n, rotate(sets, static(n, fused))))
      cases.append(('%sdynamic:%s:%d' % (tag, g, n), (4 + nb) * n, rotate(sets, dynamic(n, fused, 1))))
      cases.append(('%sdynamic_skipped:%s:%d' % (tag, g, n), (4 + (12 if fused else 0)) * n, rotate(sets, dynamic(n, fused, 5))))
    cases.append(('check:%s:%d' % (g, n), 4 * n, rotate(sets, lambda p, n=n, ls=ls: call('tg_nonfinite_check', p[1], n, ls, st))))
    cases.append(('ema:%s:%d' % (g, n), 12 * n, rotate(sets, lambda p, n=n: call('tg_ema_update', p[4], p[0], n, w.data_ptr(), st))))

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
  by = {r['case'].rsplit(':', 1)[0]: r for r in rows}
  ratios = {}
  for g in flat:
    ratios[g] = dict(dynamic_over_static=by['dynamic:' + g]['us'] / by['static:' + g]['us'], expected_from_bytes=32.0 / 28.0,
                     fused_dynamic_over_static=by['fused_dynamic:' + g]['us'] / by['fused_static:' + g]['us'],
                     fused_expected_from_bytes=40.0 / 36.0,
                     added_us=by['dynamic:' + g]['us'] - by['static:' + g]['us'],
                     check_gb_per_s=by['check:' + g]['gb_per_s'], ema_gb_per_s=by['ema:' + g]['gb_per_s'])
  res = dict(device=torch.cuda.get_device_name(0), launches=args.launches, rounds=args.rounds, cases=rows, ratios=ratios)
  print(json.dumps(res), flush=True)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
      json.dump(res, f, indent=1)


if __name__ == '__main__':
  main()
