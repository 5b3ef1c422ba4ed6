#!/usr/bin/env python
"""Times the training monitor (twingan_amd/monitor.py) on the GPU, on the trainer of BASELINE configs[3] as bench.py runs it
(256x256, max_ch 256, bf16, batch 16, hipGraph replay):

  python tools/monitor_bench.py [--launches 20] [--warmup 3] [--rounds 5] [--steps 6] [--out profiles/monitor_bench.json]

  (a) read_out        the launches of one full read-out -- every variable of both groups and one group's gradients through
                      tg_summary_multi, without the sample pass -- between two HIP events after --warmup untimed ones: the median
                      of --launches, next to bytes / HBM peak (the kernel reads every element once and is memory-shaped: the
                      bandwidth bound is the one that applies), and the same for each group's table alone
      grid_set        the eight grids of one logged step (8 forward runs of the sample pass, then 8 tg_image_grid_u8 launches),
                      the two parts timed apart; the grids' bound is (bytes read + bytes written) / HBM peak
  (b) ms_per_step     of that trainer with no monitor and with a monitor attached whose summaries and grids are never due,
                      alternated in one call: --rounds rounds of --steps G+D steps each way, host clock around a region that
                      ends in a synchronise; both medians and the spread of the rounds of the same code

Every timed part runs under a time limit of its own (--limit seconds, a watchdog that ends the process)."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import threading
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from twingan_amd import Config      # noqa: E402
from twingan_amd.monitor import Monitor      # noqa: E402

HBM_PEAK = 8.0e12      # bytes / s, the MI355X's specified HBM3E bandwidth


def limited(what, seconds, fn):
  def expire():
    sys.stderr.write('monitor_bench: %s exceeded its limit of %d s\n' % (what, seconds))
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


def timed_ms(fn, launches):
  evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
  for e0, e1 in evs:
    e0.record()
    fn()
    e1.record()
  torch.cuda.synchronize()
  return [e0.elapsed_time(e1) for e0, e1 in evs]


def row(name, ms, nbytes):
  m = median(ms)
  bound = nbytes / HBM_PEAK * 1e3
  return dict(case=name, ms=m, ms_min=min(ms), ms_max=max(ms), bytes=nbytes, hbm_bound_ms=bound, bound_by='HBM bandwidth',
              hbm_peak_fraction=bound / m, gb_per_s=nbytes / m * 1e-6)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--launches', type=int, default=20)
  ap.add_argument('--warmup', type=int, default=3)
  ap.add_argument('--rounds', type=int, default=5)
  ap.add_argument('--steps', type=int, default=6)
  ap.add_argument('--limit', type=int, default=120)
  ap.add_argument('--out', default=None)
  args = ap.parse_args()
  assert torch.cuda.is_available(), 'needs a GPU'
  from twingan_amd import ops
  from twingan_amd.twingan import Trainer
  os.environ.setdefault('TG_STRICT_DISPATCH', '1')
  dev = 'cuda:0'
  tr = Trainer(Config(hw=256, max_ch=256, precision='bf16'), device=dev, seed=0, use_graph=True)
  ga, gb = torch.Generator().manual_seed(1234), torch.Generator().manual_seed(4321)
  a = torch.rand(16, 256, 256, 3, generator=ga).to(dev).to(torch.bfloat16).contiguous()
  b = torch.rand(16, 256, 256, 3, generator=gb).to(dev).to(torch.bfloat16).contiguous()

  def warm():
    for _ in range(2):
      tr.run(a, b)
      tr.run(a, b)
    torch.cuda.synchronize()
  limited('warm-up steps', 600, warm)
  assert tr.use_graph, tr.graph_fallback_reason
  sa, sb = tr.static_inputs()
  sa.copy_(a)
  sb.copy_(b)
  tmp = tempfile.mkdtemp(prefix='monitor_bench_')
  mon = Monitor(sample_fn=lambda hw, n: (a, b), save_summaries_secs=1e9, log_image_every_n_iter=0).begin(tr, tmp, 16)
  res = dict(device=torch.cuda.get_device_name(0), launches=args.launches, rounds=args.rounds, steps=args.steps,
             variables={g: len(v) for g, v in mon.names.items()})

  # ---- (a) the read-out's launches and the grid set, device events -------------------------------------------------------------
  group = tr.last_run[0]
  tables = [('variables:' + g, mon._var_tables[g], 1.0) for g in tr.store.GROUPS] + [('gradients:' + group, mon._grad_tables[group], mon._grad_scale(group)[0])]
  buf = ops.SummaryBuffer(sum(t.njobs for _, t, _ in tables), tr.device)

  def read_out():
    r = 0
    for _, t, scale in tables:
      ops.tensor_summaries(table=t, scale=scale, out=buf, row=r)
      r += t.njobs
  cases = [('read_out', read_out, sum(t.nbytes for _, t, _ in tables))]
  for name, t, scale in tables:
    cases.append((name, lambda t=t, scale=scale: ops.tensor_summaries(table=t, scale=scale, out=buf, row=0), t.nbytes))
  rows = []
  for name, fn, nbytes in cases:
    limited(name + ' warm-up', args.limit, lambda fn=fn: ([fn() for _ in range(args.warmup)], torch.cuda.synchronize()))
    rows.append(row(name, limited(name, args.limit, lambda fn=fn: timed_ms(fn, args.launches)), nbytes))
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  buf.read()
  res['read_out_copy_ms'] = 1e3 * (time.perf_counter() - t0)      # host clock: the one device-to-host copy and its unpacking
  res['read_out_copy_bytes'] = int(buf.raw.numel())
  res['read_out_tensors'] = int(buf.n)
  runs = limited('sample pass', args.limit, lambda: mon._forward(8))
  torch.cuda.synchronize()
  grid_bytes = sum(r[k].numel() * r[k].element_size() for r in runs for k in
                   ('sources', 'targets', 's_prime_output', 't_prime_output', 's_cycle_output', 't_cycle_output')) * 5 // 3
  grid_bytes += 10 * 16 * 256 * 8 * 256 * 3      # six grids of 8 columns, two of 16
  limited('grids warm-up', args.limit, lambda: ([mon.render_grids(runs) for _ in range(args.warmup)], torch.cuda.synchronize()))
  rows.append(row('grid_set:8_grids', limited('grids', args.limit, lambda: timed_ms(lambda: mon.render_grids(runs), args.launches)),
                  grid_bytes))
  del runs
  fwd = limited('sample passes', 600, lambda: timed_ms(lambda: mon._forward(8), max(args.launches // 4, 3)))
  res['grid_set_forward_ms'] = dict(ms=median(fwd), ms_min=min(fwd), ms_max=max(fwd), runs_per_set=8,
                                    note='8 forward runs of the generators at batch 16: compute, no bandwidth bound stated')
  res['device_times'] = rows

  # ---- (b) ms per step without and with an attached monitor that does not fire -------------------------------------------------
  def region(with_monitor):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(args.steps):
      tr.run(sa, sb)
      tr.run(sa, sb)
      if with_monitor:
        mon.step(tr, 1000003 + k)      # never a multiple of anything that is due
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / args.steps
  limited('step warm-up', 600, lambda: (region(False), region(True)))
  plain, watched = [], []
  for _ in range(args.rounds):
    plain.append(limited('steps without monitor', 600, lambda: region(False)))
    watched.append(limited('steps with monitor', 600, lambda: region(True)))
  res['ms_per_step'] = dict(no_monitor=median(plain), monitor_attached=median(watched), no_monitor_rounds=plain, monitor_attached_rounds=watched,
                            spread_no_monitor=max(plain) - min(plain), spread_monitor_attached=max(watched) - min(watched),
                            difference=median(watched) - median(plain),
                            within_spread=abs(median(watched) - median(plain)) <= max(max(plain) - min(plain), max(watched) - min(watched)))
  mon.end()
  tr.close()
  shutil.rmtree(tmp, ignore_errors=True)
  print(json.dumps(res), flush=True)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
      json.dump(res, f, indent=1)


if __name__ == '__main__':
  main()
