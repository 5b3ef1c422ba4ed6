#!/usr/bin/env python
"""Times the split (cross-replica) route of the batch normalisers next to the fused route they take on one clone
(Config.cross_replica_norm; include/twingan_hip_syncnorm.h):

  python tools/syncnorm_bench.py [--hw 256] [--max-ch 256] [--batch 3] [--reps 30] [--warmup 3] [--out profiles/syncnorm_bench.json]

  world 1   The normaliser calls of ONE generator-loss pass of the --hw batch_renorm configuration are recorded (a spy on the
            library calls: [passes, B*H, W, C] views, flags, pooled or not), and every distinct one is run both ways on
            resident tensors between two HIP events, forward (statistics + apply) and backward apart:
              fused   ops.instance_stats + ops.norm_act(stats=...)            (tg_instance_norm_stats, tg_norm_act_fwd / _bwd)
              split   the same with replicas=dp.ReplicaGather(1): moments, merge, forward / sums, apply; the gather of one
                      clone is a device copy, so what is timed is the route's launches without any wire
            After --warmup untimed runs the two are timed ALTERNATELY, --reps times each; median, least and greatest go to
            the JSON next to the algorithmic bytes of each route (tensor passes only).  These are launches of a few
            microseconds issued from python: the times include the host's launch gaps, as they do in the eager step.
  2 GPUs    where two are visible: two clones over RCCL, the eager step of the same configuration with the flag off and on
            (median of --step-reps steps after --warmup), and the all-gathers per step.  Otherwise that part is left out and
            the JSON says so.

Every timed part runs under a time limit of its own (--limit seconds, a watchdog that ends the process)."""
import argparse
import json
import os
import socket
import sys
import threading

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from twingan_amd import Config, _lib, ops      # noqa: E402
from twingan_amd.dp import ReplicaGather       # noqa: E402

DTYPES = {'bf16': torch.bfloat16, 'fp16': torch.float16, 'fp32': torch.float32}


def limited(what, seconds, fn):
  def expire():
    sys.stderr.write('syncnorm_bench: %s exceeded its limit of %d s\n' % (what, seconds))
    sys.stderr.flush()
    os._exit(124)
  t = threading.Timer(seconds, expire)
  t.daemon = True
  t.start()
  try:
    return fn()
  finally:
    t.cancel()


def _cfg(args, **kw):
  return Config(hw=args.hw, max_ch=args.max_ch, precision=args.precision, generator_norm_type='batch_renorm', **kw)


def recorded_shapes(args, dev):
  """-> ([(n, h, w, c, flags, pooled, calls)], gathers per generator-loss pass) of one pass of the configuration."""
  from twingan_amd import twingan as T
  tr = T.Trainer(_cfg(args), device=dev, seed=0)
  dt = DTYPES[args.precision]
  g = torch.Generator().manual_seed(0)
  s, t = (torch.rand(args.batch, args.hw, args.hw, 3, generator=g).to(dev).to(dt) for _ in range(2))
  seen, order = {}, []
  real = ops.call

  def spy(name, *a, **kw):
    if name == 'tg_norm_act_fwd' and not (a[15] & _lib.NF_NOSTATS):      # y, mean, rstd, gamma, beta, gamma2, beta2, split, rows, z, pn, n, h, w, c, flags
      order.append((a[11], a[12], a[13], a[14], a[15]))
    elif name == 'tg_pool2x2_fwd' and order and order[-1][:4] == tuple(a[2:6]):
      order[-1] = order[-1] + (True,)
    return real(name, *a, **kw)
  ops.call = spy
  try:
    with torch.no_grad():
      T.generator_loss(tr.P, s, t, tr.cfg)
  finally:
    ops.call = real
  torch.cuda.synchronize()
  for k in order:
    k = k if len(k) == 6 else k + (False,)
    seen[k] = seen.get(k, 0) + 1
  tr.close()
  return [k + (v,) for k, v in seen.items()], 2 * len(order)      # one gather forward, one backward per normalised layer


def time_shape(shape, dt, dev, reps, warmup):
  n, h, w, c, flags, pooled, calls = shape
  gen = torch.Generator(device=dev).manual_seed(1)
  y = torch.randn(n, h, w, c, generator=gen, device=dev).to(dt).requires_grad_(True)
  gz = torch.randn(n, h, w, c, generator=gen, device=dev).to(dt)
  gzp = torch.randn(n, h // 2, w // 2, c, generator=gen, device=dev).to(dt) if pooled else None
  ga = (1.0 + 0.1 * torch.randn(n, c, generator=gen, device=dev)).requires_grad_(True)
  be = (0.1 * torch.randn(n, c, generator=gen, device=dev)).requires_grad_(True)
  kw = dict(lrelu=bool(flags & _lib.NF_LRELU), pixel_norm=bool(flags & _lib.NF_PIXNORM), in_eps=1e-3, pool=pooled)
  rep = ReplicaGather(1)
  routes = {'fused': None, 'split': rep}

  def forward(r):
    st = ops.instance_stats(y.detach(), 1e-3, replicas=r)
    return ops.norm_act(y, ga, be, stats=st, replicas=r, **kw)

  def backward(out):
    y.grad = ga.grad = be.grad = None
    if pooled:
      torch.autograd.backward(list(out), [gz, gzp])
    else:
      out.backward(gz)
  ev = {(k, p): [] for k in routes for p in ('fwd', 'bwd')}
  for i in range(warmup + reps):
    for k, r in routes.items():
      e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
      e[0].record()
      out = forward(r)
      e[1].record()
      backward(out)
      e[2].record()
      if i >= warmup:
        ev[(k, 'fwd')].append((e[0], e[1]))
        ev[(k, 'bwd')].append((e[1], e[2]))
  torch.cuda.synchronize()
  es = y.element_size()
  numel = y.numel()
  pool_b = numel // 4 * es if pooled else 0
  # tensor passes: fused forward = statistics read + (read, write); backward = 2 reads of (gz, y) + write.  The split route
  # reads and writes the same tensors (its extra traffic is the [n][k][c] rows); its pooled output is a pass of its own.
  algo = {('fused', 'fwd'): 3 * numel * es + (5 * pool_b if pooled else 0), ('split', 'fwd'): 3 * numel * es + (5 * pool_b if pooled else 0),
          ('fused', 'bwd'): 5 * numel * es + 2 * pool_b, ('split', 'bwd'): 5 * numel * es + 2 * pool_b}
  row = dict(n=n, h=h, w=w, c=c, flags=flags, pooled=pooled, calls_per_pass=calls, dtype=str(dt), reps=reps, warmup=warmup,
             order='alternating', gathered_row_bytes=dict(fwd=n * 3 * c * 4, bwd=n * 2 * c * 4))
  for (k, p), pairs in ev.items():
    us = sorted(1e3 * a.elapsed_time(b) for a, b in pairs)
    row['%s_%s' % (k, p)] = dict(us=us[len(us) // 2], us_min=us[0], us_max=us[-1], bytes=algo[(k, p)])
  return row


def _step_worker(rank, port, args, flag, q):
  import datetime
  import torch.distributed as dist
  from twingan_amd.twingan import Trainer
  os.environ['MASTER_ADDR'], os.environ['MASTER_PORT'] = '127.0.0.1', str(port)
  dev = 'cuda:%d' % rank
  torch.cuda.set_device(dev)
  dist.init_process_group('nccl', rank=rank, world_size=2, timeout=datetime.timedelta(seconds=120))
  try:
    tr = Trainer(_cfg(args, cross_replica_norm=flag), device=dev, seed=0, world_size=2)
    dt = DTYPES[args.precision]
    g = torch.Generator().manual_seed(rank)
    s, t = (torch.rand(args.batch, args.hw, args.hw, 3, generator=g).to(dev).to(dt) for _ in range(2))
    for _ in range(2 * args.warmup):
      tr.run(s, t)
    if tr.replicas is not None:
      tr.replicas.reset_stats()
    ev = []
    for _ in range(args.step_reps):
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      e0.record()
      tr.run(s, t)
      e1.record()
      ev.append((e0, e1))
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    st = tr.replicas.stats() if tr.replicas is not None else dict(gather_bytes=0, collectives=0)
    if rank == 0:
      q.put(dict(flag=flag, step_ms=ms[len(ms) // 2], step_ms_min=ms[0], step_ms_max=ms[-1], steps=args.step_reps,
                 gathers_per_step=st['collectives'] / float(args.step_reps), gather_bytes_per_step=st['gather_bytes'] / float(args.step_reps)))
    dist.barrier()
  finally:
    dist.destroy_process_group()


def two_gpu_steps(args):
  import torch.multiprocessing as mp
  ctx = mp.get_context('spawn')
  rows = []
  for flag in (False, True):
    sk = socket.socket()
    sk.bind(('127.0.0.1', 0))
    port = sk.getsockname()[1]
    sk.close()
    q = ctx.Queue()
    procs = [ctx.Process(target=_step_worker, args=(r, port, args, flag, q)) for r in range(2)]
    try:
      for p in procs:
        p.start()
      rows.append(q.get(timeout=args.limit))
      for p in procs:
        p.join(timeout=120)
    finally:
      for p in procs:
        if p.is_alive():
          p.terminate()
          p.join(timeout=30)
  return rows


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--hw', type=int, default=256)
  ap.add_argument('--max-ch', dest='max_ch', type=int, default=256)
  ap.add_argument('--batch', type=int, default=3)      # runner.TWINGAN_HW_TO_BATCH_SIZE at 256 x 256
  ap.add_argument('--precision', default='bf16', choices=sorted(DTYPES))
  ap.add_argument('--reps', type=int, default=30)
  ap.add_argument('--warmup', type=int, default=3)
  ap.add_argument('--step-reps', dest='step_reps', type=int, default=10)
  ap.add_argument('--limit', type=int, default=240)
  ap.add_argument('--out', default=os.path.join('profiles', 'syncnorm_bench.json'))
  args = ap.parse_args()
  if not torch.cuda.is_available():
    sys.exit('syncnorm_bench: no GPU visible (there is no CPU path to time)')
  dev = 'cuda:0'
  torch.cuda.set_device(dev)
  shapes, gathers = limited('recording the shapes', args.limit, lambda: recorded_shapes(args, dev))
  shapes.sort(key=lambda k: (-k[1] * k[2], -k[3], k[0], k[5]))
  rows = [limited('shape %s' % (s,), args.limit, lambda s=s: time_shape(s, DTYPES[args.precision], dev, args.reps, args.warmup)) for s in shapes]
  tot = {k: sum(r[k]['us'] * r['calls_per_pass'] for r in rows) for k in ('fused_fwd', 'fused_bwd', 'split_fwd', 'split_bwd')}
  result = dict(tool='tools/syncnorm_bench.py', device=torch.cuda.get_device_name(0), torch=torch.__version__,
                config=dict(hw=args.hw, max_ch=args.max_ch, batch=args.batch, precision=args.precision, generator_norm_type='batch_renorm'),
                normalised_layers_per_generator_pass=gathers // 2, gathers_per_generator_step=gathers,
                per_generator_pass_us=tot, shapes=rows)
  if torch.cuda.device_count() >= 2:
    result['two_gpus'] = two_gpu_steps(args)
  else:
    result['two_gpus'] = None
    result['two_gpus_note'] = 'one GPU visible: the eager step with the flag on / off was not measured'
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'w') as fh:
    json.dump(result, fh, indent=1)
    fh.write('\n')
  for r in rows:
    print('[%d, %4d, %3d, %3d] flags %d pool %d x%d  fwd fused %7.1f us split %7.1f us   bwd fused %7.1f us split %7.1f us'
          % (r['n'], r['h'], r['w'], r['c'], r['flags'], r['pooled'], r['calls_per_pass'], r['fused_fwd']['us'], r['split_fwd']['us'],
             r['fused_bwd']['us'], r['split_bwd']['us']))
  print('one generator pass (%d normalised layers): fused %.0f + %.0f us, split %.0f + %.0f us (forward + backward), %d gathers per step'
        % (gathers // 2, tot['fused_fwd'], tot['fused_bwd'], tot['split_fwd'], tot['split_bwd'], gathers))
  if result['two_gpus']:
    for r in result['two_gpus']:
      print('two GPUs, flag %s: step %.2f ms, %.1f gathers per step' % (r['flag'], r['step_ms'], r['gathers_per_step']))


if __name__ == '__main__':
  main()
