"""Cross-replica batch statistics (Config.cross_replica_norm; include/twingan_hip_syncnorm.h).

1. tg_norm_moments + tg_norm_moments_merge against float64 of the stored inputs, R replicas emulated in one process; the bound
   is twice the error of the unchanged tg_instance_norm_stats on the same data viewed as one group, plus 4 fp32 ulp of the value.
2. tg_norm_act_bwd_sums + tg_norm_act_bwd_apply (and tg_norm_act_fwd on the merged statistics) element by element against
   tests/elementwise.py's norm_act_reference on the concatenated single-group view, with the bounds of the fused path.
3. Two clones on one GPU over gloo: the clones' outputs, summed gradients and state against ONE clone on the concatenated
   batch with the flag off; a Trainer's clones end with equal parameters and bit-identical state (and do not with the flag off).

1 and 2 also run over the emulated kernels (TG_EMU=1); 3 starts two child processes once for the whole module."""
import os
import sys
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import elementwise as E      # noqa: E402

EW_DTYPES = {'f32': torch.float32, 'bf16': torch.bfloat16, 'f16': torch.float16}
BN_EPS = 1e-3      # the batch normalisers' epsilon (pggan.BN_EPS)
FP32_GRAD_TOL = 5e-3         # tests/test_gpu_model.py: whole-model fp32 gradients, aggregate rel-L2 over a group ...
FP32_VAR_GRAD_TOL = 2e-2     # ... and every single variable of non-negligible norm (sized against the float64 oracle)


def dev():
  return torch.device('cuda:0')


def host(t):
  return t.detach().float().cpu().numpy().astype(np.float64)


def _round_to(a, dtype):
  t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
  return t.float().to(dtype).double().cpu()


def _f32(n, dv=None):
  return torch.empty(n, dtype=torch.float32, device=dv or dev())


# ------------------------------------------------------------------------------------------------ raw entry points
def _moments(O, y):
  from twingan_amd import _lib
  n, h, w, c = y.shape
  ws = _f32(n * _lib.load().tg_norm_chunks(n, h, w) * 2 * c)
  mom = _f32((n, 3, c))
  O.call('tg_norm_moments', O._p(y), O._p(mom), O._p(ws), n, h, w, c, O._dt(y), O._stream())
  return mom


def _merge(O, gathered, count, eps):
  R, n, _, c = gathered.shape
  mean, rstd = _f32(n * c), _f32(n * c)
  O.call('tg_norm_moments_merge', O._p(gathered), R, count, O._p(mean), O._p(rstd), n, c, eps, O._stream())
  return mean, rstd


# ------------------------------------------------------------------------------------------------ 1. moments and merge
MOMENT_CASES = [
    # id, per-replica view (b*h, w), c, groups n, chunks of tg_norm_chunks (1: one chunk; 5 = 4 x 64 + a tail of 4; 64: several)
    ('one_chunk_c32_n4', 4, 4, 32, 4, 1), ('one_chunk_c5_scalar_n1', 4, 4, 5, 1, 1), ('one_chunk_c8_n2', 4, 4, 8, 2, 1),
    ('tail_chunk_c256_n2', 10, 26, 256, 2, 5), ('tail_chunk_c24_scalar_n4', 10, 26, 24, 4, 5), ('tail_chunk_c3_scalar_n1', 10, 26, 3, 1, 5),
    ('64_chunks_c8_n1', 64, 64, 8, 1, 64), ('64_chunks_c32_n2', 64, 64, 32, 2, 64), ('64_chunks_c5_scalar_n4', 64, 64, 5, 4, 64),
]


@pytest.mark.parametrize('dname', sorted(EW_DTYPES))
@pytest.mark.parametrize('case', MOMENT_CASES, ids=[c[0] for c in MOMENT_CASES])
def test_moments_merge_against_float64(case, dname):
  """R in {1, 2, 3, 8} replicas of [n, b*h, w, c], two kinds of data each: ordinary activations, and a large offset (fp32:
  mean 300, sigma 0.05; 16-bit: mean 8, sigma 0.25) where raw sums and sums of squares would cancel.  Reference: float64 mean
  and rsqrt(var + eps) of the stored values of the concatenation [n, R*b*h, w, c].  Bound per (group, channel): 2 x the worst
  error of tg_instance_norm_stats (unchanged from before this route existed) on that concatenation, + 4 fp32 ulp of the value.

  Measured on an MI355X, worst error / bound over the nine shapes, R and both statistics: fp32 0.47 (activations), 0.23
  (offset); bf16 0.39, 0.21; fp16 0.36, 0.16 -- the table of DESIGN.md section 4 is this test's printed output.  With the mean
  gathered as ONE fp32 word the offset data missed the bound in fp32 by up to 79 x (16 pixels per replica; 1.6 x at 4096): the
  rounding of each replica's mean enters the merged variance, which is why tg_norm_moments writes the mean as a pair."""
  import twingan_amd.ops as O
  from twingan_amd import _lib
  name, bh, w, c, n, chunks = case
  dtype = EW_DTYPES[dname]
  assert _lib.load().tg_norm_chunks(n, bh, w) == chunks, 'norm_chunks moved: the case ids name stale branches'
  bad = []
  for R in (1, 2, 3, 8):
    for kind in ('plain', 'offset'):
      rng = np.random.RandomState(zlib.crc32(('%s %s %d %s' % (name, dname, R, kind)).encode()) % (2 ** 31))
      if kind == 'plain':
        y = rng.randn(R, n, bh, w, c) * 1.5 + 0.7 + 0.5 * rng.randn(1, 1, 1, 1, c)
      else:
        mu, sd = (300.0, 0.05) if dtype == torch.float32 else (8.0, 0.25)
        y = mu + sd * rng.randn(R, n, bh, w, c)
      y = _round_to(y, dtype)                                                # the stored inputs, float64
      cat = y.permute(1, 0, 2, 3, 4).reshape(n, R * bh, w, c).contiguous()   # one clone on the concatenated batch
      m64 = cat.mean(dim=(1, 2)).numpy().reshape(-1)
      r64 = (1.0 / np.sqrt(cat.numpy().var(axis=(1, 2)) + BN_EPS)).reshape(-1)
      me, re = O.instance_stats(cat.to(dev()).to(dtype), BN_EPS)
      yd = y.to(dev()).to(dtype)
      gathered = torch.stack([_moments(O, yd[r].contiguous()) for r in range(R)]).contiguous()
      mm, rm = _merge(O, gathered, bh * w, BN_EPS)
      torch.cuda.synchronize()
      for what, got, old, ref in (('mean', mm, me, m64), ('rstd', rm, re, r64)):
        e_old = np.abs(host(old) - ref).max()
        err = np.abs(host(got) - ref)
        bound = 2.0 * e_old + 4.0 * np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
        ratio = float((err / bound).max())
        print('[syncnorm moments] %-26s %-4s R=%d %-6s %s: existing kernel %.3e, merged %.3e, worst error / bound %.3f'
              % (name, dname, R, kind, what, e_old, err.max(), ratio))
        if not ratio <= 1.0:
          bad.append((R, kind, what, float(e_old), float(err.max()), ratio))
  assert not bad, bad


def test_merge_is_rank_ordered_and_refuses_bad_counts():
  """The merge reads rows 0 .. R-1 in order and nothing else; a count of 0, no replicas, or R * count >= 2^31 are errors."""
  import twingan_amd.ops as O
  from twingan_amd import _lib
  rng = np.random.RandomState(3)
  g = torch.from_numpy(np.abs(rng.randn(3, 2, 3, 5)).astype(np.float32)).to(dev())
  a = _merge(O, g, 7, BN_EPS)
  b = _merge(O, g.clone(), 7, BN_EPS)
  torch.cuda.synchronize()
  assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
  mean = (host(g)[:, :, 0, :] + host(g)[:, :, 1, :]).mean(axis=0).reshape(-1)
  assert np.abs(host(a[0]) - mean).max() < 1e-6
  for R, count in ((0, 7), (3, 0), (3, 2 ** 30)):
    with pytest.raises(_lib.TgError, match='outside'):
      O.call('tg_norm_moments_merge', O._p(g), R, count, O._p(a[0]), O._p(a[1]), 2, 5, BN_EPS, O._stream())


def test_only_the_split_route_refuses_constant_statistics():
  """The backward entry points share their argument checks, not this one: constant statistics (NF_NOSTATS: ops.pixel_norm,
  ops.affine_act) have no sums to share, so tg_norm_act_bwd_sums / tg_norm_act_bwd_apply refuse them, while the fused
  tg_norm_act_bwd runs them.  A pooled gradient over an odd height is refused by both routes."""
  import twingan_amd.ops as O
  from twingan_amd import _lib
  lib = _lib.load()

  def routes(h, w, pooled, flags):
    n, c = 1, 8
    rng = np.random.RandomState(17)
    t = lambda *shape: torch.from_numpy(rng.randn(*shape).astype(np.float32)).to(dev())
    y, gz, gy = t(n, h, w, c), t(n, h, w, c), torch.full((n, h, w, c), float('nan'), device=dev())
    gzp = t(n, h // 2, w // 2, c) if pooled else None
    one, zero = torch.ones(n * c, device=dev()), torch.zeros(n * c, device=dev())
    ws, local = _f32(n * lib.tg_norm_chunks(n, h, w) * 2 * c), _f32((n, 2, c))
    common = (O._p(gz), O._p(gzp), O._p(y), None, O._p(zero), O._p(one), O._p(one), O._p(zero), None, None, n)
    fused = lambda: O.call('tg_norm_act_bwd', *common, O._p(gy), 0, None, None, None, None, O._p(ws), n, h, w, c, flags, 0.2, 0,
                           O._dt(y), O._stream())
    sums = lambda: O.call('tg_norm_act_bwd_sums', *common, 0, None, None, None, None, O._p(ws), O._p(local), n, h, w, c, flags,
                          0.2, 0, O._dt(y), O._stream())
    apply_ = lambda: O.call('tg_norm_act_bwd_apply', *common, 0, O._p(gy), O._p(local.view(1, n, 2, c)), 1, n, h, w, c, flags,
                            0.2, O._dt(y), O._stream())
    return fused, sums, apply_, gy

  fused, sums, apply_, gy = routes(2, 2, False, _lib.NF_NOSTATS)
  for entry in (sums, apply_):
    with pytest.raises(_lib.TgError, match='NF_NOSTATS'):
      entry()
  assert fused() == 0
  torch.cuda.synchronize()
  assert torch.isfinite(gy).all()
  fused, sums, apply_, _ = routes(3, 2, True, 0)
  for entry in (fused, sums, apply_):
    with pytest.raises(_lib.TgError, match='even h, w'):
      entry()


# ------------------------------------------------------------------------------------------------ 2. the split backward
def _near_zero(r64, r32):
  """tests/test_gpu_ops.py _near_zero: where the float64 pre-activation is inside its own bound 2^-24 |u| + 16 E32(u)."""
  u, u32 = r64['u'].numpy(), r32['u'].numpy()
  small = np.abs(u) < 2.0 ** -6
  e_u = E.e32(u32[small], u[small]) if small.sum() >= 256 else E.e32(u32, u)
  return np.abs(u) < E.e32_bound(u, e_u, torch.float32)


def _seeded(make, refs, lrelu, seed):
  """The first of seeds seed, seed + 1, ... whose float64 reference ALONE has fewer than 1e-5 of its pre-activations inside
  their bound (a condition on the inputs, decided before any kernel runs)."""
  for s in range(seed, seed + 8):
    inp = make(s)
    r64, r32 = refs(inp, torch.float64), refs(inp, torch.float32)
    near = _near_zero(r64, r32) if lrelu else None
    if near is None or near.mean() < 1e-5:
      return inp, r64, r32, near
  raise AssertionError('no seed in [%d, %d) meets the LeakyReLU condition' % (seed, seed + 8))


SPLIT_CASES = [
    # id, R, n, per-replica (b*h, w), c, lrelu, pixel norm, pooled-gradient input, split (None: one domain), mode
    #   mode 'ret': parameter gradients returned; 'sink': accumulated into buffers that already hold values; 'rows': one
    #   parameter row per group ([n, c], written)
    ('r3_two_domains_lrelu_pn_tail_chunk', 3, 2, 10, 26, 32, True, True, False, 1, 'ret'),
    ('r2_scalar_c5_plain', 2, 3, 10, 26, 5, False, False, False, None, 'ret'),
    ('r2_pooled_gradient_pn_sink', 2, 2, 12, 8, 8, True, True, True, None, 'sink'),
    ('r2_rows_scalar_c24_lrelu', 2, 3, 5, 13, 24, True, False, False, None, 'rows'),
    ('r2_rows_pn_pooled_gradient', 2, 2, 6, 4, 16, True, True, True, None, 'rows'),
    ('r8_16_chunks_lrelu_sink_split0', 8, 1, 64, 16, 8, True, False, False, 0, 'sink'),
]


@pytest.mark.parametrize('dname', sorted(EW_DTYPES))
@pytest.mark.parametrize('case', SPLIT_CASES, ids=[c[0] for c in SPLIT_CASES])
def test_split_backward_elementwise(case, dname):
  """R emulated replicas: moments -> merge -> tg_norm_act_fwd per chunk, tg_norm_act_bwd_sums per chunk (stacked = the
  all-gather), tg_norm_act_bwd_apply per chunk.  Every element of z and gy of the chunks put together, and the replicas'
  parameter gradients added up, against norm_act_reference (float64) on the concatenated view [n, R*b*h, w, c] -- the bounds of
  the fused path (u |ref| + 16 E32; the other LeakyReLU slope only where the float64 pre-activation is inside its own bound,
  for at most 1e-5 of the elements)."""
  import twingan_amd.ops as O
  from twingan_amd import _lib
  name, R, n, bh, w, c, lrelu, pn, pool, split, mode = case
  dtype = EW_DTYPES[dname]
  two, rows = split is not None, mode == 'rows'
  H = R * bh

  def make(seed):
    rng = np.random.RandomState(seed)
    y = _round_to(rng.randn(n, H, w, c) * 1.5 + 0.7 + 0.5 * rng.randn(1, 1, 1, c), dtype)
    gz = _round_to(rng.randn(n, H, w, c), dtype)
    gzp = _round_to(rng.randn(n, H // 2, w // 2, c), dtype) if pool else None
    shp = (n, c) if rows else (c,)
    par = [torch.from_numpy((o + s * rng.randn(*shp)).astype(np.float32)).double() for o, s in ((1.0, 0.2), (0.0, 0.1)) * 2]
    return y, gz, gzp, par

  def refs(inp, dt, flip=None):
    y, gz, gzp, par = inp
    return E.norm_act_reference(y.to(dt), par[0], par[1], gz, par[2] if two else None, par[3] if two else None, split=split,
                                lrelu=lrelu, pixel_norm=pn, pool=pool, gzp=gzp, eps=BN_EPS, flip=flip)
  inp, r64, r32, near = _seeded(make, refs, lrelu, 40 + len(name))
  y, gz, gzp, par = inp
  npar = 4 if two else 2
  pd = [p.float().to(dev()).contiguous() for p in par[:npar]] + [None] * (4 - npar)
  flags = (_lib.NF_LRELU if lrelu else 0) | (_lib.NF_PIXNORM if pn else 0)
  sp = split if two else n
  lib = _lib.load()
  chunk = lambda t, r, d: None if t is None else t[:, r * (bh // d):(r + 1) * (bh // d)].contiguous().to(dev()).to(dtype)
  ys = [chunk(y, r, 1) for r in range(R)]
  gzs = [chunk(gz, r, 1) for r in range(R)]
  gzps = [chunk(gzp, r, 2) for r in range(R)]
  mean, rstd = _merge(O, torch.stack([_moments(O, t) for t in ys]).contiguous(), bh * w, BN_EPS)
  zs, ss = [], []
  for r in range(R):
    z = torch.empty_like(ys[r])
    s = _f32(n * bh * w) if pn else None
    O.call('tg_norm_act_fwd', O._p(ys[r]), O._p(mean), O._p(rstd), O._p(pd[0]), O._p(pd[1]), O._p(pd[2]), O._p(pd[3]), sp,
           1 if rows else 0, O._p(z), O._p(s), n, bh, w, c, flags, 0.2, 1e-6, O._dt(z), O._stream())
    zs.append(z)
    ss.append(s)
  # parameter gradients: 'ret' / 'rows' written per replica and added here (what the gradient all-reduce does); 'sink': every
  # replica's call accumulates into the same pre-filled buffers
  pre = [torch.from_numpy(np.random.RandomState(5 + i).randn(c).astype(np.float32)).to(dev()) for i in range(npar)]
  sinks = [t.clone() for t in pre]
  per_rep, locals_ = [], []
  for r in range(R):
    if mode == 'sink':
      outs = sinks
    else:
      outs = [_f32((n, c) if rows else c) for _ in range(npar)]
    outs = list(outs) + [None] * (4 - npar)
    ws = _f32(n * lib.tg_norm_chunks(n, bh, w) * 2 * c)
    local = _f32((n, 2, c))
    O.call('tg_norm_act_bwd_sums', O._p(gzs[r]), O._p(gzps[r]), O._p(ys[r]), O._p(ss[r]), O._p(mean), O._p(rstd), O._p(pd[0]),
           O._p(pd[1]), O._p(pd[2]), O._p(pd[3]), sp, 1 if rows else 0, O._p(outs[0]), O._p(outs[1]), O._p(outs[2]), O._p(outs[3]),
           O._p(ws), O._p(local), n, bh, w, c, flags, 0.2, 1 if mode == 'sink' else 0, O._dt(ys[r]), O._stream())
    per_rep.append(outs)
    locals_.append(local)
  gathered = torch.stack(locals_).contiguous()
  gys = []
  for r in range(R):
    gy = torch.empty_like(ys[r])
    O.call('tg_norm_act_bwd_apply', O._p(gzs[r]), O._p(gzps[r]), O._p(ys[r]), O._p(ss[r]), O._p(mean), O._p(rstd), O._p(pd[0]),
           O._p(pd[1]), O._p(pd[2]), O._p(pd[3]), sp, 1 if rows else 0, O._p(gy), O._p(gathered), R, n, bh, w, c, flags, 0.2,
           O._dt(gy), O._stream())
    gys.append(gy)
  torch.cuda.synchronize()
  what = 'syncnorm[%s,%s]' % (name, dname)
  ref = r64['z'].numpy()
  r = E.assert_elementwise(host(torch.cat(zs, dim=1)), ref, E.e32_bound(ref, E.e32(r32['z'].numpy(), ref), dtype), what + ' z')
  print('[elementwise] %s z worst ratio %.3f' % (what, r))
  ref = r64['gy'].numpy()
  alt = refs(inp, torch.float64, torch.from_numpy(near))['gy'].numpy() if near is not None and near.any() else None
  r = E.assert_elementwise(host(torch.cat(gys, dim=1)), ref, E.e32_bound(ref, E.e32(r32['gy'].numpy(), ref), dtype), what + ' gy',
                           alt_ref=alt, alt_where=near)
  print('[elementwise] %s gy worst ratio %.3f' % (what, r))
  for i, nm in enumerate(('gamma', 'beta', 'gamma2', 'beta2')[:npar]):
    ref = r64['grads'][i].numpy()
    bound = E.e32_bound(ref, E.e32(r32['grads'][i].numpy(), ref), torch.float32)
    if mode == 'sink':      # R additions into what the buffer held: their roundings named here
      got = host(sinks[i]) - host(pre[i])
      bound = bound + R * 2.0 ** -24 * (np.abs(host(pre[i])) + np.abs(ref))
    else:                   # the replicas' gradients added in float64 here (the all-reduce's fp32 additions are not under test)
      got = sum(host(per_rep[r][i]) for r in range(R))
      bound = bound + R * 2.0 ** -24 * np.abs(ref)
    r = E.assert_elementwise(got, ref, bound, '%s %s gradient (%s)' % (what, nm, mode))
    print('[elementwise] %s %s gradient worst ratio %.3f' % (what, nm, r))


def test_autograd_route_with_one_replica_matches_the_fused_route():
  """ops.norm_act(..., replicas=ReplicaGather(1)) -- the split route end to end through autograd, the gather a copy -- against
  the fused route on the same tensors: same statistics up to their roundings, so z / gy / parameter gradients agree to the
  fused path's own bound against float64 taken twice (two kernels of one formula)."""
  import twingan_amd.ops as O
  from twingan_amd.dp import ReplicaGather
  rng = np.random.RandomState(11)
  n, h, w, c = 2, 12, 10, 16
  y0 = torch.from_numpy(rng.randn(n, h, w, c).astype(np.float32))
  gz = torch.from_numpy(rng.randn(n, h, w, c).astype(np.float32)).to(dev())
  gzp = torch.from_numpy(rng.randn(n, h // 2, w // 2, c).astype(np.float32)).to(dev())
  rep = ReplicaGather(1)
  got = {}
  for key, kw in (('fused', {}), ('split', dict(replicas=rep))):
    y = y0.clone().to(dev()).requires_grad_(True)      # a leaf of its own for each route
    ga = torch.full((c,), 1.1, device=dev()).requires_grad_(True)
    be = torch.full((c,), 0.1, device=dev()).requires_grad_(True)
    z, zp = O.norm_act(y, ga, be, lrelu=True, pixel_norm=True, in_eps=BN_EPS, pool=True, **kw)
    torch.autograd.backward([z, zp], [gz, gzp])
    torch.cuda.synchronize()
    got[key] = [host(t) for t in (z, zp, y.grad, ga.grad, be.grad)]
  assert rep.stats() == dict(gather_bytes=0, collectives=0)      # one replica: no collective
  for a, b, nm in zip(got['fused'], got['split'], ('z', 'zp', 'gy', 'ggamma', 'gbeta')):
    assert np.abs(a - b).max() <= 2e-5 * max(1.0, np.abs(a).max()), (nm, np.abs(a - b).max())


# ------------------------------------------------------------------------------------------------ 3. two clones over gloo
def _clone_batches(rank):
  g = torch.Generator().manual_seed(900 + rank)
  return torch.rand(2, 16, 16, 3, generator=g), torch.rand(2, 16, 16, 3, generator=g)


def _cotangents(rank):
  g = torch.Generator().manual_seed(950 + rank)
  return {k: torch.randn(2, 16, 16, 3, generator=g) for k in ('s_prime', 's_cycle', 't_prime', 't_cycle')}


def _generator_side(tr, cfg, s, t, cot):
  """One training-mode pass of the encoder and the four generator passes, a fixed cotangent on the four translations (a loss
  of per-sample terms only) -> (outputs, generator-group gradients, state variables), on the host."""
  from twingan_amd import pggan
  from twingan_amd import twingan as T
  d = tr.device
  tr.store.zero_grad('g')
  tr._set_requires_grad(g=True, d=False)
  pggan.prepare_run(tr.P, cfg)
  o = T.forward_generators(tr.P, s.to(d).contiguous(), t.to(d).contiguous(), cfg)
  loss = sum((o[k].float() * cot[k].to(d)).sum() for k in sorted(cot))
  loss.backward()
  pggan.end_run(tr.P)
  grads = {k: v.cpu().numpy() for k, v in tr.store.grad_dict().items() if k in set(tr.store.names('g'))}
  outs = {k: o[k].detach().float().cpu().numpy() for k in cot}
  state = {k: v.detach().cpu().numpy().copy() for k, v in tr.store.state.items()}
  return outs, grads, state


def _gen_cfg(norm, **kw):
  from twingan_amd import Config
  return Config(hw=16, max_ch=16, precision='fp32', generator_norm_type=norm, **kw)


def _trainer_cfg(flag):
  from twingan_amd import Config
  return Config(hw=16, max_ch=16, precision='fp32', generator_norm_type='batch_renorm', overlap_cut_hw=8, cross_replica_norm=flag)


def _sync_worker(rank, world, port, q, backend):
  import datetime
  import torch.distributed as dist
  os.environ['MASTER_ADDR'] = '127.0.0.1'
  os.environ['MASTER_PORT'] = str(port)
  device = 'cuda:%d' % (rank if backend == 'nccl' else 0)      # gloo: both ranks share the box's single GPU
  torch.cuda.set_device(device)
  dist.init_process_group(backend, rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
  try:
    from twingan_amd.twingan import Trainer
    out = {}
    if backend == 'gloo':
      for norm in ('batch_norm', 'batch_renorm'):
        cfg = _gen_cfg(norm, cross_replica_norm=True)
        tr = Trainer(cfg, device=device, seed=8, world_size=world)
        assert tr.replicas is not None and tr.P.replicas is tr.replicas and tr.replicas.rank == rank
        s, t = _clone_batches(rank)
        out['gen_' + norm] = _generator_side(tr, cfg, s, t, _cotangents(rank)) + (tr.replicas.stats(),)
        tr.close()
    for flag in ((True, False) if backend == 'gloo' else (True,)):
      tr = Trainer(_trainer_cfg(flag), device=device, seed=7, world_size=world)
      assert tr.split, 'more than one clone: the segmented backward, its all-reduces between the normalisers\' gathers'
      s, t = (x.to(device) for x in _clone_batches(rank))
      for _ in range(4):
        tr.run(s, t)
      torch.cuda.synchronize()
      out['trainer_%s' % ('on' if flag else 'off')] = (
          tr.store.flat['g'].cpu().numpy(), tr.store.flat['d'].cpu().numpy(),
          {k: v.detach().cpu().numpy().copy() for k, v in tr.store.state.items()},
          tr.replicas.stats() if tr.replicas is not None else None)
      tr.close()
    q.put((rank, out))
    dist.barrier()
  finally:
    dist.destroy_process_group()


def _run_two_clones(backend):
  """Two child processes, started once; every wait has a limit and the children never outlive the call."""
  import socket
  import torch.multiprocessing as mp
  sk = socket.socket()
  sk.bind(('127.0.0.1', 0))
  port = sk.getsockname()[1]
  sk.close()
  ctx = mp.get_context('spawn')
  q = ctx.Queue()
  procs = [ctx.Process(target=_sync_worker, args=(r, 2, port, q, backend)) for r in range(2)]
  try:
    for p in procs:
      p.start()
    got = {}
    for _ in range(2):
      r, out = q.get(timeout=300)
      got[r] = out
    for p in procs:
      p.join(timeout=120)
      assert p.exitcode == 0, 'a clone exited with %r' % (p.exitcode,)
    return got
  finally:
    for p in procs:
      if p.is_alive():
        p.terminate()
        p.join(timeout=30)


@pytest.fixture(scope='module')
def two_clones():
  return _run_two_clones('gloo')


@pytest.mark.parametrize('norm', ['batch_norm', 'batch_renorm'])
def test_data_parallel_two_clones_cross_replica_generator_matches_one_clone(two_clones, norm):
  """Each clone's training-mode translations equal its rows of ONE clone that runs the concatenated batch (2 + 2 images per
  pass) with the flag off; the clones' generator gradients add up to that clone's; all three hold the same state."""
  from twingan_amd.twingan import Trainer
  cfg = _gen_cfg(norm)
  tr = Trainer(cfg, device='cuda:0', seed=8)
  b0, b1 = _clone_batches(0), _clone_batches(1)
  c0, c1 = _cotangents(0), _cotangents(1)
  outs, grads, state = _generator_side(tr, cfg, torch.cat([b0[0], b1[0]]), torch.cat([b0[1], b1[1]]),
                                       {k: torch.cat([c0[k], c1[k]]) for k in c0})
  tr.close()
  for rank in (0, 1):
    o_r, _, st_r, stats = two_clones[rank]['gen_' + norm]
    assert stats['collectives'] > 0 and stats['gather_bytes'] > 0
    for k in outs:
      want = outs[k][2 * rank:2 * rank + 2]
      err = np.abs(o_r[k] - want).max()
      print('[two clones, %s] rank %d %s: max |difference| %.3e' % (norm, rank, k, err))
      assert err <= 1e-4 * max(1.0, np.abs(want).max()), (rank, k, err)
    assert set(st_r) == set(state)
    for k, v in state.items():
      assert np.abs(st_r[k] - v).max() <= 1e-5 * max(1.0, np.abs(v).max()), (rank, k)
  st0, st1 = two_clones[0]['gen_' + norm][2], two_clones[1]['gen_' + norm][2]
  assert all(st0[k].tobytes() == st1[k].tobytes() for k in st0), 'the clones\' state variables differ in their bits'
  g0, g1 = two_clones[0]['gen_' + norm][1], two_clones[1]['gen_' + norm][1]
  num = den = 0.0
  worst = (0.0, None)
  top = max(np.linalg.norm(v.astype(np.float64)) for v in grads.values())
  for k, ref in grads.items():
    a, b = g0[k].astype(np.float64) + g1[k].astype(np.float64), ref.astype(np.float64)
    num += np.sum((a - b) ** 2)
    den += np.sum(b ** 2)
    e = np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-12)
    if e > worst[0] and np.linalg.norm(b) >= 1e-3 * top:
      worst = (e, k)
  tot = np.sqrt(num / (den + 1e-30))
  print('[two clones, %s] summed generator gradients: aggregate rel-L2 %.3e, worst variable %s %.3e' % (norm, tot, worst[1], worst[0]))
  assert tot < FP32_GRAD_TOL and worst[0] < FP32_VAR_GRAD_TOL, (tot, worst)


def _check_trainer_clones(got, key):
  for i in (0, 1):
    a, b = got[0][key][i], got[1][key][i]
    assert np.abs(a - b).max() <= 1e-6 * max(1.0, np.abs(a).max()), 'clones diverged'
  st0, st1 = got[0][key][2], got[1][key][2]
  return st0, st1


def test_data_parallel_two_clones_cross_replica_trainer_state(two_clones):
  """Four runs of the Trainer (segmented backward, one all-reduce per segment between the normalisers' gathers): with the flag
  both clones end with equal parameters and BIT-identical state variables; without it the same two clones' moving means
  differ -- the flag is what aligns them."""
  st0, st1 = _check_trainer_clones(two_clones, 'trainer_on')
  assert set(st0) == set(st1) and any('moving_mean' in k for k in st0)
  diff = [k for k in st0 if st0[k].tobytes() != st1[k].tobytes()]
  assert not diff, diff[:5]
  stats = two_clones[0]['trainer_on'][3]
  assert stats['collectives'] > 0 and stats == two_clones[1]['trainer_on'][3]
  print('[two clones] trainer, 4 runs: %d all-gathers, %d bytes received per clone' % (stats['collectives'], stats['gather_bytes']))
  of0, of1 = _check_trainer_clones(two_clones, 'trainer_off')
  assert two_clones[0]['trainer_off'][3] is None
  moved = [k for k in of0 if 'moving_mean' in k and np.abs(of0[k] - of1[k]).max() > 0]
  assert moved, 'without the flag the clones\' moving means were expected to differ'


def test_data_parallel_two_clones_cross_replica_trainer_nccl():
  """The Trainer test over RCCL on two GPUs, where two are visible."""
  if torch.cuda.device_count() < 2:
    pytest.skip('needs two GPUs')
  got = _run_two_clones('nccl')
  st0, st1 = _check_trainer_clones(got, 'trainer_on')
  assert not [k for k in st0 if st0[k].tobytes() != st1[k].tobytes()]
