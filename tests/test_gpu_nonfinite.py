"""Inf and NaN propagate and stay contained, kernel by kernel (tests/nonfinite.py: the contract, the helpers, the case tables).

Every case runs through the Python ops or the C ABI as the element-wise tests do: the unplanted inputs twice (equal bits: the
launch is bit-reproducible, and containment is then bit-equality with that launch), the planted inputs once.  The oracle
decides which output elements must be non-finite.  Outputs a case table lists under `atomic` meet in atomics and take their
family's bound instead; so do the elements the oracle changes without making them non-finite.  Runs over the emulated kernels
too (TG_EMU=1)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nonfinite as NF      # noqa: E402

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
DT = {'f32': torch.float32, 'bf16': torch.bfloat16, 'f16': torch.float16}
BOUND_ROUTE = set()      # (case id, dtype, output) of the launches that were held to a bound, printed with -s


@pytest.fixture(scope='module')
def ops():
  from twingan_amd import ops as _ops
  return _ops


def dev(a, dname='f32', grad=False):
  t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV).to(DT[dname]).contiguous()
  return t.requires_grad_(True) if grad else t


def host(t):
  return t.detach().float().cpu().numpy().astype(np.float64)


# ------------------------------------------------------------------------------------------------ launchers, one per family
def _pred_loss(ops, case, inp, dname):
  mode, a, b = case.par['mode'], case.par['a'], case.par['b']
  loss, gx = [], []
  for row in inp['x']:
    x = dev(row, grad=True)
    out = ops.PredLossFn.apply(x, mode, float(a), float(b), NF.PRED_W)
    (out * NF.PRED_G).backward()
    loss.append(out.detach())
    gx.append(x.grad)
  return dict(loss=torch.cat(loss), gx=torch.stack(gx))


def _pred_losses(ops, case, inp, dname):
  groups, gs = inp['x'].shape
  x = dev(inp['x'].reshape(-1, 1), grad=True)
  out = ops.pred_losses(x, gs, NF.PRED_JOBS, 5)
  live = [t for t in range(5) if NF.PRED_GTS[t] is not None]
  torch.autograd.backward([out[t] for t in live], [torch.full((1,), NF.PRED_GTS[t], device=DEV) for t in live])
  return dict(terms=torch.cat([o.detach() for o in out]), gx=x.grad.reshape(groups, gs))


def _abs_diff(ops, case, inp, dname):
  a, b = dev(inp['a'], dname, True), dev(inp['b'], dname, True)
  loss = ops.abs_diff_mean(a, b, NF.ABS_W)
  (loss * NF.ABS_G).backward()
  return dict(loss=loss.detach(), ga=a.grad, gb=b.grad)


def _gradient_penalty(ops, case, inp, dname):
  g = dev(inp['g'], dname, True)
  loss = ops.gradient_penalty(g, NF.GP_LAM)
  (loss * NF.GP_G).backward()
  return dict(loss=loss.detach(), gg=g.grad)


def _variance(ops, case, inp, dname):
  var, interp = [], []
  for r in range(inp['x'].shape[0]):
    x = dev(inp['x'][r], dname)
    var.append(ops.batch_variance(x))
    interp.append(ops.dragan_interpolates(x, dev(inp['noise'][r], dname), dev(inp['alpha'][r])))
  return dict(var=torch.cat(var), interp=torch.stack(interp))


def _sums(ops, case, inp, dname):
  mean, gmean, add_n = [], [], []
  for r in range(3):
    x = dev(inp['x'][r], dname, True)
    m = ops.mean(x, -1.0)
    m.backward(dev(inp['g'][r:r + 1]))      # the gradient of a mean is tg_fill_scaled by the incoming scalar
    mean.append(m.detach())
    gmean.append(x.grad)
    add_n.append(ops.sum_scalars([dev(inp['t'][r, i:i + 1]) for i in range(inp['t'].shape[1])]))
  return dict(mean=torch.cat(mean), gmean=torch.stack(gmean), add_n=torch.cat(add_n))


def _axpby(ops, case, inp, dname):
  a, b = case.par.get('ab', NF.AXPBY)
  x, y = dev(inp['x'], dname), dev(inp['y'], dname)
  out = torch.empty_like(x)
  ops.call('tg_axpby', x.data_ptr(), y.data_ptr(), out.data_ptr(), x.numel(), a, b, ops._dt(x), ops._stream())
  return dict(out=out)


def _lerp(ops, case, inp, dname):
  return dict(out=ops.lerp(dev(inp['x'], dname), dev(inp['y'], dname), 0.25))


def _sample_lerp(ops, case, inp, dname):
  return dict(out=ops.sample_lerp(dev(inp['x'], dname), dev(inp['y'], dname), dev(inp['alpha'])))


def _gdrop(ops, case, inp, dname):
  return dict(out=ops.gdrop(dev(inp['x'], dname), NF.GDROP_S, noise=dev(inp['noise']), c_logical=inp['x'].shape[3]))


def _cast(ops, case, inp, dname):
  if case.par.get('to_f32'):
    return dict(out=ops.cast_raw(dev(inp['x'], dname), torch.float32))
  return dict(out=ops.cast_raw(dev(2.0 * inp['x']), DT[dname]))


def _lrelu_bwd(ops, case, inp, dname):
  return dict(out=ops.lrelu_bwd_raw(dev(inp['g'], dname), dev(inp['z'], dname), 0.2))


def _lrelu_pool_bwd(ops, case, inp, dname):
  bias = torch.zeros(inp['z'].shape[3], device=DEV)
  g, gb = ops.lrelu_pool_bwd(dev(inp['gz'], dname), dev(inp['gzp'], dname), dev(inp['z'], dname), 0.2, bias, True)
  return dict(g=g, gb=gb)


def _pool(ops, case, inp, dname):
  x = dev(inp['x'], dname, True)
  y = ops.Pool2Fn.apply(x, case.par.get('scale', 0.25))
  if case.par.get('fwd_only'):
    return dict(y=y.detach())
  y.backward(dev(inp['gy'], dname))
  return dict(y=y.detach(), gx=x.grad)


def _upsample_concat(ops, case, inp, dname):
  x0, x1 = dev(inp['x0'], dname, True), dev(inp['x1'], dname, True)
  out = ops.upsample2x_concat(x0, x1)
  out.backward(dev(inp['go'], dname))
  return dict(out=out.detach(), g0=x0.grad, g1=x1.grad)


def _norm_act(ops, case, inp, dname):
  from twingan_amd import _lib
  p = case.par
  n, h, w, c = inp['y'].shape
  assert _lib.load().tg_norm_chunks(n, h, w) == NF.norm_chunking(n, h * w)[0][0], 'norm_chunks moved: the plants no longer sit at a block edge'
  y = dev(inp['y'], dname, True)
  names = ('gamma', 'beta') + (('gamma2', 'beta2') if p['split'] is not None else ())
  par = [dev(inp[k], grad=True) for k in names]
  kw = dict(lrelu=True, pixel_norm=p['pn'], pool=p['pool'])
  if p['split'] is not None:
    kw.update(gamma2=par[2], beta2=par[3], split=p['split'])
  if p.get('rows'):      # [n, c] parameter rows take their statistics from the caller
    kw.update(stats=ops.instance_stats(y.detach(), 1e-6))
  if p.get('replicas'):
    from twingan_amd.dp import ReplicaGather
    kw.update(replicas=ReplicaGather(1))
  out = (ops.layer_norm_act if p['layer'] else ops.norm_act)(y, par[0], par[1], **kw)
  z, zp = out if p['pool'] else (out, None)
  if p['pool']:
    torch.autograd.backward([z, zp], [dev(inp['gz'], dname), dev(inp['gzp'], dname)])
  else:
    z.backward(dev(inp['gz'], dname))
  res = dict(z=z.detach(), gy=y.grad)
  if p['pool']:
    res['zp'] = zp.detach()
  res.update({'g' + k: t.grad for k, t in zip(names, par)})
  return res


def _conv(ops, case, inp, dname):
  """Forward with bias and LeakyReLU, masked forward (gy: the mask source), backward-data, masked backward-data (x: the mask
  source) -- and each must have run the kernel family the case is for (`direct`: the dispatch itself sends channel counts the
  MFMA kernels refuse to the one-thread-per-output kernels)."""
  from twingan_amd import _lib
  from twingan_amd._lib import TG_EPI_BIAS, TG_EPI_LRELU
  spec = ops.ConvSpec(case.par['k'], case.par['pad'], 0, 0.2)
  x, gy, w, b = dev(inp['x'], dname), dev(inp['gy'], dname), dev(inp['w']), dev(inp['b'])
  direct = case.par['symbol'] == 'direct'
  out, ran = {}, {}
  for name, fn in (('fwd', lambda: ops.conv_fwd_raw(x, w, b, spec, TG_EPI_BIAS | TG_EPI_LRELU)),
                   ('fwd_masked', lambda: ops.conv_fwd_masked_raw(x, w, gy, spec)),
                   ('bwd', lambda: ops.conv_bwd_data_raw(gy, w, tuple(x.shape), spec)),
                   ('bwd_masked', lambda: ops.conv_bwd_data_masked_raw(gy, w, x, spec))):
    out[name] = fn()
    ran[name] = _lib.load().tg_last_kernel().decode()
  want = case.par['symbol']
  assert all(want in s and (direct or ('f16' in s) == (dname == 'f16')) for s in ran.values()), (case.id, dname, want, ran)
  assert not case.par.get('sets') or all(s.endswith(',sets>') for s in ran.values()), ran      # ONE launch picks the set per image
  if case.par.get('extras'):
    n, h, wd, c = out['fwd'].shape
    ys, st = ops.conv_fwd_stats_raw(x, w, spec)
    assert st is not None, 'the statistics epilogue did not run'
    out['stats_y'], out['part_sum'] = ys, st.part.view(n, st.chunks, 2, c).sum(dim=1)
    out['pool_z'], out['zp'] = ops.conv_fwd_pool_raw(x, w, b, spec, TG_EPI_BIAS | TG_EPI_LRELU)
    assert 'pool' in _lib.load().tg_last_kernel().decode()
    assert ops.conv_fwd_pool_signs_supported(x, w, spec, TG_EPI_BIAS | TG_EPI_LRELU)
    sg, out['signs_zp'] = ops.conv_fwd_pool_signs_raw(x, w, b, spec, TG_EPI_BIAS | TG_EPI_LRELU)
    bad = (~torch.isfinite(out['pool_z'].float())).view(n, h, wd, c // 8, 8).any(dim=-1)      # a byte over a non-finite z is not pinned
    out['signs'] = torch.where(bad, torch.full((), float('nan'), device=sg.device), sg.float())
  return out


def _softmax_rows(ops, case, inp, dname):
  return dict(p=ops.softmax_rows(dev(inp['s'], dname)), ds=ops.SoftmaxRowsBwdFn.apply(dev(inp['p'], dname), dev(inp['dp'], dname)))


def _bgemm(ops, case, inp, dname):
  a, b, at, bt = (dev(inp[k], dname) for k in ('a', 'b', 'at', 'bt'))
  bsz, m, k = a.shape
  n, pad = b.shape[2], 3

  def padded(t):      # rows `pad` elements apart, NaN in between
    buf = torch.full((t.shape[0], t.shape[1], t.shape[2] + pad), float('nan'), dtype=t.dtype, device=DEV)
    buf[..., :t.shape[2]] = t
    return buf
  ap, bp, cp = padded(a), padded(b), padded(dev(inp['c0'], dname))
  ops.call('tg_batched_gemm', ap.data_ptr(), bp.data_ptr(), cp.data_ptr(), bsz, m, n, k, 0, 0, k + pad, n + pad, n + pad,
           m * (k + pad), k * (n + pad), m * (n + pad), 0.5, 1, ops._dt(a), 0, ops._stream())
  assert bool(torch.isnan(cp[..., n:].float()).all()), 'the padding of C was written'
  return dict(c=ops.bgemm(a, b, False, False, 0.5), ct=ops.bgemm(at, bt, True, True, 0.5), cnt=ops.bgemm(a, bt, False, True, 0.5),
              ctn=ops.bgemm(at, b, True, False, 0.5), cabi=cp[..., :n].contiguous())


def _last_kernel():
  from twingan_amd import _lib
  return _lib.load().tg_last_kernel().decode()


def _wgrad(ops, case, inp, dname):
  from twingan_amd import _lib
  if case.par.get('det') and not ops.deterministic():      # the ordered slab reduction: bit-reproducible
    was = _lib.load().tg_set_deterministic(1)
    try:
      return _wgrad(ops, case, inp, dname)
    finally:
      _lib.load().tg_set_deterministic(was)
  spec = ops.ConvSpec(3, 'SAME')
  out = dev(inp['sink'])
  res = {}
  if 'xb' in inp:      # the paired launch, added into the sink
    assert ops.conv_bwd_weight2_raw(dev(inp['xa'], dname), dev(inp['ga'], dname), dev(inp['xb'], dname), dev(inp['gb'], dname), spec, out)
  else:                # one launch, the bias gradient riding along
    res['gbias'] = torch.zeros(inp['ga'].shape[3], dtype=torch.float32, device=DEV)
    ops.conv_bwd_weight_raw(dev(inp['xa'], dname), dev(inp['ga'], dname), spec, out=out, gbias=res['gbias'])
  sym = _last_kernel()
  assert sym.startswith(case.par['symbol']), (case.id, sym)
  res['gw'] = out
  return res


def _pointwise(ops, case, inp, dname):
  from twingan_amd import _lib
  if case.par.get('det') and not ops.deterministic():
    was = _lib.load().tg_set_deterministic(1)
    try:
      return _pointwise(ops, case, inp, dname)
    finally:
      _lib.load().tg_set_deterministic(was)
  x, w, b = dev(inp['x'], dname, True), dev(inp['w'], grad=True), dev(inp['b'], grad=True)
  y = ops.pointwise_conv(x, w.view(1, 1, *w.shape), b)
  y.backward(dev(inp['gy'], dname))
  out = dict(y=y.detach(), gx=x.grad, gw=w.grad, gb=b.grad)
  if w.shape[0] <= 4:
    out['ym'] = ops._pw_fwd_masked_raw(x.detach(), w.detach(), False, dev(inp['gy'], dname), 0.2)
  return out


def _upcat_conv(ops, case, inp, dname):
  x0, x1, w = dev(inp['x0'], dname, True), dev(inp['x1'], dname, True), dev(inp['w'], grad=True)
  assert ops.upcat_conv_supported(x0, x1, w)
  perm = case.par['perm']
  x1s = x1 if not perm else torch.cat([x1[1:2], x1[0:1], x1[2:3]]).detach().contiguous().requires_grad_(True)
  y = ops.upcat_conv(x0, x1s, w, 1, (1, 0, 2)) if perm else ops.upcat_conv(x0, x1, w)
  assert 'up' in _last_kernel(), _last_kernel()
  y.backward(dev(inp['gy'], dname))
  g1 = x1s.grad
  with torch.no_grad():
    ys, st = ops.upcat_conv_stats(x0, x1s, w, 1, (1, 0, 2)) if perm else ops.upcat_conv_stats(x0, x1, w)
  assert st is not None, 'the statistics epilogue did not run'
  return dict(y=y.detach(), g0=x0.grad, g1=g1 if not perm else torch.cat([g1[1:2], g1[0:1], g1[2:3]]), gw=w.grad, stats_y=ys,
              part_sum=st.part.view(3, st.chunks, 2, 16).sum(dim=1))


def _mbstd(ops, case, inp, dname):
  from twingan_amd.params import mbstd_cpad
  n, groups, c = NF.MB
  cpad = mbstd_cpad(c)
  x = dev(inp['x'], dname, True)
  out = ops.minibatch_state_concat(x, cpad, groups)
  go = torch.zeros((n, 4, 4, cpad), dtype=DT[dname], device=DEV)
  go[..., :c + 1] = dev(inp['go'], dname)
  go.requires_grad_(True)
  gx, = torch.autograd.grad(out, x, grad_outputs=go, create_graph=True)
  ggo, gx2 = torch.autograd.grad(gx, [go, x], grad_outputs=dev(inp['v'], dname))      # the second-order kernel
  return dict(out=out.detach()[..., :c + 1], gx=gx.detach(), ggo=ggo[..., :c + 1], gx2=gx2)


def _tanh(ops, case, inp, dname):
  return dict(y=ops.tanh(dev(inp['x'], dname)))


def _tanh_bwd_mul3(ops, case, inp, dname):
  y, g, v = (dev(inp[k], dname) for k in ('y', 'g', 'v'))
  gx, gy = torch.empty_like(g), torch.empty_like(g)
  ops.call('tg_tanh_bwd', g.data_ptr(), y.data_ptr(), gx.data_ptr(), g.numel(), ops._dt(g), ops._stream())
  ops.call('tg_mul3', y.data_ptr(), g.data_ptr(), v.data_ptr(), gy.data_ptr(), -2.0, g.numel(), ops._dt(g), ops._stream())
  return dict(gx=gx, gy=gy)


def _dot(ops, case, inp, dname):
  out, ga, gb = [], [], []
  for r in range(3):
    a, b = dev(inp['a'][r], dname, True), dev(inp['b'][r], dname, True)
    o = ops.DotFn.apply(a, b)
    (o * 1.5).backward()
    out.append(o.detach()), ga.append(a.grad), gb.append(b.grad)
  return dict(out=torch.cat(out), ga=torch.stack(ga), gb=torch.stack(gb))


def _fully_connected(ops, case, inp, dname):
  x, w, b = dev(inp['x'], dname, True), dev(inp['w'], grad=True), dev(inp['b'], grad=True)
  y = ops.fully_connected(x, w, b)
  y.backward(dev(inp['g']))
  return dict(y=y.detach(), gx=x.grad, gw=w.grad, gb=b.grad)


def _cosine_distance(ops, case, inp, dname):
  e, p = dev(inp['e']), dev(inp['p'], grad=True)
  (ops.cosine_distance(e, p, 0.7) * 1.5).backward()
  rows = [ops.cosine_distance(e[b:b + 1].contiguous(), p.detach()[b:b + 1].contiguous(), 0.7) for b in range(e.shape[0])]
  return dict(rows=torch.cat(rows), gp=p.grad)


def _channel_sum(ops, case, inp, dname):
  from twingan_amd import _lib
  lib, g, out = _lib.load(), dev(inp['g'], dname), {}
  for det, name in ((0, 'atomic'), (1, 'ordered')):
    was = lib.tg_set_deterministic(det)
    try:
      out[name] = ops.channel_sum_raw(g)
    finally:
      lib.tg_set_deterministic(was)
  return out


def _cat_rows(ops, case, inp, dname):
  return dict(out=ops.cat_rows([dev(inp['a'], dname), dev(inp['b'], dname)]))


def _lrelu_bwd_bias(ops, case, inp, dname):
  g, z = dev(inp['g'], dname), dev(inp['z'], dname)
  out, gb = torch.empty_like(z), torch.zeros(z.shape[3], dtype=torch.float32, device=DEV)
  ops.call('tg_lrelu_bwd_bias', g.data_ptr(), z.data_ptr(), out.data_ptr(), gb.data_ptr(), z.numel() // z.shape[3], z.shape[3], 0.2, 0,
           ops._dt(z), ops._stream())
  return dict(out=out, gb=gb)


def _spectral_norm(ops, case, inp, dname):
  ws = [dev(inp['w'][i]).view(3, 3, 8, 16).requires_grad_(True) for i in range(3)]
  res = [ops.spectral_norm(ws[i], dev(inp['u'][i]).view(1, 16)) for i in range(3)]
  for r in res:
    r[0].backward(torch.ones_like(r[0]))      # G = 1: the oracle's
  return dict(w_bar=torch.stack([r[0].detach().reshape(72, 16) for r in res]), u_new=torch.stack([r[1].reshape(-1) for r in res]),
              gw=torch.stack([w.grad.reshape(72, 16) for w in ws]))


def _small_gemm(ops, case, inp, dname):
  a, b = dev(inp['a'], grad=True), dev(inp['b'], grad=True)
  c = ops.GemmFn.apply(a, b, False, False)
  c.backward(dev(inp['g']))
  return dict(c=c.detach(), ga=a.grad, gb=b.grad, ctt=ops.GemmFn.apply(dev(inp['a'].T.copy()), dev(inp['b'].T.copy()), True, True))


def _scale_dev(ops, case, inp, dname):
  return dict(out=torch.stack([ops.scale_dev(dev(inp['x'][r], dname), dev(inp['s'][r:r + 1])) for r in range(3)]))


def _softmax_bwd_bwd(ops, case, inp, dname):
  p, dp, v = (dev(inp[k], dname) for k in ('p', 'dp', 'v'))
  gp = torch.empty_like(p)
  ops.call('tg_softmax_rows_bwd_bwd', p.data_ptr(), dp.data_ptr(), v.data_ptr(), gp.data_ptr(), p.shape[0], p.shape[1], ops._dt(p), ops._stream())
  return dict(gp=gp)


def _spectral_norm_multi(ops, case, inp, dname):
  k = inp['w'].shape[0]
  items = [(dev(inp['w'][i]).view(1, 1, 24, 16), dev(inp['u'][i]).view(1, 16), torch.empty(24 * 16, device=DEV)) for i in range(k)]
  outs, _ = ops.spectral_norm_multi(items)
  return dict(w_bar=torch.stack([o[0].reshape(24, 16) for o in outs]), u_new=torch.stack([o[1].reshape(-1) for o in outs]))


def _flash_second_order(ops, case, inp, dname):
  q, k, v, go = (dev(inp[n], dname, True) for n in ('q', 'k', 'v', 'go'))
  with ops.second_order():
    assert ops.flash_attention_trainable(q, v) == ops.USE_FLASH_BWD_BWD
    o = ops.flash_attention(q, k, v)
    gq, gk, gv = torch.autograd.grad(o, (q, k, v), go, create_graph=True)
    loss = (gq.float() * dev(inp['aq'])).sum() + (gk.float() * dev(inp['ak'])).sum() + (gv.float() * dev(inp['av'])).sum()
    adj = torch.autograd.grad(loss, (q, k, v, go))
  return dict(zip(('adj_q', 'adj_k', 'adj_v', 'adj_go'), adj))


def _unpool(ops, case, inp, dname):
  from twingan_amd._lib import TG_EPI_BIAS, TG_EPI_LRELU
  spec = ops.ConvSpec(3, 'SAME', 0, 0.2)
  x, w, b, gzp = dev(inp['x'], dname), dev(inp['w']), dev(inp['b']), dev(inp['gzp'], dname)
  sg, _ = ops.conv_fwd_pool_signs_raw(x, w, b, spec, TG_EPI_BIAS | TG_EPI_LRELU)
  out = ops.conv_bwd_data_unpool_raw(gzp, sg, w, x, tuple(x.shape), spec, True)
  assert out is not None, 'the unpooling backward-data refused the shape'
  return dict(gx=out[0], kept=out[1])


def _norm_conv_stats(ops, case, inp, dname):
  x, w = dev(inp['x'], dname), dev(inp['w'])
  y, st = ops.conv2d_stats(x, w)
  assert st is not None, 'the conv wrote no statistics'
  y = y.detach().requires_grad_(True)
  z = ops.norm_act(y, dev(inp['gamma']), dev(inp['beta']), lrelu=True, pixel_norm=True, conv_stats=st)
  z.backward(dev(inp['gz'], dname))
  return dict(y=y.detach(), z=z.detach(), gy=y.grad)


def _rows(ops, case, inp, dname):
  head, picked = ops.rows(dev(inp['x'], dname, True), ((0, 2), ((1, 2), (3, 5))))
  return dict(head=head.detach(), picked=picked.detach())


def _flash_attention(ops, case, inp, dname):
  q, k, v = (dev(inp[n], dname, True) for n in 'qkv')
  assert ops.flash_attention_supported(q, v)
  o = ops.flash_attention(q, k, v)
  o.backward(dev(inp['go'], dname))
  o_raw, lse = ops.flash_attention_fwd_raw(q.detach(), k.detach(), v.detach())
  assert torch.equal(o_raw.view(torch.int16), o.detach().view(torch.int16))
  return dict(o=o.detach(), lse=lse, dq=q.grad, dk=k.grad, dv=v.grad)


LAUNCH = dict(flash_second_order=_flash_second_order, unpool=_unpool, norm_conv_stats=_norm_conv_stats, rows=_rows, tanh_bwd_mul3=_tanh_bwd_mul3, spectral_norm_multi=_spectral_norm_multi, small_gemm=_small_gemm, scale_dev=_scale_dev, softmax_bwd_bwd=_softmax_bwd_bwd, lerp=_lerp, wgrad=_wgrad, pointwise=_pointwise, upcat_conv=_upcat_conv, mbstd=_mbstd, tanh=_tanh, dot=_dot, fully_connected=_fully_connected,
              cosine_distance=_cosine_distance, channel_sum=_channel_sum, cat_rows=_cat_rows, lrelu_bwd_bias=_lrelu_bwd_bias,
              spectral_norm=_spectral_norm, flash_attention=_flash_attention,
              softmax_rows=_softmax_rows, bgemm=_bgemm, conv=_conv, norm_act=_norm_act, pred_loss=_pred_loss, pred_losses=_pred_losses, abs_diff=_abs_diff, gradient_penalty=_gradient_penalty,
              variance=_variance, sums=_sums, axpby=_axpby, sample_lerp=_sample_lerp, gdrop=_gdrop, cast=_cast, lrelu_bwd=_lrelu_bwd,
              lrelu_pool_bwd=_lrelu_pool_bwd, pool=_pool, upsample_concat=_upsample_concat)


# ------------------------------------------------------------------------------------------------ the one test body
TRIPLES = [t for c in NF.CASES for t in c.triples()]


@pytest.mark.parametrize('case,dname,what', TRIPLES, ids=['%s-%s-%s' % (c.id, d, w) for c, d, w in TRIPLES])
def test_nonfinite_propagates_and_stays_contained(ops, case, dname, what):
  inputs = case.make(dname)
  planted = case.planted(inputs, dname, what)
  sets = case.expected(inputs, planted, dname)
  NF.check_case(sets, case.units)
  run = lambda inp: {k: host(v) for k, v in LAUNCH[case.family](ops, case, inp, dname).items()}
  base, again = run(inputs), run(inputs)
  got = run(planted)
  torch.cuda.synchronize()
  assert set(got) == set(sets), (sorted(got), sorted(sets))
  bound, failures = None, []
  for name, s in sorted(sets.items()):
    assert np.all(np.isfinite(base[name])), '%s %s: the unplanted launch is not finite' % (case.id, name)
    same = np.array_equal(base[name].view(np.int64), again[name].view(np.int64))
    assert same or name in case.atomic, '%s %s %s: two launches on the same inputs differ in bits, and the table does not list ' \
        'the output as meeting in atomics' % (case.id, dname, name)
    bitwise = same and name not in case.atomic
    if (not bitwise or s.touched.any()) and bound is None:
      bound = case.bound(planted, sets, dname)
    if not bitwise:
      BOUND_ROUTE.add((case.id, dname, name))
      print('[nonfinite] %s %s %s takes the bound route' % (case.id, dname, name))
    try:
      NF.assert_propagates_and_contains(got[name], base[name] if bitwise else None, s.taint, s.ref, None if bound is None else bound[name],
                                        '%s[%s,%s] %s' % (case.id, dname, what, name), touched=s.touched)
    except AssertionError as e:      # every output of the case is reported, not the first alone
      failures.append(str(e))
  assert not failures, '\n'.join(failures)


# ------------------------------------------------------------------------------------------------ tg_nonfinite_check
def test_nonfinite_check_over_several_ranges_before_one_tick():
  """Trainer._apply checks a group's ranges one after the other and ticks once: `found` goes up at the first range that holds
  an Inf or NaN and no later clean range takes it down.  One special value per range: element 0, the last element, the tail
  behind the last whole vector, a view one element off the 16-byte boundary (the element-by-element kernel), and a vector that
  the clamped second load re-reads (4099 elements: 3 workgroups, 768 lanes; lanes 256..767 find `i + 768` past the 1024 vectors
  and load vector i again) -- each after a clean range and followed by one."""
  from twingan_amd._lib import TgLossScaleState, call
  numel = 4099
  buf = torch.randn(numel + 8, generator=torch.Generator().manual_seed(5)).to(DEV)
  state = torch.zeros(8, dtype=torch.int32, device=DEV)
  state.copy_(torch.frombuffer(bytearray(bytes(TgLossScaleState(scale=4.0, seed=4.0, inv_scale=0.25, found=0, skip=0, good_steps=0,
                                                                skipped=0))), dtype=torch.int32))
  st = torch.cuda.current_stream().cuda_stream

  def found(x):
    call('tg_nonfinite_check', x.data_ptr(), x.numel(), state.data_ptr(), st)
    return TgLossScaleState.from_buffer_copy(state.cpu().numpy().tobytes()).found
  for off, pos, what in ((0, 0, '+inf'), (0, numel - 1, 'nan'), (0, numel // 4 * 4, '-inf'), (1, 2000, 'nan'), (3, numel - 1, '+inf'),
                         (0, 4 * 500, 'nan'), (0, 4 * 500 + 3, '-inf')):
    x = buf[off:off + numel]
    assert (x.data_ptr() % 16 == 0) == (off == 0)
    state[3] = 0
    assert found(x) == 0, 'a clean range raised the flag'
    keep = float(x[pos])
    x[pos] = NF.WHAT[what]
    assert found(x) == 1, '%s at element %d of the range at offset %d was not seen' % (what, pos, off)
    x[pos] = keep
    assert found(x) == 1 and found(buf[4:4 + 64]) == 1, 'a clean range reset the flag'
