"""Moving averages of the model variables (Config.moving_average_decay; model/model_inheritor.py:53-56,1063-1092,1150-1155):
the kernels element by element (tg_ema_update, tg_adam_ema_step, tg_ema_update_multi), the trainer's averages against a
float64 recomputation from its own snapshots -- eager and replayed from hipGraphs --, and the checkpoint round trip.

The per-element bound of one update avg <- avg - (avg - var) * w from the fp32 values the launch read:
  |got - want| <= 1.01 u (|want| + 2 |avg - var| w) + 2^-149,   u = 2^-24
-- three fp32 roundings (the difference, the product, the final subtraction; a fused multiply-add drops one of them)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import elementwise as E      # noqa: E402

pytestmark = pytest.mark.gpu

U = E.U32                       # the fp32 unit roundoff, 2^-24
SUBNORMAL = 2.0 ** -149
EMA = '/ExponentialMovingAverage'
DEV = 'cuda:0'
PAD = 64                        # canary elements on either side of a view (keeps the view's base 256-byte aligned)
CANARY = 7.0

# (numel, elements the views start into their buffers): one element, a partial / just over one workgroup, a size that is no
# multiple of the 16-byte vector, more than the grid cap covers in one sweep; 4-byte-aligned-only views
SIZES = [(1, 0), (255, 0), (257, 0), (4099, 0), (5000000, 0), (257, 1), (257, 3), (4099, 1), (4099, 3)]
_SIZE_ID = lambda p: '%d+%d' % p
WEIGHTS = [np.float32(0.9), np.float32(1) - np.float32(0.999)]


def _stream():
  return torch.cuda.current_stream().cuda_stream


def _view(numel, off, fill=None):
  """-> (buffer with canaries, view of numel elements starting PAD + off elements in)."""
  buf = torch.full((numel + 2 * PAD + 4,), CANARY, dtype=torch.float32, device=DEV)
  v = buf[PAD + off:PAD + off + numel]
  if fill is not None:
    v.copy_(fill)
  return buf, v


def _canaries_ok(buf, numel, off):
  return bool((buf[:PAD + off] == CANARY).all()) and bool((buf[PAD + off + numel:] == CANARY).all())


def ema_step_ref(a, x, w):
  """One update in float64 from the fp32 values (as float64 arrays) -> (want, bound)."""
  w = float(w)
  want = a - (a - x) * w
  return want, 1.01 * U * (np.abs(want) + 2.0 * np.abs(a - x) * w) + SUBNORMAL


def ema_weight(decay, n):
  """TF 1.8 ExponentialMovingAverage(decay, num_updates=n) in float32 -> w = 1 - min(decay, (1 + n) / (10 + n))."""
  n = np.float32(n)
  d = min(np.float32(decay), (np.float32(1) + n) / (np.float32(10) + n))
  return np.float32(1) - np.float32(d)


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize('w', WEIGHTS, ids=['w0.9', 'w0.001'])
@pytest.mark.parametrize('size', SIZES, ids=_SIZE_ID)
def test_ema_update_elementwise(size, w):
  """tg_ema_update, ten successive updates with a fresh ``var`` each, checked after every one against float64 from the fp32
  values the launch read.  Mixed into the randn inputs by element index: var == avg exactly (must come back bit-equal),
  avg = 0 at the start, var = 0, magnitudes 1e30 and 1e-30.  w is read from the device.  The views sit between canaries;
  avg and var start at different 4-byte-aligned offsets in the unaligned cases."""
  from twingan_amd._lib import call
  numel, off = size
  gen = torch.Generator().manual_seed(numel + 17 * off)
  kind = torch.arange(numel) % 8
  mag = torch.where(kind == 4, 1e30, torch.where(kind == 5, 1e-30, 1.0)).float()
  a0 = torch.randn(numel, generator=gen) * mag
  a0[kind == 2] = 0.0
  abuf, avg = _view(numel, off, a0)
  xoff = (4 - off) % 4
  xbuf, var = _view(numel, xoff)
  w_dev = torch.tensor([float(w)], dtype=torch.float32, device=DEV)
  assert np.float32(w_dev.item()) == w
  same = (kind == 1).to(DEV)
  worst = 0.0
  for step in range(10):
    x = torch.randn(numel, generator=gen) * mag
    x[kind == 3] = 0.0
    var.copy_(x)
    var[same] = avg[same]
    prev_a, prev_x = avg.clone(), var.clone()
    call('tg_ema_update', avg.data_ptr(), var.data_ptr(), numel, w_dev.data_ptr(), _stream())
    want, bound = ema_step_ref(prev_a.double().cpu().numpy(), prev_x.double().cpu().numpy(), w)
    worst = max(worst, E.assert_elementwise(avg.double().cpu().numpy(), want, bound, 'ema update %d' % step))
    assert torch.equal(avg[same].view(torch.int32), prev_a[same].view(torch.int32)), 'avg == var changed avg at update %d' % step
    assert torch.equal(var, prev_x), 'the launch wrote its input'
  assert _canaries_ok(abuf, numel, off) and _canaries_ok(xbuf, numel, xoff)
  print('ema update numel %d + %d, w %g: worst error / bound %.3f' % (numel, off, float(w), worst))


@pytest.mark.parametrize('size', SIZES, ids=_SIZE_ID)
def test_adam_ema_fused_equals_unfused(size):
  """Ten steps of tg_adam_tick + tg_adam_ema_step on one copy of the state against tg_adam_tick + tg_adam_step + tg_ema_update
  on another: theta, m, v and avg bit for bit after every step.  The gradient mix of test_adam_step_elementwise (g = 0
  throughout, |g| = 1e4, |g| = 1e-20, theta = 0; gradients times 1024 with grad_scale = 1 / 1024)."""
  from twingan_amd._lib import call
  numel, off = size
  gen = torch.Generator().manual_seed(numel % 1000 + off)
  ar = torch.arange(numel)
  kind = ar % 4
  scale = torch.where(kind == 1, 1e4, torch.where(kind == 2, 1e-20, torch.where(kind == 3, 0.0, 1.0))).double()
  th0 = torch.randn(numel, generator=gen)
  th0[ar % 8 == 0] = 0.0
  avg0 = torch.randn(numel, generator=gen)
  zero = torch.zeros(numel)
  sides = []
  for _ in range(2):      # [fused, unfused]: (buffer, view) of theta, m, v, avg + step counter and rate
    sides.append(dict(th=_view(numel, off, th0), m=_view(numel, off, zero), v=_view(numel, off, zero), avg=_view(numel, off, avg0),
                      step=torch.zeros(1, dtype=torch.int64, device=DEV), lr=torch.zeros(1, dtype=torch.float32, device=DEV)))
  gbuf, gdev = _view(numel, off)
  w_dev = torch.tensor([float(WEIGHTS[0])], dtype=torch.float32, device=DEV)
  st = _stream()
  p = lambda side, k: side[k][1].data_ptr()
  for t in range(1, 11):
    gdev.copy_((torch.randn(numel, generator=gen).double() * scale * 1024.0).float())
    f, u = sides
    for side in sides:
      call('tg_adam_tick', side['step'].data_ptr(), side['lr'].data_ptr(), 1e-4, 0.5, 0.99, st)
    call('tg_adam_ema_step', p(f, 'th'), gdev.data_ptr(), p(f, 'm'), p(f, 'v'), p(f, 'avg'), numel, f['lr'].data_ptr(), 0.5, 0.99,
         1e-8, 1.0 / 1024.0, w_dev.data_ptr(), st)
    call('tg_adam_step', p(u, 'th'), gdev.data_ptr(), p(u, 'm'), p(u, 'v'), None, numel, 0.0, u['lr'].data_ptr(), 0.5, 0.99, 1e-8,
         1.0 / 1024.0, st)
    call('tg_ema_update', p(u, 'avg'), p(u, 'th'), numel, w_dev.data_ptr(), st)
    for k in ('th', 'm', 'v', 'avg'):      # whole buffers: the canaries with them
      assert torch.equal(f[k][0].view(torch.int32), u[k][0].view(torch.int32)), '%s differs at step %d' % (k, t)
  for side in sides:
    for k in ('th', 'm', 'v', 'avg'):
      assert _canaries_ok(side[k][0], numel, off), k
  assert _canaries_ok(gbuf, numel, off)
  assert not torch.equal(sides[0]['avg'][1].cpu(), avg0) and not torch.equal(sides[0]['th'][1].cpu(), th0)


def _ema_table(pairs):
  """Device job table of tg_ema_update_multi over (avg, var) tensor pairs -> (table, njobs, total_blocks)."""
  from twingan_amd import _lib
  from twingan_amd._lib import call
  host = ctypes.create_string_buffer(_lib.load().tg_ema_table_bytes(len(pairs)))
  blocks = ctypes.c_int32(0)
  for j, (a, x) in enumerate(pairs):
    call('tg_ema_table_fill', a.data_ptr(), x.data_ptr(), a.numel(), j, ctypes.addressof(host), ctypes.byref(blocks))
  return torch.frombuffer(bytearray(host.raw), dtype=torch.uint8).to(DEV), len(pairs), blocks.value


@pytest.mark.parametrize('sizes', [[1, 3, 16, 255, 256, 1000] * 7 + [70000], [5]], ids=['43jobs', '1job'])
def test_ema_update_multi_matches_single(sizes):
  """tg_ema_update_multi over separately allocated tensors (each between canaries) equals tg_ema_update per tensor, bit for
  bit, over three updates; the canaries and the inputs are untouched."""
  from twingan_amd._lib import call
  gen = torch.Generator().manual_seed(len(sizes))
  multi, single, xs = [], [], []
  for i, n in enumerate(sizes):
    a0 = torch.randn(n, generator=gen)
    multi.append(_view(n, i % 4, a0))
    single.append(_view(n, i % 4, a0))
    xs.append(_view(n, (i + 1) % 4, torch.randn(n, generator=gen)))
  w_dev = torch.tensor([float(WEIGHTS[0])], dtype=torch.float32, device=DEV)
  tab, njobs, blocks = _ema_table([(m[1], x[1]) for m, x in zip(multi, xs)])
  assert njobs == len(sizes) and blocks == sum((n + 1023) // 1024 for n in sizes)
  x_before = [x[0].clone() for x in xs]
  for step in range(3):
    call('tg_ema_update_multi', tab.data_ptr(), njobs, blocks, w_dev.data_ptr(), _stream())
    for s, x in zip(single, xs):
      call('tg_ema_update', s[1].data_ptr(), x[1].data_ptr(), s[1].numel(), w_dev.data_ptr(), _stream())
    for i, (m, s) in enumerate(zip(multi, single)):
      assert torch.equal(m[0].view(torch.int32), s[0].view(torch.int32)), 'job %d (%d elements) at update %d' % (i, sizes[i], step)
  for i, n in enumerate(sizes):
    assert _canaries_ok(multi[i][0], n, i % 4)
    assert torch.equal(xs[i][0], x_before[i])
    assert not torch.equal(multi[i][1], torch.full_like(multi[i][1], CANARY))


def test_ema_errors_are_loud():
  """Null pointers, numel = 0 and njobs = 0 raise TgError and launch nothing."""
  from twingan_amd import _lib
  from twingan_amd._lib import TgError, call
  n = 64
  bufs = {k: torch.full((n,), 3.0, dtype=torch.float32, device=DEV) for k in ('th', 'g', 'm', 'v', 'avg', 'x')}
  lr = torch.full((1,), 1e-4, dtype=torch.float32, device=DEV)
  w = torch.full((1,), 0.5, dtype=torch.float32, device=DEV)
  p = {k: b.data_ptr() for k, b in bufs.items()}
  st = _stream()
  adam = [p['th'], p['g'], p['m'], p['v'], p['avg'], n, lr.data_ptr(), 0.5, 0.99, 1e-8, 1.0, w.data_ptr(), st]
  for i in (0, 1, 2, 3, 4, 6, 11):
    bad = list(adam)
    bad[i] = None
    with pytest.raises(TgError):
      call('tg_adam_ema_step', *bad)
  for numel in (0, -5):
    with pytest.raises(TgError):
      call('tg_adam_ema_step', *(adam[:5] + [numel] + adam[6:]))
    with pytest.raises(TgError):
      call('tg_ema_update', p['avg'], p['x'], numel, w.data_ptr(), st)
  for bad in ((None, p['x'], n, w.data_ptr(), st), (p['avg'], None, n, w.data_ptr(), st), (p['avg'], p['x'], n, None, st)):
    with pytest.raises(TgError):
      call('tg_ema_update', *bad)
  host = ctypes.create_string_buffer(max(_lib.load().tg_ema_table_bytes(1), 1))
  blocks = ctypes.c_int32(0)
  assert _lib.load().tg_ema_table_bytes(0) == 0
  for bad in ((None, p['x'], n), (p['avg'], None, n), (p['avg'], p['x'], 0)):
    with pytest.raises(TgError):
      call('tg_ema_table_fill', bad[0], bad[1], bad[2], 0, ctypes.addressof(host), ctypes.byref(blocks))
  with pytest.raises(TgError):
    call('tg_ema_table_fill', p['avg'], p['x'], n, 0, None, ctypes.byref(blocks))
  assert blocks.value == 0
  tab, njobs, total = _ema_table([(bufs['avg'], bufs['x'])])
  for bad in ((None, 1, total, w.data_ptr(), st), (tab.data_ptr(), 0, total, w.data_ptr(), st), (tab.data_ptr(), 1, 0, w.data_ptr(), st),
              (tab.data_ptr(), 1, total, None, st)):
    with pytest.raises(TgError):
      call('tg_ema_update_multi', *bad)
  torch.cuda.synchronize()
  for k, b in bufs.items():
    assert bool((b == 3.0).all()), '%s was written by a refused call' % k


# ------------------------------------------------------------------------------------------------ trainer
def _cfg(**kw):
  from twingan_amd import Config
  return Config(hw=32, max_ch=16, precision='fp32', loss_architecture='wgan', **kw)


def _batch(seed=9):
  g = torch.Generator().manual_seed(seed)
  return torch.rand(2, 32, 32, 3, generator=g).to(DEV), torch.rand(2, 32, 32, 3, generator=g).to(DEV)


def _snap(tr):
  return {k: v.double().cpu().numpy() for k, v in tr.store.state_dict(include_state=True).items()}


def _check_averages(tr, start, snaps, steps, decay, what):
  """``start``: {name: float64 array} the averages before the first of the runs; ``snaps[i]`` the variables after run i,
  ``steps[i]`` the global step when run i was entered.  Recomputes every model variable's average in float64 with float32
  weights, sums the per-update bounds, and compares with the trainer's averages_dict()."""
  from twingan_amd.params import is_model_variable
  names = [k for k in snaps[0] if is_model_variable(k)]
  avg = {k: np.array(start[k], dtype=np.float64) for k in names}
  bound = {k: np.zeros_like(avg[k]) for k in names}
  for snap, n in zip(snaps, steps):
    w = ema_weight(decay, n)
    for k in names:
      avg[k], b = ema_step_ref(avg[k], snap[k], w)
      bound[k] = bound[k] + b
  got = tr.store.averages_dict()
  assert set(got) == {k + EMA for k in names}, 'the averaged variables are the model variables'
  assert not any(k.endswith('/sa_gamma' + EMA) for k in got)
  worst = 0.0
  for k in names:
    g = got[k + EMA].double().cpu().numpy()
    assert g.shape == avg[k].shape, (k, g.shape, avg[k].shape)
    worst = max(worst, E.assert_elementwise(g, avg[k], bound[k], '%s: average of %s' % (what, k)))
  return worst


def _run_and_check(tr, decay, runs, what):
  s, t = _batch()
  start = _snap(tr)
  assert tr.global_step == 0
  snaps, steps = [], []
  for i in range(runs):
    steps.append(tr.global_step)
    tr.run(s, t)
    if i == 0 and tr.use_graph:
      assert tr.graph_fallback_reason is None, tr.graph_fallback_reason
    snaps.append(_snap(tr))
  assert steps == [i // 2 for i in range(runs)]      # n_critic = 2: both runs of a G+D pair see the same global step
  moved = max(float(np.abs(snaps[-1][k] - start[k]).max()) for k in start)
  assert moved > 0.0
  worst = _check_averages(tr, start, snaps, steps, decay, what)
  print('%s: worst error / bound %.3f' % (what, worst))
  return start, snaps


@pytest.mark.parametrize('decay', [0.999, 0.05])
@pytest.mark.parametrize('norm', ['instance_norm', 'batch_norm'])
def test_trainer_averages_match_float64(norm, decay):
  """Six eager runs: every average equals the float64 recomputation from the trainer's own snapshots -- n the global step on
  entering the run, the post-run values of all model variables, every run (a discriminator run moves the generator's averages
  towards its unchanged weights).  decay 0.999: the ramp (1 + n) / (10 + n) is active; 0.05: the configured value is."""
  from twingan_amd.twingan import Trainer
  tr = Trainer(_cfg(generator_norm_type=norm, moving_average_decay=decay), device=DEV, seed=4)
  start, snaps = _run_and_check(tr, decay, 6, '%s decay %g' % (norm, decay))
  if norm == 'batch_norm':
    assert any('moving_mean' in k for k in start)
    k = 'generator/block_4x4x16/Conv/BatchNorm/moving_mean_s'
    assert float(np.abs(snaps[-1][k] - start[k]).max()) > 0.0      # a state variable that moves is among the averaged
  tr.close()


def test_trainer_averages_attention_gate_is_live():
  """--do_self_attention (with spectral norm, so that the power-iteration vectors u are among the state): sa_gamma is no model
  variable -- it has no average, and averaged_state_dict() carries its live value next to the averaged ones."""
  from twingan_amd.twingan import Trainer
  tr = Trainer(_cfg(do_self_attention=True, self_attention_hw=16, spectral_norm=True, moving_average_decay=0.999), device=DEV, seed=4)
  start, snaps = _run_and_check(tr, 0.999, 4, 'attention + spectral norm')
  gates = [k for k in start if k.endswith('/sa_gamma')]
  assert gates and any(k.endswith('/u') for k in start)
  live, sd, avgs = tr.store.state_dict(include_state=True), tr.store.averaged_state_dict(), tr.store.averages_dict()
  assert set(sd) == set(live)
  assert any(float(live[k].abs().max()) > 0.0 for k in gates), 'the gates did not train'
  for k in live:
    if k in gates:
      assert torch.equal(sd[k], live[k])
    else:
      assert torch.equal(sd[k], avgs[k + EMA]) and sd[k].shape == live[k].shape
  assert set(tr.store.averaged_state_dict(include_state=False)) == set(tr.store.state_dict())
  tr.close()


@pytest.mark.parametrize('norm', ['instance_norm', 'batch_norm'])
def test_trainer_averages_graph_replay(norm):
  """The same check on Trainer(use_graph=True): the three launches replay inside the captured apply graphs and read the
  current weight from the device scalar.  The recomputation starts at the initial values, so it also proves that the capture's
  undone warm-up left no trace in the averages."""
  from twingan_amd.twingan import Trainer
  tr = Trainer(_cfg(generator_norm_type=norm, moving_average_decay=0.999), device=DEV, seed=4, use_graph=True)
  _run_and_check(tr, 0.999, 6, '%s replayed' % norm)
  assert tr.use_graph and tr.graph_fallback_reason is None, tr.graph_fallback_reason
  tr.close()


def test_averaging_does_not_disturb_training():
  """Two trainers of one seed, with and without averages, five runs: the same trajectory to what two trainers of this
  configuration are allowed (test_graph_replay_matches_eager_steps: 5e-3 relative L2); no average buffers without the flag."""
  from twingan_amd.twingan import Trainer
  s, t = _batch()
  a = Trainer(_cfg(generator_norm_type='batch_norm', moving_average_decay=0.999), device=DEV, seed=4)
  b = Trainer(_cfg(generator_norm_type='batch_norm'), device=DEV, seed=4)
  assert b.cfg.moving_average_decay is None and not b.store.averaged and b.store.avg == {} and b.store.state_avg == {}
  assert not hasattr(b, '_ema_w_dev')
  assert set(a.store.avg) == {'g', 'd'} and all(a.store.avg[g].shape == a.store.slots[g][0].shape for g in 'gd')
  for _ in range(5):
    a.run(s, t)
    b.run(s, t)
  torch.cuda.synchronize()
  assert (a.adam_t, a.n_critic_counter, a.global_step) == (b.adam_t, b.n_critic_counter, b.global_step) == (5, 5, 2)
  sa, sb = a.store.state_dict(include_state=True), b.store.state_dict(include_state=True)
  assert set(sa) == set(sb)
  num = sum(float(((sa[k] - sb[k]).double() ** 2).sum()) for k in sa)
  den = sum(float((sa[k].double() ** 2).sum()) for k in sa)
  assert (num / den) ** 0.5 < 5e-3, (num / den) ** 0.5
  with pytest.raises(AssertionError):
    b.store.averages_dict()
  a.close()
  b.close()
  assert a.store.avg == {} and a.store.state_avg == {}


# ------------------------------------------------------------------------------------------------ checkpoints
CKPT_NORM = 'batch_norm'
CKPT_DECAY = 0.999


@pytest.fixture(scope='module')
def trained(tmp_path_factory):
  """One averaging trainer after three runs and its checkpoint, and a checkpoint of the same configuration without averages."""
  from twingan_amd import checkpoint as ckpt
  from twingan_amd.twingan import Trainer
  root = tmp_path_factory.mktemp('ema')
  s, t = _batch()
  tr = Trainer(_cfg(generator_norm_type=CKPT_NORM, moving_average_decay=CKPT_DECAY), device=DEV, seed=4)
  plain = Trainer(_cfg(generator_norm_type=CKPT_NORM), device=DEV, seed=4)
  for _ in range(3):
    tr.run(s, t)
    plain.run(s, t)
  with_avg = ckpt.save(tr, str(root / 'avg'))
  without = ckpt.save(plain, str(root / 'plain'))
  plain.close()
  return dict(trainer=tr, dir=str(root / 'avg'), prefix=with_avg, plain_prefix=without, batch=(s, t))


def test_checkpoint_round_trip_carries_the_averages(trained):
  """save -> restore into a fresh trainer of another seed: the averages are the saved ones exactly, and a further run updates
  them from the restored values (the float64 check again).  Key sets: without the flag exactly today's; with it, those plus
  '<var>/ExponentialMovingAverage' of every model variable.  A checkpoint without averages does not restore into an averaging
  trainer: KeyError naming the first missing key."""
  from twingan_amd import checkpoint as ckpt
  from twingan_amd.params import is_model_variable
  from twingan_amd.twingan import Trainer
  tr = trained['trainer']
  saved = tr.store.averages_dict()
  fresh = Trainer(_cfg(generator_norm_type=CKPT_NORM, moving_average_decay=CKPT_DECAY), device=DEV, seed=11)
  k0 = 'generator/block_4x4x16/Conv/weights' + EMA
  assert not torch.equal(fresh.store.averages_dict()[k0], saved[k0])
  assert ckpt.restore(fresh, trained['prefix']) == tr.global_step == 1
  got = fresh.store.averages_dict()
  assert set(got) == set(saved) and all(torch.equal(got[k], saved[k]) for k in saved)
  start = {k[:-len(EMA)]: v.double().cpu().numpy() for k, v in got.items()}
  n = fresh.global_step
  fresh.run(*trained['batch'])
  _check_averages(fresh, start, [_snap(fresh)], [n], CKPT_DECAY, 'the run after restore')
  # key sets
  variables = list(tr.store.specs) + list(tr.store.state_specs)
  today = set(variables) | {k + sfx for k in tr.store.specs for sfx in ('/Adam', '/Adam_1')} | \
      {'beta1_power', 'beta2_power', 'global_step', 'n_critic_counter', ckpt.RNG_DRAWS_KEY}
  shadows = {k + EMA for k in variables if is_model_variable(k)}
  assert len(shadows) == len(variables) and shadows
  assert set(ckpt.read_checkpoint(trained['plain_prefix'])) == today
  assert set(ckpt.read_checkpoint(trained['prefix'])) == today | shadows
  with pytest.raises(KeyError) as err:
    ckpt.restore(fresh, trained['plain_prefix'])
  assert EMA in str(err.value)
  # a trainer without averages ignores the shadows of a checkpoint that has them
  plain = Trainer(_cfg(generator_norm_type=CKPT_NORM), device=DEV, seed=12)
  ckpt.restore(plain, trained['prefix'])
  assert plain.store.avg == {} and torch.equal(plain.store.state_dict()[k0[:-len(EMA)]], tr.store.state_dict()[k0[:-len(EMA)]])
  fresh.close()
  plain.close()


def test_warm_start_and_inference_with_averages(trained):
  """runner.warm_start and checkpoint.init_from_checkpoint load the variables and leave the averages at the new trainer's
  initial values.  ImageInferer.from_checkpoint(moving_average=True) translates with the shadows: the same images as
  ImageInferer over averaged_state_dict(), other images than the raw weights give."""
  from twingan_amd import checkpoint as ckpt
  from twingan_amd.inference import ImageInferer
  from twingan_amd.runner import warm_start
  from twingan_amd.twingan import Trainer
  tr = trained['trainer']
  cfg = _cfg(generator_norm_type=CKPT_NORM, moving_average_decay=CKPT_DECAY)
  k0 = 'generator/block_4x4x16/Conv/weights'
  for how in ('warm_start', 'init_from_checkpoint'):
    new = Trainer(cfg, device=DEV, seed=21)
    init = new.store.averages_dict()
    if how == 'warm_start':
      loaded = warm_start(new, tr.store.state_dict(include_state=True))
    else:
      loaded = ckpt.init_from_checkpoint(new, trained['dir'])
    assert k0 in loaded and torch.equal(new.store.state_dict()[k0], tr.store.state_dict()[k0])
    after = new.store.averages_dict()
    assert all(torch.equal(after[k], init[k]) for k in init), how
    assert not torch.equal(after[k0 + EMA], new.store.state_dict()[k0])
    new.close()
  images = (trained['batch'][0].float().cpu().numpy() * 255.0).astype(np.uint8)
  from_file = ImageInferer.from_checkpoint(cfg, trained['dir'], device=DEV, moving_average=True).infer(images)
  from_store = ImageInferer(cfg, tr.store.averaged_state_dict(), device=DEV).infer(images)
  raw = ImageInferer.from_checkpoint(cfg, trained['dir'], device=DEV, moving_average=False).infer(images)
  assert from_file.shape == (2, 32, 32, 3) and np.isfinite(from_file).all()
  assert np.array_equal(from_file, from_store)
  assert not np.array_equal(from_file, raw)
  assert np.array_equal(raw, ImageInferer(cfg, tr.store.state_dict(include_state=True), device=DEV).infer(images))
