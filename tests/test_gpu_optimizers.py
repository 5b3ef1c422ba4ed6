"""The --optimizer rules besides Adam (Config.optimizer; model/model_inheritor.py:516-565): tg_optim_step element by element
against tests/optim_ref.py, fused against unfused bit for bit, the dynamic-loss-scale guard, the argument errors, and the
trainer -- eager, replayed from hipGraphs, averaged, loss-scaled -- with the checkpoint round trip.  Also runnable over the
emulated kernels (TG_EMU=1), the graph replays excepted."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import elementwise as E      # noqa: E402
import optim_ref as R        # noqa: E402

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
PAD = 64                        # canary elements on either side of a view (keeps the view's base 256-byte aligned)
CANARY = 7.0
LR = 1e-3
GSCALE = 1.0 / 1024.0
W = float(np.float32(0.9))
# (numel, elements the views start into their buffers, steps): one element, fewer than a vector, a partial / just over one
# workgroup, no multiple of the 16-byte vector; a 4-byte-aligned-only view (the element-by-element kernels); more than the
# 4096-workgroup cap covers in one sweep of 16-byte accesses
SIZES = [(1, 0, 10), (3, 0, 10), (255, 0, 10), (257, 0, 10), (1027, 0, 10), (1027, 1, 10), (5000000, 0, 2)]
_SIZE_ID = lambda p: '%d+%d' % p[:2]


def _stream():
  return torch.cuda.current_stream().cuda_stream


def _view(numel, off, fill=None):
  """-> (buffer with canaries, view of numel elements starting PAD + off elements in)."""
  buf = torch.full((numel + 2 * PAD + 4,), CANARY, dtype=torch.float32, device=DEV)
  v = buf[PAD + off:PAD + off + numel]
  if fill is not None:
    v.copy_(torch.as_tensor(fill))
  return buf, v


def _canaries_ok(buf, numel, off):
  return bool((buf[:PAD + off] == CANARY).all()) and bool((buf[PAD + off + numel:] == CANARY).all())


def _bits(t):
  return t.view(torch.int32)


def _hyper(rule, **kw):
  from twingan_amd._lib import TgOptimHyper
  h = R.default_hyper(rule, lr=LR)._replace(**kw)
  return h, TgOptimHyper(*h)


def _mix(numel, gen):
  """The gradient mix of test_adam_step_elementwise: by element index |g| ordinary, 1e4, 1e-20, identically 0; theta = 0 on
  every eighth element."""
  ar = torch.arange(numel)
  kind = ar % 4
  scale = torch.where(kind == 1, 1e4, torch.where(kind == 2, 1e-20, torch.where(kind == 3, 0.0, 1.0))).double()
  th0 = torch.randn(numel, generator=gen)
  th0[ar % 8 == 0] = 0.0
  return kind, scale, th0


def _draw(numel, gen, scale):
  return (torch.randn(numel, generator=gen).double() * scale * 1024.0).float()


def _side(rule, numel, off, th0, avg0=None):
  """One copy of the state a rule owns: theta, its slots at their initial values, the average."""
  side = dict(th=_view(numel, off, th0), slots=[_view(numel, off, torch.from_numpy(x)) for x in R.slot_init(rule, numel)])
  if avg0 is not None:
    side['avg'] = _view(numel, off, avg0)
  return side


def _apply(rule, side, g, numel, chyper, gscale=GSCALE, guard=None, w_dev=None):
  from twingan_amd._lib import call
  p = [s[1].data_ptr() for s in side['slots']] + [None, None]
  avg = side['avg'][1].data_ptr() if w_dev is not None else None
  call('tg_optim_step', R.RULE_ID[rule], side['th'][1].data_ptr(), g.data_ptr(), p[0], p[1], avg, numel, ctypes.byref(chyper),
       gscale, guard, w_dev.data_ptr() if w_dev is not None else None, _stream())


def _buffers(side):
  return [('theta', side['th'])] + [('slot%d' % i, s) for i, s in enumerate(side['slots'])] + \
      ([('avg', side['avg'])] if 'avg' in side else [])


def _state(scale, skip):
  from twingan_amd._lib import TgLossScaleState
  st = TgLossScaleState(scale=scale, seed=scale, inv_scale=1.0 / scale, found=0, skip=skip, good_steps=0, skipped=0)
  buf = torch.full((24,), 0x5a5a5a5a, dtype=torch.int32, device=DEV)
  buf[8:16].copy_(torch.frombuffer(bytearray(bytes(st)), dtype=torch.int32))
  return buf, buf[8:16]


# ------------------------------------------------------------------------------------------------ kernel
@pytest.mark.parametrize('size', SIZES, ids=_SIZE_ID)
@pytest.mark.parametrize('rule', R.RULES)
def test_optim_step_elementwise(rule, size):
  """tg_optim_step, plain form, grad_scale = 1 / 1024 on gradients times 1024: after EVERY step theta and each slot lie inside
  the bounds of optim_ref.step -- one step in float64 from the fp32 state the launch read.  Elements whose gradient is 0
  throughout keep theta and the slots bit for bit, but for rmsprop's mean square (it decays) and ftrl (linear stays 0, so
  TF's rule writes theta = 0: asserted as such)."""
  numel, off, steps = size
  gen = torch.Generator().manual_seed(numel % 1000 + off)
  kind, scale, th0 = _mix(numel, gen)
  h, ch = _hyper(rule)
  side = _side(rule, numel, off, th0)
  gbuf, g = _view(numel, off)
  start = [b[1].clone() for _, b in _buffers(side)]
  worst = 0.0
  for t in range(steps):
    g.copy_(_draw(numel, gen, scale))
    prev = [b[1].double().cpu().numpy() for _, b in _buffers(side)]
    gprev = g.clone()
    _apply(rule, side, g, numel, ch)
    refs, bounds = R.step(rule, prev[0], gprev.double().cpu().numpy(), prev[1:], h, GSCALE)
    for (nm, b), ref, bound in zip(_buffers(side), refs, bounds):
      worst = max(worst, E.assert_elementwise(b[1].double().cpu().numpy(), ref, bound, '%s %s step %d' % (rule, nm, t)))
    assert torch.equal(g, gprev), 'the launch wrote its gradient'
  zero = (kind == 3).to(DEV)
  for i, ((nm, b), was) in enumerate(zip(_buffers(side), start)):
    if rule == 'ftrl' and nm == 'theta':
      assert bool((b[1][zero] == 0).all()), 'ftrl: linear == 0 must write theta = 0'
    elif rule == 'rmsprop' and nm == 'slot0':
      assert numel < 4 or bool((b[1][zero] < was[zero]).all()), 'rmsprop: the mean square of g = 0 decays'
    else:
      assert torch.equal(_bits(b[1][zero]), _bits(was[zero])), '%s: %s moved where g = 0 throughout' % (rule, nm)
    assert _canaries_ok(b[0], numel, off), nm
  assert _canaries_ok(gbuf, numel, off)
  assert not torch.equal(side['th'][1], start[0])
  print('optim %s numel %d + %d: worst error / bound %.3f' % (rule, numel, off, worst))


def test_ftrl_learning_rate_power_elementwise():
  """ftrl with lr_power = -0.3 (the powf instantiation), l1 and l2 set: five steps of 1027 elements inside the bounds."""
  numel, off = 1027, 0
  gen = torch.Generator().manual_seed(5)
  _, scale, th0 = _mix(numel, gen)
  h, ch = _hyper('ftrl', lr_power=-0.3, l1=1e-3, l2=0.05)
  side = _side('ftrl', numel, off, th0)
  _, g = _view(numel, off)
  for t in range(5):
    g.copy_(_draw(numel, gen, scale))
    prev = [b[1].double().cpu().numpy() for _, b in _buffers(side)]
    _apply('ftrl', side, g, numel, ch)
    refs, bounds = R.step('ftrl', prev[0], g.double().cpu().numpy(), prev[1:], h, GSCALE)
    for (nm, b), ref, bound in zip(_buffers(side), refs, bounds):
      E.assert_elementwise(b[1].double().cpu().numpy(), ref, bound, 'ftrl^-0.3 %s step %d' % (nm, t))


@pytest.mark.parametrize('size', [(1027, 0), (1027, 1), (4099, 0), (4099, 3)], ids=_SIZE_ID)
@pytest.mark.parametrize('rule', R.RULES)
def test_optim_fused_equals_unfused(rule, size):
  """tg_optim_step with the average on one copy of the state against tg_optim_step without it followed by tg_ema_update on
  another: theta, the slots and the average bit for bit after each of ten steps (whole buffers, the canaries with them)."""
  from twingan_amd._lib import call
  numel, off = size
  gen = torch.Generator().manual_seed(numel + off)
  _, scale, th0 = _mix(numel, gen)
  avg0 = torch.randn(numel, generator=gen)
  _, ch = _hyper(rule)
  f, u = _side(rule, numel, off, th0, avg0), _side(rule, numel, off, th0, avg0)
  gbuf, g = _view(numel, off)
  w_dev = torch.tensor([W], dtype=torch.float32, device=DEV)
  for t in range(10):
    g.copy_(_draw(numel, gen, scale))
    _apply(rule, f, g, numel, ch, w_dev=w_dev)
    _apply(rule, u, g, numel, ch)
    call('tg_ema_update', u['avg'][1].data_ptr(), u['th'][1].data_ptr(), numel, w_dev.data_ptr(), _stream())
    for (nm, a), (_, b) in zip(_buffers(f), _buffers(u)):
      assert torch.equal(_bits(a[0]), _bits(b[0])), '%s: %s differs at step %d' % (rule, nm, t)
  assert all(_canaries_ok(b[0], numel, off) for _, b in _buffers(f)) and _canaries_ok(gbuf, numel, off)
  assert not torch.equal(f['avg'][1].cpu(), avg0) and not torch.equal(f['th'][1].cpu(), th0)


@pytest.mark.parametrize('size', [(1027, 0), (1027, 1)], ids=_SIZE_ID)
@pytest.mark.parametrize('rule', R.RULES)
def test_optim_guard(rule, size):
  """skip = 1: theta and the slots are bit-identical before and after, the average equals tg_ema_update of the old theta.
  skip = 0 with inv_scale = 1 / 1024: bit-identical to the plain call with grad_scale = 1 / 1024, fused and not."""
  from twingan_amd._lib import call
  numel, off = size
  gen = torch.Generator().manual_seed(numel + off + 3)
  _, scale, th0 = _mix(numel, gen)
  avg0 = torch.randn(numel, generator=gen)
  _, ch = _hyper(rule)
  w_dev = torch.tensor([W], dtype=torch.float32, device=DEV)
  gbuf, g = _view(numel, off)
  g.copy_(_draw(numel, gen, scale))
  for fused in (False, True):
    a, b = _side(rule, numel, off, th0, avg0), _side(rule, numel, off, th0, avg0)
    _, skip = _state(1024.0, 1)
    before = [x[0].clone() for _, x in _buffers(a)]
    _apply(rule, a, g, numel, ch, gscale=123.0, guard=skip.data_ptr(), w_dev=w_dev if fused else None)
    if fused:
      call('tg_ema_update', b['avg'][1].data_ptr(), b['th'][1].data_ptr(), numel, w_dev.data_ptr(), _stream())
    for (nm, x), was, (_, y) in zip(_buffers(a), before, _buffers(b)):
      if nm == 'avg' and fused:
        assert torch.equal(_bits(x[0]), _bits(y[0])) and not torch.equal(_bits(x[0]), _bits(was)), 'the average of a skipped apply'
      else:
        assert torch.equal(_bits(x[0]), _bits(was)), '%s: a skipped apply wrote %s' % (rule, nm)
    sbuf, go = _state(1024.0, 0)
    for t in range(3):
      _apply(rule, a, g, numel, ch, gscale=123.0, guard=go.data_ptr(), w_dev=w_dev if fused else None)
      _apply(rule, b, g, numel, ch, gscale=GSCALE, w_dev=w_dev if fused else None)
      for (nm, x), (_, y) in zip(_buffers(a), _buffers(b)):
        assert torch.equal(_bits(x[0]), _bits(y[0])), '%s: guarded %s differs from the plain call at step %d' % (rule, nm, t)
    assert bool((sbuf[:8] == 0x5a5a5a5a).all()) and bool((sbuf[16:] == 0x5a5a5a5a).all())
    assert not torch.equal(a['th'][1].cpu(), th0)
  assert _canaries_ok(gbuf, numel, off)


def test_optim_errors_are_loud():
  """Every argument error raises TgError with the argument's name, and nothing is launched."""
  from twingan_amd import _lib
  from twingan_amd._lib import TgError, call
  n = 64
  bufs = {k: torch.full((n,), 3.0, dtype=torch.float32, device=DEV) for k in ('th', 'g', 's0', 's1', 'avg')}
  w = torch.full((1,), 0.5, dtype=torch.float32, device=DEV)
  p = {k: b.data_ptr() for k, b in bufs.items()}
  _, ch = _hyper('rmsprop')
  hp, st = ctypes.byref(ch), _stream()
  good = lambda rule: [rule, p['th'], p['g'], p['s0'], p['s1'], p['avg'], n, hp, 1.0, None, w.data_ptr(), st]
  lib = _lib.load()
  assert [lib.tg_optim_slot_count(r) for r in range(6)] == [0, 1, 1, 2, 2, 2]
  assert lib.tg_optim_slot_count(-1) < 0 and lib.tg_optim_slot_count(6) < 0

  def refused(args, word):
    with pytest.raises(TgError) as e:
      call('tg_optim_step', *args)
    assert word in str(e.value), (word, str(e.value))
  for rule in (-1, 6, 99):
    refused(good(rule), 'rule')
  for i, word in ((1, 'theta'), (2, 'grad'), (7, 'hyper')):
    bad = good(3)
    bad[i] = None
    refused(bad, word)
  for numel in (0, -5):
    bad = good(3)
    bad[6] = numel
    refused(bad, 'numel')
  for rule, i, word in ((1, 3, 'slot0'), (2, 3, 'slot0'), (3, 3, 'slot0'), (3, 4, 'slot1'), (4, 4, 'slot1'), (5, 3, 'slot0'), (5, 4, 'slot1')):
    bad = good(rule)
    bad[i] = None
    refused(bad, word)
  bad = good(0)
  bad[10] = None
  refused(bad, 'w_dev')      # avg without w_dev
  bad = good(0)
  bad[5] = None
  refused(bad, 'avg')        # w_dev without avg
  _, pos = _hyper('ftrl', lr_power=0.5)
  bad = good(5)
  bad[7] = ctypes.byref(pos)
  refused(bad, 'lr_power')
  torch.cuda.synchronize()
  for k, b in bufs.items():
    assert bool((b == 3.0).all()), '%s was written by a refused call' % k
  # the slots a rule lacks may be null, and are not touched when they are not
  call('tg_optim_step', 0, p['th'], p['g'], None, None, None, n, hp, 1.0, None, None, st)
  call('tg_optim_step', 1, p['th'], p['g'], p['s0'], None, None, n, hp, 1.0, None, None, st)
  torch.cuda.synchronize()
  assert bool((bufs['s1'] == 3.0).all()) and bool((bufs['avg'] == 3.0).all()) and not bool((bufs['th'] == 3.0).any())


# ------------------------------------------------------------------------------------------------ trainer
HW = 16


class _Deterministic:
  def __enter__(self):
    from twingan_amd import _lib
    self.lib = _lib.load()
    self.was = self.lib.tg_set_deterministic(1)

  def __exit__(self, *exc):
    self.lib.tg_set_deterministic(self.was)


def _cfg(**kw):
  from twingan_amd import Config
  kw.setdefault('precision', 'fp32')
  return Config(hw=HW, max_ch=8, **kw)


def _batch(dtype=torch.float32):
  g = torch.Generator().manual_seed(8)
  s, t = torch.rand(2, HW, HW, 3, generator=g), torch.rand(2, HW, HW, 3, generator=g)
  return s.to(DEV).to(dtype), t.to(DEV).to(dtype)


def _trainer_hyper(cfg):
  rule = cfg.optimizer
  return R.Hyper(lr=cfg.learning_rate, momentum=cfg.rmsprop_momentum if rule == 'rmsprop' else cfg.momentum,
                 decay_or_rho=cfg.adadelta_rho if rule == 'adadelta' else cfg.rmsprop_decay, eps=cfg.opt_epsilon,
                 lr_power=cfg.ftrl_learning_rate_power, l1=cfg.ftrl_l1, l2=cfg.ftrl_l2)


def _owned(tr, group):
  s = tr.store
  return [s.flat[group].detach().clone()] + [t.clone() for t in s.slots[group]]


def _everything(tr):
  s = tr.store
  out = {'flat/' + g: s.flat[g].detach().clone() for g in s.GROUPS}
  out.update({'slot%d/%s' % (i, g): t.clone() for g in s.GROUPS for i, t in enumerate(s.slots[g])})
  out.update({'avg/' + g: t.clone() for g, t in s.avg.items()})
  return out


def _differing(a, b):
  return [k for k in a if not torch.equal(_bits(a[k]), _bits(b[k]))]


def _variables(tr):
  """Every variable and every slot variable by its checkpoint name (the flat buffers' alignment padding is no variable)."""
  out = dict(tr.store.state_dict(include_state=True))
  out.update(tr.store.slot_dict())
  return out


@pytest.mark.parametrize('rule', R.RULES)
def test_trainer_applies_match_float64(rule):
  """Four eager runs (two applies per group) from the seeded state: after each apply the group's theta and slots equal the
  float64 rule applied to the theta, the slots and the flat gradient the apply consumed, element by element; the other group
  is untouched; the slots start at the table's values and the counters advance as under Adam."""
  from twingan_amd.twingan import Trainer
  tr = Trainer(_cfg(optimizer=rule), device=DEV, seed=3)
  st = tr.store
  assert not hasattr(st, 'm') and not hasattr(st, 'v')      # no Adam moments beside the rule's own slots
  for g in st.GROUPS:
    assert len(st.slots[g]) == len(R.SLOT_NAMES[rule])
    for t, want in zip(st.slots[g], R.slot_init(rule, 1)):
      assert t.numel() == st.flat[g].numel() and bool((t == float(want[0])).all())
  s, t = _batch()
  h = _trainer_hyper(tr.cfg)
  worst = 0.0
  for i in range(4):
    group, other = ('g', 'd') if i % 2 == 0 else ('d', 'g')
    before, rest = _owned(tr, group), _owned(tr, other)
    tr.run(s, t)
    grad = st.grad[group].double().cpu().numpy()      # the flat gradient the apply read: cleared only by the group's next run
    assert np.isfinite(grad).all() and np.abs(grad).max() > 0
    refs, bounds = R.step(rule, before[0].double().cpu().numpy(), grad, [x.double().cpu().numpy() for x in before[1:]], h, 1.0)
    for j, (got, ref, bound) in enumerate(zip(_owned(tr, group), refs, bounds)):
      worst = max(worst, E.assert_elementwise(got.double().cpu().numpy(), ref, bound, '%s run %d: %s' % (rule, i, 'theta slot0 slot1'.split()[j])))
    assert i >= 2 or not torch.equal(before[0], st.flat[group].detach()), 'the first apply of %s moved nothing' % group
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(rest, _owned(tr, other))), 'run %d touched the other group' % i
  assert (tr.adam_t, tr.n_critic_counter, tr.global_step) == (4, 4, 2) and int(tr._adam_step_dev.item()) == 4
  print('trainer %s: worst error / bound %.3f' % (rule, worst))
  tr.close()


def test_trainer_adam_moments_are_slots_and_snapshot_restores_them():
  """optimizer='adam': after two runs slots[g] is [m, v], two buffers of flat[g]'s shape with v >= 0 everywhere and both groups'
  moments moved; _snapshot -> one more run -> _restore leaves every buffer as it was before that run, bit for bit."""
  from twingan_amd.twingan import Trainer
  tr = Trainer(_cfg(optimizer='adam', moving_average_decay=0.999), device=DEV, seed=3)
  st = tr.store
  s, t = _batch()
  tr.run(s, t)
  tr.run(s, t)
  for g in st.GROUPS:
    assert len(st.slots[g]) == 2 and all(x.shape == st.flat[g].shape and x.dtype == torch.float32 for x in st.slots[g])
    assert bool((st.slots[g][1] >= 0).all()) and float(st.slots[g][1].max()) > 0 and float(st.slots[g][0].abs().max()) > 0
  before = _everything(tr)
  counters = (tr.adam_t, tr.n_critic_counter, tr.global_step, int(tr._adam_step_dev.item()))
  snap = tr._snapshot()
  tr.run(s, t)
  moved = _differing(before, _everything(tr))
  assert {'flat/g', 'slot0/g', 'slot1/g', 'avg/g'} <= set(moved), moved
  tr._restore(snap)
  bad = _differing(before, _everything(tr))
  assert not bad, bad
  assert (tr.adam_t, tr.n_critic_counter, tr.global_step, int(tr._adam_step_dev.item())) == counters == (2, 2, 1, 2)
  tr.close()


@pytest.mark.parametrize('rule', R.RULES)
def test_trainer_optimizer_graph_replay(rule):
  """The same four runs eager and replayed from captured graphs (deterministic mode): parameters, slots and averages agree bit
  for bit after every run -- the hyper-parameters are by value, the average's weight is a device pointer."""
  from twingan_amd.twingan import Trainer
  s, t = _batch()
  with _Deterministic():
    trs = [Trainer(_cfg(optimizer=rule, moving_average_decay=0.999), device=DEV, seed=3, use_graph=graph) for graph in (False, True)]
    for i in range(4):
      for tr in trs:
        tr.run(s, t)
      assert trs[1].use_graph and trs[1].graph_fallback_reason is None, trs[1].graph_fallback_reason
      bad = _differing(_everything(trs[0]), _everything(trs[1]))
      assert not bad, ('run %d' % i, bad)
    assert trs[0].adam_t == trs[1].adam_t == 4 and int(trs[1]._adam_step_dev.item()) == 4
  for tr in trs:
    tr.close()


def _ema_weight(decay, n):
  n = np.float32(n)
  d = min(np.float32(decay), (np.float32(1) + n) / (np.float32(10) + n))
  return np.float32(1) - np.float32(d)


@pytest.mark.parametrize('rule', R.RULES)
def test_trainer_averages_follow_float64(rule):
  """moving_average_decay = 0.999, four eager runs: every group's flat average follows the float64 recurrence over the
  trainer's own post-run parameters, with the float32 weight of the global step on entering the run (the approach of
  test_trainer_averages_match_float64); the applied parameters still match the rule."""
  from twingan_amd.twingan import Trainer
  decay = 0.999
  tr = Trainer(_cfg(optimizer=rule, moving_average_decay=decay), device=DEV, seed=3)
  st = tr.store
  s, t = _batch()
  h = _trainer_hyper(tr.cfg)
  avg = {g: st.avg[g].double().cpu().numpy() for g in st.GROUPS}
  assert all(np.array_equal(avg[g], st.flat[g].detach().double().cpu().numpy()) for g in st.GROUPS)
  bound = {g: np.zeros_like(avg[g]) for g in st.GROUPS}
  for i in range(4):
    group = 'gd'[i % 2]
    before = _owned(tr, group)
    w = _ema_weight(decay, tr.global_step)
    tr.run(s, t)
    refs, bounds = R.step(rule, before[0].double().cpu().numpy(), st.grad[group].double().cpu().numpy(),
                          [x.double().cpu().numpy() for x in before[1:]], h, 1.0)
    E.assert_elementwise(st.flat[group].detach().double().cpu().numpy(), refs[0], bounds[0], '%s run %d theta' % (rule, i))
    for g in st.GROUPS:
      avg[g], b = R.ema(avg[g], st.flat[g].detach().double().cpu().numpy(), w)
      bound[g] = bound[g] + b
      E.assert_elementwise(st.avg[g].double().cpu().numpy(), avg[g], bound[g], '%s run %d: average of group %s' % (rule, i, g))
  assert not torch.equal(st.avg['g'], st.flat['g'].detach())
  tr.close()


@pytest.mark.parametrize('rule', R.RULES)
def test_trainer_first_apply_is_skipped_under_dynamic_loss_scale(rule):
  """fp16 with dynamic_loss_scale from 2^24: the scaled backward overflows on this model, so the first apply of each group is
  skipped -- theta and the slots untouched bit for bit, the group's scale halved, the host counters advanced."""
  from twingan_amd.twingan import Trainer
  tr = Trainer(_cfg(optimizer=rule, precision='fp16', dynamic_loss_scale=True, loss_scale=2.0 ** 24, loss_scale_growth_interval=1000),
               device=DEV, seed=3)
  s, t = _batch(torch.float16)
  for i, group in enumerate('gd'):
    before = _owned(tr, group)
    tr.run(s, t)
    assert not bool(torch.isfinite(tr.store.grad[group]).all())
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(before, _owned(tr, group))), 'the skipped apply of %s wrote' % group
  state = tr.loss_scale_state()
  assert state['applies'] == 0 and all(state[g]['skipped'] == 1 and state[g]['scale'] == 2.0 ** 23 for g in 'gd'), state
  assert (tr.adam_t, tr.n_critic_counter, tr.global_step) == (2, 2, 1)
  tr.close()


def _work_tags(cfg, dtype=torch.float32):
  from twingan_amd import _lib
  from twingan_amd.twingan import Trainer
  tr = Trainer(cfg, device=DEV, seed=3)
  s, t = _batch(dtype)
  _lib.profiler = []
  try:
    tr.run(s, t)
    tr.run(s, t)
    rows = [(r[0], r[1], r[3]) for r in _lib.profiler]
  finally:
    _lib.profiler = None
  n = {g: tr.store.flat[g].numel() for g in 'gd'}
  tr.close()
  return rows, n


_APPLY_CALLS = ('tg_adam_step', 'tg_adam_ema', 'tg_optim')


def test_adam_work_rows_are_unchanged():
  """optimizer='adam' keeps its work= rows (adam:numel%d, 28 bytes per element; adam_ema: 36) and never calls tg_optim_step."""
  for kw, name, tag, b in (({}, 'tg_adam_step', 'adam', 28), (dict(moving_average_decay=0.5), 'tg_adam_ema_step', 'adam_ema', 36)):
    rows, n = _work_tags(_cfg(optimizer='adam', **kw))
    applies = [r for r in rows if r[0].startswith(_APPLY_CALLS)]
    assert applies == [(name, '%s:numel%d' % (tag, n[g]), b * n[g]) for g in 'gd'], applies


@pytest.mark.parametrize('rule,per', [('sgd', 12), ('momentum', 20), ('adagrad', 20), ('rmsprop', 28), ('adadelta', 28), ('ftrl', 28)])
def test_optim_work_rows(rule, per):
  """The other rules' rows are optim_<rule>[_ema][_guarded]:numel%d with the rule's bytes per element, 8 more with the average
  (every form for rmsprop, the plain and the fullest for the rest)."""
  forms = [({}, '', 0), (dict(moving_average_decay=0.5, dynamic_loss_scale=True), '_ema_guarded', 8)]
  if rule == 'rmsprop':
    forms += [(dict(moving_average_decay=0.5), '_ema', 8), (dict(dynamic_loss_scale=True), '_guarded', 0)]
  for kw, sfx, extra in forms:
    rows, n = _work_tags(_cfg(optimizer=rule, **kw))
    applies = [r for r in rows if r[0].startswith(_APPLY_CALLS)]
    assert applies == [('tg_optim_step', 'optim_%s%s:numel%d' % (rule, sfx, n[g]), (per + extra) * n[g]) for g in 'gd'], applies


# ------------------------------------------------------------------------------------------------ checkpoints
@pytest.mark.parametrize('rule', ['rmsprop', 'momentum'])
def test_checkpoint_round_trip(rule, tmp_path):
  """Saved after two applies and restored into a fresh trainer of another seed: theta, the slots and the counters are
  bit-equal; the file holds the variables, the rule's slots under TF's names and the bookkeeping keys -- no /Adam*, no
  beta power.  Restoring it into an Adam trainer names both optimisers; init_from_checkpoint loads every model variable."""
  from twingan_amd import checkpoint as ckpt
  from twingan_amd.twingan import Trainer
  tr = Trainer(_cfg(optimizer=rule), device=DEV, seed=3)
  s, t = _batch()
  tr.run(s, t)
  tr.run(s, t)
  prefix = ckpt.save(tr, str(tmp_path / rule))
  arrays = ckpt.read_checkpoint(prefix)
  st = tr.store
  want = set(st.specs) | set(st.state_specs) | {k + '/' + slot for k in st.specs for slot in R.SLOT_NAMES[rule]} | \
      {'global_step', 'n_critic_counter', ckpt.RNG_DRAWS_KEY}
  assert set(arrays) == want, sorted(set(arrays) ^ want)[:6]
  assert not any('/Adam' in k or k.endswith('_power') for k in arrays)
  fresh = Trainer(_cfg(optimizer=rule), device=DEV, seed=11)
  assert _differing(_variables(tr), _variables(fresh))
  assert ckpt.restore(fresh, prefix) == tr.global_step == 1
  assert not _differing(_variables(tr), _variables(fresh))
  assert any(k.endswith('/' + R.SLOT_NAMES[rule][0]) for k in _variables(tr))
  assert (fresh.adam_t, fresh.n_critic_counter, fresh.global_step) == (tr.adam_t, tr.n_critic_counter, tr.global_step) == (2, 2, 1)
  assert int(fresh._adam_step_dev.item()) == 2
  adam = Trainer(_cfg(), device=DEV, seed=5)
  with pytest.raises(ValueError) as e:
    ckpt.restore(adam, prefix)
  assert rule in str(e.value) and 'adam' in str(e.value)
  loaded = ckpt.init_from_checkpoint(adam, prefix)
  assert set(loaded) == {k for k in list(st.specs) + list(st.state_specs) if not k.endswith('/sa_gamma')}
  assert not _differing({'flat/' + g: st.flat[g].detach() for g in 'gd'}, {'flat/' + g: adam.store.flat[g].detach() for g in 'gd'})
  # and the other way round: an Adam file does not resume a trainer of this rule
  adam_prefix = ckpt.save(adam, str(tmp_path / 'adam'))
  with pytest.raises(ValueError) as e:
    ckpt.restore(fresh, adam_prefix)
  assert rule in str(e.value) and 'adam' in str(e.value)
  for x in (tr, fresh, adam):
    x.close()
