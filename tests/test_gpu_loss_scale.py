"""Dynamic loss scaling decided on the device (Config.dynamic_loss_scale): the non-finite check element by
element, the tick's schedule against a plain restatement and torch._amp_update_scale_, the guarded applies bit for bit
against the static ones, a skipped apply, the trainer in fp16 from a scale that overflows by itself -- eager and replayed
from hipGraphs --, and the checkpoint round trip.

Every comparison here is of bits, except the first applied Adam step of the trainer, which is held to
elementwise.adam_step_bounds from the trainer's own gradient and state."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import elementwise as E      # noqa: E402

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
PAD = 64                        # canary elements on either side of a view (keeps the view's base 256-byte aligned)
CANARY = 7.0
INF = float('inf')
MAX_SCALE = 2.0 ** 24
# tg_nonfinite_check's grid (include/twingan_hip.h): at most 2048 workgroups of 256 threads; 8 elements per thread and trip
# through 16-byte loads, 1 element by element
SWEEP_VEC, SWEEP_SCALAR = 2048 * 256 * 8, 2048 * 256
CHECK_SIZES = [(1, 0), (255, 0), (257, 0), (4099, 0), (257, 1), (257, 3), (4099, 3), (SWEEP_VEC + 4099, 0), (SWEEP_SCALAR + 4099, 1)]
APPLY_SIZES = [(1, 0), (255, 0), (257, 0), (4099, 0), (257, 1), (4099, 3), (4096 * 256 + 4099, 0)]
_SIZE_ID = lambda p: '%d+%d' % p
FLAGGED = {'+inf': 0x7f800000, '-inf': 0xff800000, 'qnan': 0x7fc00000, '-qnan1': 0xffc00001, 'snan': 0x7f800001}
B1, B2, EPS, LR = 0.5, 0.99, 1e-8, 1e-4


def _stream():
  return torch.cuda.current_stream().cuda_stream


def _i32(bits):
  return bits - (1 << 32) if bits >= (1 << 31) else bits


def _view(numel, off, fill=None, canary=CANARY):
  """-> (buffer with canaries, view of numel elements starting PAD + off elements in)."""
  buf = torch.full((numel + 2 * PAD + 4,), canary, dtype=torch.float32, device=DEV)
  v = buf[PAD + off:PAD + off + numel]
  if fill is not None:
    v.copy_(fill)
  return buf, v


def _canaries_ok(buf, numel, off, canary=CANARY):
  return bool((buf[:PAD + off] == canary).all()) and bool((buf[PAD + off + numel:] == canary).all())


def _bits(t):
  return t.view(torch.int32)


def _new_state(scale, world=1, found=0, good=0, skipped=0):
  """A TgLossScaleState on the device between canary words -> (int32 buffer, int32[8] view of the state)."""
  from twingan_amd._lib import TgLossScaleState
  st = TgLossScaleState(scale=scale, seed=scale / world, inv_scale=1.0 / scale, found=found, skip=0, good_steps=good, skipped=skipped)
  buf = torch.full((24,), 0x5a5a5a5a, dtype=torch.int32, device=DEV)
  buf[8:16].copy_(torch.frombuffer(bytearray(bytes(st)), dtype=torch.int32))
  return buf, buf[8:16]


def _read_state(view):
  from twingan_amd._lib import TgLossScaleState
  return TgLossScaleState.from_buffer_copy(view.cpu().numpy().tobytes())


FOUND = 3      # index of `found` among the state's eight 32-bit words


# ------------------------------------------------------------------------------------------------ 1. the check kernel
def _clean(numel, gen):
  """Finite values only: +-FLT_MAX, +-0, the smallest subnormals and normal numbers, by element index."""
  x = torch.randn(numel, generator=gen)
  kind = torch.arange(numel) % 8
  fmax = float(np.finfo(np.float32).max)
  for k, val in ((1, fmax), (2, -fmax), (3, 0.0), (4, -0.0)):
    x[kind == k] = val
  xb = x.view(torch.int32)
  xb[kind == 5] = 1                    # 2^-149
  xb[kind == 6] = _i32(0x80000001)     # -2^-149
  return x


@pytest.mark.parametrize('size', CHECK_SIZES, ids=_SIZE_ID)
def test_nonfinite_check_elementwise(size):
  """One special value at a time at the first and last element, the last element of the 16-byte body, the first of the tail
  behind it, the middle, and an element of the second grid sweep: +-inf and NaNs of both signs, quiet and signalling, raise
  `found`; a buffer of +-FLT_MAX, +-0, subnormals and normal numbers does not -- between +inf canaries, so a read of one
  element outside the range would.  The launch ORs: a flag at 1 stays 1 over a clean range.  Nothing but the flag word of the
  state is written, and the input keeps its bits."""
  from twingan_amd._lib import call
  numel, off = size
  gen = torch.Generator().manual_seed(numel + 31 * off)
  buf, x = _view(numel, off, _clean(numel, gen), canary=INF)
  before = _bits(buf).clone()
  sbuf, state = _new_state(128.0, good=2, skipped=5)
  sbefore = sbuf.clone()

  def check():
    call('tg_nonfinite_check', x.data_ptr(), numel, state.data_ptr(), _stream())
    rest = torch.ones(24, dtype=torch.bool, device=DEV)
    rest[8 + FOUND] = False
    assert torch.equal(sbuf[rest], sbefore[rest]), 'the launch wrote more of the state than `found`'
    return int(state[FOUND].item())

  assert check() == 0, 'a clean buffer raised the flag (a finite value taken for inf / NaN, or a read outside the range)'
  state[FOUND] = 1
  assert check() == 1, 'a clean range cleared a flag that was already up'
  body = numel // 4 * 4
  sweep = SWEEP_VEC if off % 4 == 0 else SWEEP_SCALAR
  spots = {0, numel - 1, numel // 2, max(body - 1, 0), min(body, numel - 1)}
  if numel > sweep + 5:
    spots |= {sweep + 5, sweep // 2 + 3}      # the second sweep; the second 16-byte load of the first trip
  xb = _bits(x)
  for pos in sorted(spots):
    keep = int(xb[pos].item())
    for name, pattern in FLAGGED.items():
      xb[pos] = _i32(pattern)
      state[FOUND] = 0
      assert check() == 1, '%s at element %d of %d + %d was not seen' % (name, pos, numel, off)
    xb[pos] = keep
  state[FOUND] = 0
  assert check() == 0
  assert torch.equal(_bits(buf), before), 'the launch wrote its input'


def test_loss_scale_errors_are_loud():
  """Null pointers, numel <= 0, an interval / cap / world below 1 raise TgError and launch nothing."""
  from twingan_amd import _lib
  from twingan_amd._lib import TgError, call
  assert _lib.load().tg_loss_scale_state_bytes() == 32
  n = 64
  b = {k: torch.full((n,), 3.0, dtype=torch.float32, device=DEV) for k in ('th', 'g', 'm', 'v', 'avg')}
  lr, w = torch.full((1,), 1e-4, device=DEV), torch.full((1,), 0.5, device=DEV)
  step = torch.zeros(1, dtype=torch.int64, device=DEV)
  sbuf, state = _new_state(4.0, found=1)
  sbefore = sbuf.clone()
  st, sp = _stream(), state.data_ptr()
  for bad in ((None, n, sp, st), (b['g'].data_ptr(), n, None, st), (b['g'].data_ptr(), 0, sp, st), (b['g'].data_ptr(), -3, sp, st)):
    with pytest.raises(TgError):
      call('tg_nonfinite_check', *bad)
  tick = [sp, step.data_ptr(), lr.data_ptr(), LR, B1, B2, 3, MAX_SCALE, 1, st]
  for i, val in ((0, None), (1, None), (2, None), (6, 0), (7, 0.5), (8, 0)):
    with pytest.raises(TgError):
      call('tg_loss_scale_tick', *(tick[:i] + [val] + tick[i + 1:]))
  adam = [b['th'].data_ptr(), b['g'].data_ptr(), b['m'].data_ptr(), b['v'].data_ptr(), n, lr.data_ptr(), B1, B2, EPS, sp, st]
  for i, val in ((0, None), (1, None), (2, None), (3, None), (4, 0), (5, None), (9, None)):
    with pytest.raises(TgError):
      call('tg_adam_step_guarded', *(adam[:i] + [val] + adam[i + 1:]))
  fused = adam[:4] + [b['avg'].data_ptr()] + adam[4:10] + [w.data_ptr(), st]
  for i, val in ((0, None), (4, None), (5, 0), (6, None), (10, None), (11, None)):
    with pytest.raises(TgError):
      call('tg_adam_ema_step_guarded', *(fused[:i] + [val] + fused[i + 1:]))
  torch.cuda.synchronize()
  assert torch.equal(sbuf, sbefore) and int(step.item()) == 0
  assert all(bool((t == 3.0).all()) for t in b.values())


# ------------------------------------------------------------------------------------------------ 2. the tick's schedule
INTERVAL = 3
# (initial scale, found flags): growth, a backoff in the middle of a count, two backoffs in a row and the floor at 1; then
# the cap at 2^24 and the way down from it
SCRIPTS = [(4.0, [0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 1, 1, 0, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 1, 0, 0, 0]),
           (2.0 ** 23, [0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0])]


def _tick_model(scale, good, skipped, found):
  if found:
    return max(scale / 2.0, 1.0), 0, skipped + 1
  good += 1
  if good >= INTERVAL:
    return min(2.0 * scale, MAX_SCALE), 0, skipped
  return scale, good, skipped


@pytest.mark.parametrize('world', [1, 2, 3])
def test_tick_schedule(world):
  """41 scripted applies with a growth interval of 3.  After every tick: scale, good-step count and skipped total equal the
  plain restatement above; while no bound has been touched also torch._amp_update_scale_ (growth 2, backoff 0.5, the same
  interval) on CPU tensors; found is cleared, skip says what was found, inv_scale is 1 / the OLD scale and seed the NEW scale /
  world; the shared Adam step and rate are bit-equal to tg_adam_tick's on a twin for every tick that was not skipped and
  untouched by a skipped one."""
  from twingan_amd._lib import call
  st = _stream()
  assert sum(len(s) for _, s in SCRIPTS) == 41
  seen = set()
  for scale0, script in SCRIPTS:
    sbuf, state = _new_state(scale0, world)
    step, lr = torch.zeros(1, dtype=torch.int64, device=DEV), torch.zeros(1, dtype=torch.float32, device=DEV)
    step2, lr2 = step.clone(), lr.clone()
    scale, good, skipped = scale0, 0, 0
    amp_scale, amp_good, clipped = torch.tensor([scale0]), torch.zeros(1, dtype=torch.int32), False
    for i, found in enumerate(script):
      state[FOUND] = found
      prev_step, prev_lr = step.clone(), lr.clone()
      call('tg_loss_scale_tick', state.data_ptr(), step.data_ptr(), lr.data_ptr(), LR, B1, B2, INTERVAL, MAX_SCALE, world, st)
      old = scale
      scale, good, skipped = _tick_model(scale, good, skipped, found)
      got = _read_state(state)
      what = 'tick %d from %g' % (i, scale0)
      assert (got.scale, got.good_steps, got.skipped) == (scale, good, skipped), what
      assert (got.found, got.skip) == (0, found), what
      assert got.inv_scale == 1.0 / old and got.seed == np.float32(scale / world), what
      clipped = clipped or (found and old == 1.0) or (not found and good == 0 and old == MAX_SCALE)
      torch._amp_update_scale_(amp_scale, amp_good, torch.tensor([float(found)]), 2.0, 0.5, INTERVAL)
      if not clipped:
        assert (float(amp_scale), int(amp_good)) == (scale, good), what
      if found:
        assert torch.equal(step, prev_step) and torch.equal(_bits(lr), _bits(prev_lr)), what
      else:
        call('tg_adam_tick', step2.data_ptr(), lr2.data_ptr(), LR, B1, B2, st)
        assert torch.equal(step, step2) and torch.equal(_bits(lr), _bits(lr2)), what
      seen.add(('skip' if found else 'grow' if scale > old else 'keep', old == 1.0, old == MAX_SCALE, good))
    assert bool((sbuf[:8] == 0x5a5a5a5a).all()) and bool((sbuf[16:] == 0x5a5a5a5a).all())
    assert int(step.item()) == len(script) - sum(script)
  # the script met what it was written for: growth, a backoff at count 1 and 2, one straight after another, floor and cap
  assert ('grow', False, False, 0) in seen and ('skip', True, False, 0) in seen and ('keep', False, True, 0) in seen


# ------------------------------------------------------------------------------------------------ 3. + 4. the guarded applies
def _adam_sides(numel, off, th0, avg0, count):
  zero = torch.zeros(numel)
  return [dict(th=_view(numel, off, th0), m=_view(numel, off, zero), v=_view(numel, off, zero), avg=_view(numel, off, avg0),
               step=torch.zeros(1, dtype=torch.int64, device=DEV), lr=torch.zeros(1, dtype=torch.float32, device=DEV))
          for _ in range(count)]


def _p(side, k):
  return side[k][1].data_ptr()


def _guarded(side, state, g, numel, w_dev, fused, interval=1000):
  from twingan_amd._lib import call
  st, sp = _stream(), state.data_ptr()
  call('tg_nonfinite_check', g.data_ptr(), numel, sp, st)
  call('tg_loss_scale_tick', sp, side['step'].data_ptr(), side['lr'].data_ptr(), LR, B1, B2, interval, MAX_SCALE, 1, st)
  if fused:
    call('tg_adam_ema_step_guarded', _p(side, 'th'), g.data_ptr(), _p(side, 'm'), _p(side, 'v'), _p(side, 'avg'), numel,
         side['lr'].data_ptr(), B1, B2, EPS, sp, w_dev.data_ptr(), st)
  else:
    call('tg_adam_step_guarded', _p(side, 'th'), g.data_ptr(), _p(side, 'm'), _p(side, 'v'), numel, side['lr'].data_ptr(), B1, B2,
         EPS, sp, st)


def _static(side, g, numel, w_dev, fused, scale):
  from twingan_amd._lib import call
  st = _stream()
  call('tg_adam_tick', side['step'].data_ptr(), side['lr'].data_ptr(), LR, B1, B2, st)
  if fused:
    call('tg_adam_ema_step', _p(side, 'th'), g.data_ptr(), _p(side, 'm'), _p(side, 'v'), _p(side, 'avg'), numel, side['lr'].data_ptr(),
         B1, B2, EPS, 1.0 / scale, w_dev.data_ptr(), st)
  else:
    call('tg_adam_step', _p(side, 'th'), g.data_ptr(), _p(side, 'm'), _p(side, 'v'), None, numel, 0.0, side['lr'].data_ptr(), B1, B2,
         EPS, 1.0 / scale, st)


def _same(a, b, keys, what):
  for k in keys:      # whole buffers: the canaries with them
    assert torch.equal(_bits(a[k][0]), _bits(b[k][0])), '%s: %s differs' % (what, k)
  assert torch.equal(a['step'], b['step']) and torch.equal(_bits(a['lr']), _bits(b['lr'])), '%s: step / rate differ' % what


def _gradient_mix(numel, gen):
  """test_adam_ema_fused_equals_unfused's: g = 0 throughout, |g| = 1e4, |g| = 1e-20, theta = 0 on every eighth element."""
  ar = torch.arange(numel)
  kind = ar % 4
  mix = torch.where(kind == 1, 1e4, torch.where(kind == 2, 1e-20, torch.where(kind == 3, 0.0, 1.0))).double()
  th0 = torch.randn(numel, generator=gen)
  th0[ar % 8 == 0] = 0.0
  return th0, torch.randn(numel, generator=gen), mix


@pytest.mark.parametrize('scale', [1.0, 128.0, 65536.0])
@pytest.mark.parametrize('size', APPLY_SIZES, ids=_SIZE_ID)
def test_guarded_apply_equals_static(size, scale):
  """Ten steps, gradients multiplied by S: check + tick + guarded apply from a state at S against tg_adam_tick + tg_adam_step
  (grad_scale = 1 / S) on a twin, and the fused forms against each other: theta, m, v (and avg), step and rate bit for bit
  after every step, canaries included.  The last size is past the apply's 4096-workgroup grid."""
  numel, off = size
  gen = torch.Generator().manual_seed(numel % 1000 + off)
  th0, avg0, mix = _gradient_mix(numel, gen)
  dyn, stat, dyn_f, stat_f = _adam_sides(numel, off, th0, avg0, 4)
  states = [_new_state(scale)[1] for _ in range(2)]
  gbuf, g = _view(numel, off)
  w_dev = torch.tensor([0.9], dtype=torch.float32, device=DEV)
  for t in range(1, 11):
    g.copy_((torch.randn(numel, generator=gen).double() * mix * scale).float())
    _guarded(dyn, states[0], g, numel, w_dev, False)
    _static(stat, g, numel, w_dev, False, scale)
    _guarded(dyn_f, states[1], g, numel, w_dev, True)
    _static(stat_f, g, numel, w_dev, True, scale)
    _same(dyn, stat, ('th', 'm', 'v', 'avg'), 'step %d' % t)
    _same(dyn_f, stat_f, ('th', 'm', 'v', 'avg'), 'fused step %d' % t)
  for s in states:
    got = _read_state(s)
    assert (got.scale, got.good_steps, got.skipped, got.skip) == (scale, 10, 0, 0)
  assert int(dyn['step'].item()) == 10 and not torch.equal(dyn['th'][1].cpu(), th0)
  assert torch.equal(dyn['avg'][1].cpu(), avg0) and not torch.equal(dyn_f['avg'][1].cpu(), avg0)
  for side in (dyn, stat, dyn_f, stat_f):
    assert all(_canaries_ok(side[k][0], numel, off) for k in ('th', 'm', 'v', 'avg'))
  assert _canaries_ok(gbuf, numel, off)


@pytest.mark.parametrize('fused', [False, True], ids=['adam', 'adam_ema'])
@pytest.mark.parametrize('size', [(257, 1), (4099, 0)], ids=_SIZE_ID)
def test_skipped_apply(size, fused):
  """Three good steps at S = 128, then one inf in the gradient: theta, m, v, the step counter and the rate keep their bits,
  canaries stay, S halves; the fused form's avg is what tg_ema_update gives from the unchanged theta.  The next apply, with a
  clean gradient, equals the static apply at S / 2."""
  from twingan_amd._lib import call
  numel, off = size
  gen = torch.Generator().manual_seed(numel + off)
  th0, avg0, mix = _gradient_mix(numel, gen)
  dyn, stat = _adam_sides(numel, off, th0, avg0, 2)
  state = _new_state(128.0)[1]
  gbuf, g = _view(numel, off)
  w_dev = torch.tensor([0.9], dtype=torch.float32, device=DEV)
  draw = lambda s: (torch.randn(numel, generator=gen).double() * mix * s).float()
  for _ in range(3):
    g.copy_(draw(128.0))
    _guarded(dyn, state, g, numel, w_dev, fused)
    _static(stat, g, numel, w_dev, fused, 128.0)
  _same(dyn, stat, ('th', 'm', 'v', 'avg'), 'before the overflow')
  g.copy_(draw(128.0))
  g[numel // 2] = INF
  before = {k: _bits(dyn[k][0]).clone() for k in ('th', 'm', 'v', 'avg')}
  step, lr = dyn['step'].clone(), dyn['lr'].clone()
  _guarded(dyn, state, g, numel, w_dev, fused)
  got = _read_state(state)
  assert (got.scale, got.good_steps, got.skipped, got.skip, got.found) == (64.0, 0, 1, 1, 0)
  assert got.inv_scale == 1.0 / 128.0 and got.seed == 64.0
  for k in ('th', 'm', 'v'):
    assert torch.equal(_bits(dyn[k][0]), before[k]), '%s changed in a skipped apply' % k
  assert torch.equal(dyn['step'], step) and torch.equal(_bits(dyn['lr']), _bits(lr))
  if fused:
    call('tg_ema_update', _p(stat, 'avg'), _p(stat, 'th'), numel, w_dev.data_ptr(), _stream())
    assert not torch.equal(_bits(dyn['avg'][0]), before['avg']), 'a skipped fused apply left the averages where they were'
  _same(dyn, stat, ('th', 'm', 'v', 'avg'), 'the skipped apply')
  g.copy_(draw(64.0))
  _guarded(dyn, state, g, numel, w_dev, fused)
  _static(stat, g, numel, w_dev, fused, 64.0)
  _same(dyn, stat, ('th', 'm', 'v', 'avg'), 'the apply after the skipped one')
  assert int(dyn['step'].item()) == 4 and _read_state(state).good_steps == 1
  assert all(_canaries_ok(dyn[k][0], numel, off) for k in ('th', 'm', 'v', 'avg')) and _canaries_ok(gbuf, numel, off)


# ------------------------------------------------------------------------------------------------ 5. - 7. the trainer
class _Deterministic:
  def __enter__(self):
    from twingan_amd import _lib
    self.lib = _lib.load()
    self.was = self.lib.tg_set_deterministic(1)

  def __exit__(self, *exc):
    self.lib.tg_set_deterministic(self.was)


HW, MAX_RUNS = 16, 80


def _cfg(**kw):
  from twingan_amd import Config
  return Config(hw=HW, max_ch=8, precision='fp16', **kw)


def _batch():
  g = torch.Generator().manual_seed(8)
  s, t = torch.rand(2, HW, HW, 3, generator=g), torch.rand(2, HW, HW, 3, generator=g)
  return s.to(DEV).half(), t.to(DEV).half()


def _tensors(tr):
  """Bit copies of everything the optimiser owns, per group, and both loss-scale states."""
  s = tr.store
  out = {'%s/%s' % (k, g): t.clone() for g in s.GROUPS for k, t in zip(('flat', 'm', 'v'), [s.flat[g]] + s.slots[g])}
  out.update({'ls/' + g: t.clone() for g, t in tr._ls.items()})
  out['step'], out['lr'] = tr._adam_step_dev.clone(), tr._lr_t_dev.clone()
  return out


def _differing(a, b):
  """The keys whose tensors differ in some bit."""
  return [k for k in a if not torch.equal(a[k].view(torch.int32), b[k].view(torch.int32))]


def _skipping_trajectory(graph, runs=None, **kw):
  """A dynamic trainer from the initial scale 2^24: the seed of the scaled backward overflows half precision by itself, so
  the first runs of each group skip until its scale has come down -- nothing is injected.  Runs until each group has made
  an apply (or ``runs`` runs) -> (trainer, per-run records: group, tensors before and after, the scaled gradient)."""
  from twingan_amd.twingan import Trainer
  tr = Trainer(_cfg(dynamic_loss_scale=True, loss_scale=MAX_SCALE, loss_scale_growth_interval=1000, **kw), device=DEV, seed=3,
               use_graph=graph)
  s, t = _batch()
  records, made = [], {'g': 0, 'd': 0}
  while len(records) < (runs or MAX_RUNS) and (runs or min(made.values()) < 1):
    group = 'g' if tr.n_critic_counter % tr.cfg.n_critic == 0 else 'd'
    before = _tensors(tr)
    tr.run(s, t)
    after = _tensors(tr)
    skipped = int(_read_state(after['ls/' + group]).skipped) - int(_read_state(before['ls/' + group]).skipped)
    made[group] += 1 - skipped
    records.append(dict(group=group, before=before, after=after, skipped=skipped, grad=tr.store.grad[group].clone()))
  assert not graph or tr.graph_fallback_reason is None, tr.graph_fallback_reason
  return tr, records


@pytest.fixture(scope='module')
def eager():
  with _Deterministic():
    tr, records = _skipping_trajectory(False)
  yield tr, records
  tr.close()


def test_trainer_skips_until_the_scale_fits(eager):
  """Skipped runs keep parameters, moments, the device step and rate bit for bit while the group's scale halves exactly once;
  the other group's state is never touched by a run; the host counters advance regardless.  The first run of each group that
  is not skipped moves the parameters, by the Adam step recomputed in float64 from the trainer's own scaled gradient and the
  state before, with grad_scale = 1 / S, within elementwise.adam_step_bounds."""
  tr, records = eager
  other = {'g': 'd', 'd': 'g'}
  first_apply = {}
  for i, r in enumerate(records):
    g, b, a = r['group'], r['before'], r['after']
    assert g == 'gd'[i % 2]
    sb, sa = _read_state(b['ls/' + g]), _read_state(a['ls/' + g])
    assert torch.equal(b['ls/' + other[g]], a['ls/' + other[g]]), 'run %d (%s) touched the other group\'s loss-scale state' % (i, g)
    assert all(torch.equal(_bits(b['%s/%s' % (k, other[g])]), _bits(a['%s/%s' % (k, other[g])])) for k in ('flat', 'm', 'v'))
    assert (sa.found, sa.skip) == (0, r['skipped']) and sa.inv_scale == 1.0 / sb.scale and sa.seed == sa.scale
    if r['skipped']:
      assert sa.scale == max(sb.scale / 2.0, 1.0) and sa.good_steps == 0, 'run %d' % i
      assert not bool(torch.isfinite(r['grad']).all())
      changed = _differing({k: b[k] for k in ('flat/' + g, 'm/' + g, 'v/' + g, 'step', 'lr')}, a)
      assert not changed, ('skipped run %d changed' % i, changed)
    else:
      assert sa.scale == sb.scale and sa.good_steps == sb.good_steps + 1 and bool(torch.isfinite(r['grad']).all())
      assert int(a['step'].item()) == int(b['step'].item()) + 1
      if g not in first_apply:
        first_apply[g] = i
        prev = [x.double().cpu().numpy() for x in (b['flat/' + g], r['grad'], b['m/' + g], b['v/' + g])]
        c = tr.cfg
        refs, bounds = E.adam_step_bounds(*prev, a['lr'].item(), c.adam_beta1, c.adam_beta2, c.opt_epsilon, 1.0 / sb.scale)
        for j, k in enumerate(('flat', 'm', 'v')):
          E.assert_elementwise(a['%s/%s' % (k, g)].double().cpu().numpy(), refs[j], bounds[j], 'first apply of %s: %s' % (g, k))
        assert not torch.equal(b['flat/' + g], a['flat/' + g]), 'the first applied run of %s moved nothing' % g
  assert set(first_apply) == {'g', 'd'}, 'no apply within %d runs: %s' % (len(records), first_apply)
  state = tr.loss_scale_state()
  skips = {g: sum(r['skipped'] for r in records if r['group'] == g) for g in 'gd'}
  assert all(skips[g] >= 1 and state[g]['skipped'] == skips[g] and state[g]['scale'] == MAX_SCALE / 2 ** skips[g] for g in 'gd'), (state, skips)
  assert state['applies'] == len(records) - sum(skips.values()) >= 2
  assert tr.adam_t == tr.n_critic_counter == len(records) and tr.global_step == len(records) // 2
  print('skipped runs per group %s of %d runs, scales %s' % (skips, len(records), {g: state[g]['scale'] for g in 'gd'}))


def test_trainer_skips_graph_replay(eager):
  """The same trajectory with use_graph=True: parameters, moments, both loss-scale states, step and rate bit-identical to the
  eager one after every run -- the captured apply graphs replay the decision, and the capture's undone warm-up (one real step
  of each kind, both skipped) left the scales, the counts and the skipped totals where they started."""
  _, records = eager
  with _Deterministic():
    tr, replayed = _skipping_trajectory(True, runs=len(records))
  assert tr.use_graph and tr.graph_fallback_reason is None, tr.graph_fallback_reason
  first = _read_state(replayed[0]['before']['ls/g'])
  assert (first.scale, first.good_steps, first.skipped) == (MAX_SCALE, 0, 0)
  for i, (e, r) in enumerate(zip(records, replayed)):
    assert e['skipped'] == r['skipped'], 'run %d' % i
    bad = _differing(e['after'], r['after'])
    assert not bad, ('run %d: hipGraph replay differs from eager launches' % i, bad)
  tr.close()


def test_skipped_runs_still_move_the_averages():
  """moving_average_decay with the dynamic scale: in the first runs (all skipped) the parameters keep their bits and BOTH
  groups' averages equal tg_ema_update applied to a copy -- every run updates every average.  The averages are moved off the
  parameters first (a fresh average equals its variable and would rightly keep its bits)."""
  from twingan_amd._lib import call
  from twingan_amd.twingan import Trainer
  with _Deterministic():
    tr = Trainer(_cfg(dynamic_loss_scale=True, loss_scale=MAX_SCALE, moving_average_decay=0.5), device=DEV, seed=3)
    s, t = _batch()
    for g in 'gd':
      tr.store.avg[g].add_(0.25)
    for i in range(3):
      flat = {g: tr.store.flat[g].clone() for g in 'gd'}
      prev = {g: tr.store.avg[g].clone() for g in 'gd'}
      tr.run(s, t)
      for g in 'gd':
        want = prev[g].clone()
        call('tg_ema_update', want.data_ptr(), flat[g].data_ptr(), want.numel(), tr._ema_w_dev.data_ptr(), _stream())
        assert torch.equal(_bits(tr.store.flat[g]), _bits(flat[g])), 'run %d was not skipped' % i
        assert torch.equal(_bits(tr.store.avg[g]), _bits(want)), 'run %d: the averages of %s' % (i, g)
        assert not torch.equal(tr.store.avg[g], prev[g]), 'run %d left the averages of %s where they were' % (i, g)
    state = tr.loss_scale_state()
  assert state['applies'] == 0 and state['g']['skipped'] == 2 and state['d']['skipped'] == 1
  tr.close()


def _quiet(graph):
  from twingan_amd.twingan import Trainer
  s, t = _batch()
  out = []
  with _Deterministic():
    for kw in (dict(dynamic_loss_scale=True, loss_scale_growth_interval=10 ** 6), {}):
      tr = Trainer(_cfg(loss_scale=128.0, **kw), device=DEV, seed=3, use_graph=graph)
      for _ in range(4):
        tr.run(s, t)
      assert not graph or tr.graph_fallback_reason is None, tr.graph_fallback_reason
      sd = {k: v.clone() for k, v in tr.store.state_dict(include_state=True).items()}
      sd.update({'%s/%s' % (k, g): t.clone() for g in 'gd' for k, t in zip(('m', 'v'), tr.store.slots[g])})
      out.append((sd, tr.loss_scale_state() if kw else None))
      tr.close()
  (dyn, state), (stat, _) = out
  assert state['applies'] == 4 and all(state[g] == dict(scale=128.0, good_steps=2, skipped=0) for g in 'gd'), state
  assert all(bool(torch.isfinite(v).all()) for v in stat.values())
  bad = [k for k in stat if not torch.equal(_bits(dyn[k]), _bits(stat[k]))]
  assert not bad, ('the dynamic trainer at a quiet scale 128 differs from the static one', bad[:5])


def test_quiet_dynamic_scale_equals_static():
  """dynamic_loss_scale with initial scale 128 and an interval longer than the test: the parameter (and moment) bits of the
  static loss_scale=128 trainer after four runs, in deterministic mode."""
  _quiet(False)


def test_quiet_dynamic_scale_equals_static_and_graph():
  """The same with both trainers replaying hipGraphs."""
  _quiet(True)


NEW_CALLS = {'tg_nonfinite_check', 'tg_loss_scale_tick', 'tg_adam_step_guarded', 'tg_adam_ema_step_guarded', 'tg_loss_scale_state_bytes'}


def test_flag_off_makes_none_of_the_new_calls(monkeypatch):
  """One G run and one D run with twingan_amd._lib.call wrapped: the static trainer makes none of the new C-ABI calls, and the
  dynamic one makes the static one's calls in the static one's order, with tg_adam_tick replaced by check + tick and
  tg_adam_step by its guarded form (the loss's multiply by the scale, a torch op, is gone: the seed carries it)."""
  from twingan_amd import _lib
  from twingan_amd.twingan import Trainer
  names = []
  real = _lib.call

  def spy(name, *args, **kw):
    names.append(name)
    return real(name, *args, **kw)
  for mod in list(sys.modules.values()):
    if getattr(mod, '__name__', '').startswith('twingan_amd') and getattr(mod, 'call', None) is real:
      monkeypatch.setattr(mod, 'call', spy)
  s, t = _batch()
  seen = {}
  for kind, kw in (('static', {}), ('dynamic', dict(dynamic_loss_scale=True))):
    tr = Trainer(_cfg(loss_scale=128.0, **kw), device=DEV, seed=3)
    del names[:]
    tr.run(s, t)
    tr.run(s, t)
    seen[kind] = list(names)
    tr.close()
  assert 'tg_adam_tick' in seen['static'] and 'tg_adam_step' in seen['static']
  assert not NEW_CALLS & set(seen['static']), NEW_CALLS & set(seen['static'])
  swapped = []
  for n in seen['static']:
    swapped += ['tg_nonfinite_check', 'tg_loss_scale_tick'] if n == 'tg_adam_tick' else ['tg_adam_step_guarded'] if n == 'tg_adam_step' else [n]
  assert seen['dynamic'] == swapped, [(i, a, b) for i, (a, b) in enumerate(zip(seen['dynamic'], swapped)) if a != b][:5]


def test_checkpoint_round_trip(eager, tmp_path):
  """Saved after the trajectory with skips and restored into a fresh trainer of another seed: both continue bit-identically
  for four runs (deterministic mode), loss-scale states included.  The saved beta powers and the apply count are the
  device's, not the attempted applies.  A checkpoint written without the flag has today's key set and restores into a dynamic
  trainer at the initial scale with zero counts; init_from_checkpoint leaves the state alone."""
  from twingan_amd import checkpoint as ckpt
  from twingan_amd.twingan import Trainer
  tr, records = eager
  s, t = _batch()
  cfg = tr.cfg
  with _Deterministic():
    prefix = ckpt.save(tr, str(tmp_path / 'dyn'))
    arrays = ckpt.read_checkpoint(prefix)
    state = tr.loss_scale_state()
    applies = state['applies']
    assert 2 <= applies < tr.adam_t == int(arrays['n_critic_counter']) == len(records)
    assert int(arrays[ckpt.ADAM_APPLIES_KEY]) == applies
    assert arrays['beta1_power'] == np.float32(cfg.adam_beta1 ** (applies + 1)) and arrays['beta2_power'] == np.float32(cfg.adam_beta2 ** (applies + 1))
    for g in 'gd':
      key = ckpt.LOSS_SCALE_PREFIX + g
      assert (float(arrays[key + '/scale']), int(arrays[key + '/good_steps']), int(arrays[key + '/skipped'])) == \
          (state[g]['scale'], state[g]['good_steps'], state[g]['skipped'])
    fresh = Trainer(cfg, device=DEV, seed=11)
    assert ckpt.restore(fresh, prefix) == tr.global_step
    assert fresh.loss_scale_state() == state and (fresh.adam_t, fresh.n_critic_counter) == (tr.adam_t, tr.n_critic_counter)
    for i in range(4):
      tr.run(s, t)
      fresh.run(s, t)
      bad = _differing(_tensors(tr), _tensors(fresh))
      assert not bad, ('run %d after the restore' % i, bad)
    # a static trainer's checkpoint: today's keys; a dynamic trainer takes it at its initial scale
    plain = Trainer(_cfg(loss_scale=128.0), device=DEV, seed=3)
    plain.run(s, t)
    plain_prefix = ckpt.save(plain, str(tmp_path / 'plain'))
    today = set(plain.store.specs) | set(plain.store.state_specs) | {k + sfx for k in plain.store.specs for sfx in ('/Adam', '/Adam_1')} | \
        {'beta1_power', 'beta2_power', 'global_step', 'n_critic_counter', ckpt.RNG_DRAWS_KEY}
    assert set(ckpt.read_checkpoint(plain_prefix)) == today
    assert set(arrays) == today | {ckpt.ADAM_APPLIES_KEY} | {ckpt.LOSS_SCALE_PREFIX + g + sfx for g in 'gd' for sfx in ('/scale', '/good_steps', '/skipped')}
    ckpt.restore(fresh, plain_prefix)
    initial = dict(scale=MAX_SCALE, good_steps=0, skipped=0)
    assert fresh.loss_scale_state() == dict(g=initial, d=initial, applies=1)
    ckpt.restore(fresh, prefix)
    ckpt.init_from_checkpoint(fresh, plain_prefix)
    assert fresh.loss_scale_state() == state
    # a static trainer reading the dynamic checkpoint takes the applies made, not the attempted ones
    ckpt.restore(plain, prefix)
    assert int(plain._adam_step_dev.item()) == applies
  fresh.close()
  plain.close()


# ------------------------------------------------------------------------------------------------ 8. an overflow planted mid-network
MID_CONV = 'discriminator_s/encoder_block_8x8x8/Conv/weights'      # the third of the discriminator's six 3x3 convs
QUIET = 128.0                                                      # every unplanted run applies at this scale (asserted)


def _run_and_read(tr, s, t):
  """One run -> (group, its loss, tensors before, tensors after, skipped by this run)."""
  group = 'g' if tr.n_critic_counter % tr.cfg.n_critic == 0 else 'd'
  before = _tensors(tr)
  loss, _ = tr.run(s, t)
  torch.cuda.synchronize()
  after = _tensors(tr)
  return group, loss.detach().float().cpu(), before, after, \
      int(_read_state(after['ls/' + group]).skipped) - int(_read_state(before['ls/' + group]).skipped)


def _assert_applied(run, what):
  group, loss, b, a, skipped = run
  sb, sa = _read_state(b['ls/' + group]), _read_state(a['ls/' + group])
  assert skipped == 0 and sa.scale == sb.scale and sa.found == 0 and bool(torch.isfinite(loss).all()), (what, skipped, sa.scale, loss)
  assert int(a['step'].item()) == int(b['step'].item()) + 1 and not torch.equal(b['flat/' + group], a['flat/' + group]), what


def _assert_skipped(run, what):
  """skipped + 1, the scale halved (not below 1), found back at 0; parameters, moments, the device step and the rate keep
  their bits; the other group is untouched."""
  group, _, b, a, skipped = run
  other = {'g': 'd', 'd': 'g'}[group]
  sb, sa = _read_state(b['ls/' + group]), _read_state(a['ls/' + group])
  assert skipped == 1 and sa.scale == max(sb.scale / 2.0, 1.0) and (sa.found, sa.skip, sa.good_steps) == (0, 1, 0), \
      (what, skipped, sb.scale, sa.scale, sa.found, sa.skip)
  changed = _differing({k: b[k] for k in ('flat/' + group, 'm/' + group, 'v/' + group, 'step', 'lr')}, a)
  assert not changed, (what + ': a skipped run changed', changed)
  touched = _differing({k: b[k] for k in ('flat/' + other, 'm/' + other, 'v/' + other, 'ls/' + other)}, a)
  assert not touched, (what + ': the other group was touched', touched)


@pytest.mark.parametrize('loss', ['hinge', 'wgan_gp'])
@pytest.mark.parametrize('graph', [False, True], ids=['eager', 'graph_replay'])
def test_mid_network_overflow_is_skipped(graph, loss):
  """One element of the fp32 master kernel of a conv in the middle of discriminator_s is +inf during ONE discriminator run
  (packs refreshed as the trainer refreshes them): every activation behind that conv is non-finite, the prediction with
  them, and the run must be skipped on the evidence of the flat gradient alone -- and must REPORT a non-finite loss (the hinge
  term relu(1 +- NaN) is NaN, np.maximum's rule; an fmaxf gives 0 and a finite loss over a broken network).  The runs before
  it apply (the precondition: nothing but the plant overflows at this scale), the other group is untouched, and with the
  element restored the next discriminator run applies.  The graph variant replays the decision from the captured graphs."""
  from twingan_amd.ops import PackCache
  from twingan_amd.twingan import Trainer
  with _Deterministic():
    tr = Trainer(_cfg(dynamic_loss_scale=True, loss_scale=QUIET, loss_scale_growth_interval=10 ** 6, loss_architecture=loss),
                 device=DEV, seed=3, use_graph=graph)
    s, t = _batch()
    for i in range(3):      # g, d, g: an unplanted run of each group applies
      _assert_applied(_run_and_read(tr, s, t), 'unplanted run %d' % i)
    w = tr.P[MID_CONV]
    assert w.dim() == 4 and w.dtype == torch.float32 and w.data_ptr() >= tr.store.flat['d'].data_ptr()
    elem = w.detach().view(-1)[w.numel() // 2:w.numel() // 2 + 1]      # a view into the group's flat buffer
    keep = elem.clone()
    elem.fill_(INF)
    PackCache.refresh(tr._group_weights['d'])
    run = _run_and_read(tr, s, t)
    assert run[0] == 'd'
    _assert_skipped(run, 'the planted run')
    assert not bool(torch.isfinite(run[1]).all()), 'the discriminator loss over a non-finite network reads %r' % (run[1],)
    elem.copy_(keep)
    PackCache.refresh(tr._group_weights['d'])
    _assert_applied(_run_and_read(tr, s, t), 'the generator run after the plant')
    run = _run_and_read(tr, s, t)
    assert run[0] == 'd'
    _assert_applied(run, 'the discriminator run after the restore')
    assert not graph or (tr.use_graph and tr.graph_fallback_reason is None), tr.graph_fallback_reason
    state = tr.loss_scale_state()
    assert state['d'] == dict(scale=QUIET / 2, good_steps=1, skipped=1) and state['g']['skipped'] == 0, state
  tr.close()


def test_nonfinite_input_pixel_skips_both_groups():
  """One NaN pixel in the source batch: the generator run and the discriminator run both skip; on the clean batch both then
  apply, and parameters, moments, step and rate are bit-equal to those of a trainer that never saw the bad batch.  That
  trainer starts at the scale the first one arrives at (QUIET / 2): a power-of-two scale is exact only above fp16's subnormal
  range, so two scales are not bit-neutral; what differs between the two is then the `skipped` counters alone.  Hinge loss:
  no random draw (gradient-penalty alphas) separates the trajectories."""
  from twingan_amd.twingan import Trainer
  kw = dict(dynamic_loss_scale=True, loss_scale_growth_interval=10 ** 6, loss_architecture='hinge')
  with _Deterministic():
    tr = Trainer(_cfg(loss_scale=QUIET, **kw), device=DEV, seed=3)
    s, t = _batch()
    bad = s.clone()
    bad[1, HW // 2, HW // 2, 1] = float('nan')
    for want in 'gd':
      run = _run_and_read(tr, bad, t)
      assert run[0] == want
      _assert_skipped(run, 'the %s run on the NaN pixel' % want)
    for want in 'gd':
      run = _run_and_read(tr, s, t)
      assert run[0] == want
      _assert_applied(run, 'the %s run on the clean batch' % want)
    ref = Trainer(_cfg(loss_scale=QUIET / 2, **kw), device=DEV, seed=3)
    for _ in 'gd':
      ref.run(s, t)
    a, b = _tensors(tr), _tensors(ref)
    differ = _differing({k: v for k, v in a.items() if not k.startswith('ls/')}, b)
    assert not differ, ('the trainer that skipped a bad batch differs from one that never saw it', differ)
    sa, sb = tr.loss_scale_state(), ref.loss_scale_state()
    assert all(sa[g] == dict(sb[g], skipped=1) and sb[g]['skipped'] == 0 for g in 'gd') and sa['applies'] == sb['applies'] == 2, (sa, sb)
  tr.close()
  ref.close()
