"""float64 one-step references of the --optimizer rules (include/twingan_hip_optim.h, csrc/reduce.hip apply_kernel) and the
error bounds of one fp32 launch.  TEST INFRASTRUCTURE.

The rules restate TF 1.8's dense kernels (core/kernels/training_ops.cc).  sgd, momentum and adadelta coincide with
torch.optim's definitions and are held to them in tests/test_optimizers_cpu.py.  For rmsprop (TF puts epsilon inside the
root), adagrad (TF 1.8 has no epsilon) and ftrl the restatement is the only reference -- parity unpinned: no TensorFlow
here -- and a hand-computed scalar step of rmsprop and of ftrl stands in the same file.

Bounds are derived, not measured: ``step`` computes one step in float64 from the fp32 state the launch READ and carries, next
to every intermediate value, a bound of its fp32 error.  Each fp32 operation adds 2^-24 of its result (an fmaf is one
operation); sqrtf and the division are not required to be correctly rounded: two units; powf (ftrl with lr_power != -0.5):
16 units, OpenCL's limit for pow; every operation may flush a subnormal result: + 2^-126.  Errors of the operands propagate to
first order with the operands' magnitudes taken at their far ends (|b| - e_b under a division).  Scalars arrive as the float32
values the kernel is given; 1 - rho is the fp32 difference the kernel computes."""
from collections import namedtuple

import numpy as np

U32 = 2.0 ** -24
TINY = 2.0 ** -126

RULES = ('sgd', 'momentum', 'adagrad', 'rmsprop', 'adadelta', 'ftrl')
RULE_ID = {r: i for i, r in enumerate(RULES)}      # TG_OPT_*
SLOT_NAMES = {'sgd': (), 'momentum': ('Momentum',), 'adagrad': ('Adagrad',), 'rmsprop': ('RMSProp', 'RMSProp_1'),
              'adadelta': ('Adadelta', 'Adadelta_1'), 'ftrl': ('Ftrl', 'Ftrl_1')}
# the struct's fields, in its order
Hyper = namedtuple('Hyper', 'lr momentum decay_or_rho eps lr_power l1 l2')


def default_hyper(rule, lr=1e-4, eps=1e-8):
  """The reference's flag defaults (model/model_inheritor.py:122-165) for ``rule``."""
  return Hyper(lr=lr, momentum=0.9, decay_or_rho=0.95 if rule == 'adadelta' else 0.9, eps=eps, lr_power=-0.5, l1=0.0, l2=0.0)


def slot_init(rule, numel, adagrad_init=0.1, ftrl_init=0.1):
  """Initial slot arrays (float32) in slot0, slot1 order: RMSProp's mean square starts at one, the accumulators at 0.1."""
  init = {'sgd': (), 'momentum': (0.0,), 'adagrad': (adagrad_init,), 'rmsprop': (1.0, 0.0), 'adadelta': (0.0, 0.0),
          'ftrl': (ftrl_init, 0.0)}[rule]
  return [np.full(numel, v, dtype=np.float32) for v in init]


class V:
  """A float64 array and the bound of its fp32 counterpart's error."""

  def __init__(self, val, err=0.0):
    self.val = np.asarray(val, dtype=np.float64)
    self.err = np.zeros_like(self.val) + err

  def mag(self):
    return np.abs(self.val) + self.err


def _v(x):
  return x if isinstance(x, V) else V(x)


def _rnd(val, err, units=1.0):
  return V(val, err + units * U32 * (np.abs(val) + err) + TINY)


def mul(a, b, units=1.0):
  a, b = _v(a), _v(b)
  return _rnd(a.val * b.val, np.abs(a.val) * b.err + np.abs(b.val) * a.err + a.err * b.err, units)


def add(a, b):
  a, b = _v(a), _v(b)
  return _rnd(a.val + b.val, a.err + b.err)


def sub(a, b):
  a, b = _v(a), _v(b)
  return _rnd(a.val - b.val, a.err + b.err)


def fma(a, b, c):
  """a b + c with ONE rounding."""
  a, b, c = _v(a), _v(b), _v(c)
  return _rnd(a.val * b.val + c.val, np.abs(a.val) * b.err + np.abs(b.val) * a.err + a.err * b.err + c.err)


def div(a, b):
  a, b = _v(a), _v(b)
  low = np.abs(b.val) - b.err
  assert bool((low > 0).all()), 'a denominator may reach zero inside its bound'
  q = a.val / b.val
  return _rnd(q, (a.err + np.abs(q) * b.err) / low, 2.0)


def sqrt(a):
  a = _v(a)
  assert bool((a.val >= 0).all())
  r = np.sqrt(a.val)
  return _rnd(r, np.minimum(a.err / (r + 1e-300), np.sqrt(a.err)), 2.0)


def power(a, q):
  """a^q for a > 0 and an exact scalar q >= 0: powf, 16 units."""
  a = _v(a)
  low = a.val - a.err
  assert bool((low > 0).all())
  r = a.val ** q
  far = np.maximum(low ** (q - 1.0), (a.val + a.err) ** (q - 1.0))      # |d/dx x^q| is monotone: its maximum sits at an end
  return _rnd(r, abs(q) * far * a.err, 16.0)


def _scalars(h, f32):
  if not f32:
    return h, 1.0 - h.decay_or_rho
  f = np.float32
  h32 = Hyper(*(float(f(x)) for x in h))
  return h32, float(f(1.0) - f(h.decay_or_rho))


def step(rule, th, g, slots, hyper, gscale=1.0, f32_scalars=True):
  """One apply of ``rule``: th, g and the slot arrays are the values the launch read (any float arrays; taken as exact).
  -> ([theta', slot0', slot1'][:1 + nslots] as float64, the bounds of the fp32 results, same shapes)."""
  h, om = _scalars(hyper, f32_scalars)
  gs = float(np.float32(gscale)) if f32_scalars else float(gscale)
  th = V(th)
  gi = mul(V(g), gs)
  s = [V(x) for x in slots]
  assert len(s) == len(SLOT_NAMES[rule]), (rule, len(s))
  if rule == 'sgd':
    out = [fma(-h.lr, gi, th)]
  elif rule == 'momentum':
    a = fma(h.momentum, s[0], gi)
    out = [fma(-h.lr, a, th), a]
  elif rule == 'adagrad':
    a = fma(gi, gi, s[0])
    out = [sub(th, div(mul(h.lr, gi), sqrt(a))), a]
  elif rule == 'rmsprop':
    ms = fma(fma(gi, gi, V(-s[0].val, s[0].err)), om, s[0])
    mom = fma(h.momentum, s[1], div(mul(h.lr, gi), sqrt(add(ms, h.eps))))
    out = [sub(th, mom), ms, mom]
  elif rule == 'adadelta':
    accum = fma(h.decay_or_rho, s[0], mul(mul(om, gi), gi))
    u = mul(div(sqrt(add(s[1], h.eps)), sqrt(add(accum, h.eps))), gi)
    upd = fma(h.decay_or_rho, s[1], mul(mul(om, u), u))
    out = [fma(-h.lr, u, th), accum, upd]
  elif rule == 'ftrl':
    n = fma(gi, gi, s[0])
    if h.lr_power == -0.5:
      pn, pa = sqrt(n), sqrt(s[0])
    else:
      pn, pa = power(n, -h.lr_power), power(s[0], -h.lr_power)
    sigma = div(sub(pn, pa), h.lr)
    lin = fma(V(-sigma.val, sigma.err), th, add(s[1], gi))
    q = fma(2.0, h.l2, div(pn, h.lr))
    a = div(sub(np.copysign(h.l1, lin.val), lin), q)
    take = np.abs(lin.val) > h.l1
    ambiguous = np.abs(np.abs(lin.val) - h.l1) <= lin.err      # the fp32 comparison may go the other way: either value
    val = np.where(take, a.val, 0.0)
    err = np.where(ambiguous, np.abs(a.val) + a.err, np.where(take, a.err, 0.0))
    out = [V(val, err + TINY), n, lin]      # the floor: a bound of exactly 0 where the zero branch is certain
  else:
    raise ValueError(rule)
  return [o.val for o in out], [o.err for o in out]


def ema(avg, var, w):
  """tg_ema_update's element in float64 with the bound of tests/test_gpu_ema.py: avg - (avg - var) w."""
  w = float(w)
  want = avg - (avg - var) * w
  return want, 1.01 * U32 * (np.abs(want) + 2.0 * np.abs(avg - var) * w) + 2.0 ** -149
