"""Propagation and containment of Inf / NaN: the helpers and the case tables of tests/test_gpu_nonfinite.py.

Dynamic loss scaling looks at the flat fp32 gradient alone (tg_nonfinite_check), so an overflow in a 16-bit pass is noticed only
if every kernel between it and that gradient turns a non-finite input into a non-finite output (PROPAGATION); and a kernel that
clamps the addresses of its dead lanes, or pads with zeros, must not let a non-finite value reach an element that never
depended on it (CONTAINMENT).  With finite inputs neither fault changes a result.

A case plants one special value into otherwise ordinary inputs; the float64 oracle of the operation (oracle/np_ops.py, the
literal formulas of tests/elementwise.py), evaluated on the planted inputs and rounded where the product path stores, says which
output elements are non-finite -- `taint` -- and the kernel must agree element for element: every taint element non-finite
(NaN and Inf are not told apart: a summation order may turn one into the other), every other element finite and, where the
launch is bit-reproducible, bit-equal to the same launch on the unplanted inputs.  Elements the oracle changes without making
them non-finite (`touched`: a 60000 next to an overflow, a NaN in a mask source that only selects a slope) and every clean
element of a launch that is not bit-reproducible take the element-wise bound of their family (tests/elementwise.py) around the
oracle: no tolerance is introduced here.

Two ambiguities are avoided by the choice of inputs, not by a tolerance:
  * implicit zero padding times a non-finite: a filter gradient gets its plants, in `gy` and in `x` alike, only at pixels whose
    k x k window lies inside the image, so that no "0 of the padding x NaN" term exists and the padded-array oracle, a kernel
    that skips the outside taps and one that multiplies them by the padding's zeros agree;
  * weights: no non-finite is planted into weights or packs here (the trainer tests of tests/test_gpu_loss_scale.py do that).

Everything in this file runs on the CPU (tests/test_nonfinite_cpu.py checks the helpers on hand-made arrays and every case
against the three case conditions, over the oracle alone).
"""
import numpy as np

import elementwise as E
from oracle import np_ops as N

BIG = 60000.0      # finite in every storage type; two of them summed (unit weights) pass fp16's 65504
WHAT = {'+inf': np.inf, '-inf': -np.inf, 'nan': np.nan, 'big': BIG}
SPECIALS = ('+inf', '-inf', 'nan')
F16_MAX = 65504.0
DNAMES = ('bf16', 'f16', 'f32')


# ------------------------------------------------------------------------------------------------ planting
def plant(x, where, what):
  """A copy of the float32 / float64 host array `x` with WHAT[what] written at `where`: one index tuple, or a list of them."""
  assert what in WHAT, what
  out = np.array(x, copy=True)
  assert out.dtype in (np.float32, np.float64), out.dtype
  for idx in ([where] if isinstance(where, tuple) else list(where)):
    assert len(idx) == out.ndim and all(0 <= i < s for i, s in zip(idx, out.shape)), (idx, out.shape)
    out[idx] = WHAT[what]
  return out


def storage_round(a, dname):
  """float64 values as the storage type holds them (round to nearest even; past the largest finite number: Inf) -> float64."""
  import torch
  a = np.asarray(a, np.float64)
  if dname in ('f32', 'fp32', 'float32'):
    with np.errstate(over='ignore'):
      return a.astype(np.float32).astype(np.float64)
  dt = {'bf16': torch.bfloat16, 'f16': torch.float16}[dname]
  return torch.from_numpy(np.ascontiguousarray(a)).to(dt).double().numpy()


# ------------------------------------------------------------------------------------------------ position pickers
def vec_width(dname):
  """Elements of one 16-byte vector."""
  return 4 if dname in ('f32', 'fp32', 'float32') else 8


def at(shape, flat):
  return tuple(int(i) for i in np.unravel_index(int(flat), shape))


def first(shape):
  return (0,) * len(shape)


def last(shape):
  """Also the last pixel of the whole tensor: the element a clamped dead lane re-reads."""
  return tuple(s - 1 for s in shape)


def last_lane_of_vector(shape, dname, vec=0):
  """The last lane of 16-byte vector number `vec` of the flat tensor."""
  V = vec_width(dname)
  assert (vec + 1) * V <= int(np.prod(shape))
  return at(shape, vec * V + V - 1)


def behind_last_vector(shape, dname):
  """The first element behind the last whole 16-byte vector (numel % 8 != 0 in 16 bit, % 4 in fp32), else None."""
  V, numel = vec_width(dname), int(np.prod(shape))
  return at(shape, numel - numel % V) if numel % V else None


def norm_chunking(n, hw, pool=False):
  """csrc/norm.hip's own arithmetic (norm_chunks: ~1024 blocks; norm_stream_chunks: ~2048 blocks over pixels, or over 2x2
  blocks of the pooled forward; min_ppb: 16 / 32 / 64 pixels at hw <= 64 / <= 256 / above) -> ((chunks, ppb) of pass 1, the
  same of the streaming pass, in its own units).  tests/test_gpu_nonfinite.py checks pass 1 against tg_norm_chunks."""
  floor = 16 if hw <= 64 else 32 if hw <= 256 else 64
  ch = (1024 + n - 1) // n
  pp = max((hw + ch - 1) // ch, floor)
  units = hw // 4 if pool else hw
  c2 = (2048 + n - 1) // n
  pp2 = max((units + c2 - 1) // c2, 16 if pool else floor)
  return ((hw + pp - 1) // pp, pp), ((units + pp2 - 1) // pp2, pp2)


def block_edge_pixels(h, w, ppb):
  """(the last pixel of block 0's range, the first pixel of block 1's) as (row, column); needs more than one block."""
  assert ppb < h * w, 'one block holds the whole image: no edge'
  return (at((h, w), ppb - 1), at((h, w), ppb))


def last_pixel(h, w):
  return (h - 1, w - 1)


def last_image(n):
  return n - 1


def first_image_of_second_group(n, split):
  """The first image that takes the second weight / parameter set."""
  assert 0 < split < n
  return split


def interior_pixel(h, w, k=3):
  """A pixel whose k x k window lies inside the image."""
  assert h > k - 1 and w > k - 1
  return (h // 2, w // 2) if min(h, w) > k else ((k - 1) // 2, (k - 1) // 2)


def corner_pixel(h, w):
  return (0, 0)


def border_pixel(h, w):
  return (0, w // 2)


# ------------------------------------------------------------------------------------------------ what the oracle expects
class Sets(object):
  """ref: the oracle on the planted inputs, as stored; taint: where it is non-finite; touched: finite, but not what the oracle
  gives on the unplanted inputs; clean = ~taint (touched is a subset of clean)."""

  def __init__(self, ref, taint, touched):
    self.ref, self.taint, self.touched = ref, taint, touched
    self.clean = ~taint


def expected_sets(oracle_fn, planted_inputs, dtype, clean_inputs=None, storage=None):
  """Evaluates the float64 oracle `oracle_fn(inputs) -> {output name: array}` on the planted inputs and applies the storage
  rounding of each output (`storage[name]`, default `dtype`: the activations' type; 'f32' for losses and parameter
  gradients) -- in fp16 a result past 65504 is stored as Inf and is therefore taint.  With `clean_inputs` the oracle is
  evaluated on them too, and `touched` marks the finite elements the plant changed.  -> {name: Sets}."""
  storage = storage or {}
  with np.errstate(all='ignore'):
    ref = oracle_fn(planted_inputs)
    base = oracle_fn(clean_inputs) if clean_inputs is not None else None
  out = {}
  for name, r in ref.items():
    st = storage.get(name, dtype)
    r = storage_round(r, st)
    taint = ~np.isfinite(r)
    if base is None:
      touched = np.zeros(r.shape, bool)
    else:
      b = storage_round(base[name], st)
      assert np.all(np.isfinite(b)), 'the oracle is not finite on the unplanted inputs of output %r' % name
      touched = ~taint & (r != b)
    out[name] = Sets(r, taint, touched)
  return out


def check_case(sets, units=None):
  """The conditions every case must meet, so that no test passes by leaving everything out: taint and clean both non-empty;
  clean holds at least one whole unit (an index of axis units[name], default 0: an image, a row, a slice, a term) of an output
  that has more than one; taint covers at most half of the outputs' elements."""
  units = units or {}
  nt = sum(int(s.taint.sum()) for s in sets.values())
  total = sum(s.taint.size for s in sets.values())
  assert nt > 0, 'the oracle makes no output element non-finite: the case checks no propagation'
  assert nt < total, 'the clean set is empty: the case checks no containment'
  assert 2 * nt <= total, 'taint covers %d of %d output elements: more than half' % (nt, total)
  whole = False
  for name, s in sets.items():
    ax = units.get(name, 0)
    if s.taint.ndim == 0 or s.taint.shape[ax] < 2:
      continue
    per_unit = np.moveaxis(s.taint, ax, 0).reshape(s.taint.shape[ax], -1).any(axis=1)
    whole = whole or bool((~per_unit).any())
  assert whole, 'no output keeps one whole clean unit (image, row, slice, channel)'
  return nt, total


def _first(mask):
  return tuple(int(i) for i in np.argwhere(mask)[0])


def assert_propagates_and_contains(got, got_clean, taint, ref, bound, what, touched=None):
  """got: the kernel's output on the planted inputs (float64 host array; 16- and 32-bit values convert exactly, so equal bits
  are equal values with equal signs of zero).
    * every `taint` element is non-finite (NaN or Inf);
    * every other element is finite;
    * got_clean given (the caller launched the unplanted case twice and found equal bits: the launch is bit-reproducible): every
      clean element outside `touched` is bit-equal to got_clean, the same launch on the unplanted inputs;
    * otherwise, and for the `touched` elements: |got - ref| <= bound, the element-wise bound of the operator's family.
  On failure: how many elements are wrong, and the first index, of each kind."""
  got = np.asarray(got, np.float64)
  taint = np.asarray(taint, bool)
  assert got.shape == taint.shape, (what, got.shape, taint.shape)
  clean = ~taint
  assert taint.any() or clean.any()
  touched = np.zeros(taint.shape, bool) if touched is None else np.asarray(touched, bool) & clean
  finite = np.isfinite(got)
  msgs = []
  swallowed = taint & finite
  if swallowed.any():
    i = _first(swallowed)
    sat = int((swallowed & (np.abs(got) == F16_MAX)).sum())
    msgs.append('%d of %d taint elements are finite (swallowed), first at %s = %.9g%s'
                % (swallowed.sum(), taint.sum(), i, got[i], '; %d of them sit at 65504: a saturating store' % sat if sat else ''))
  leaked = clean & ~finite
  if leaked.any():
    i = _first(leaked)
    msgs.append('%d of %d clean elements are non-finite (leaked), first at %s = %r' % (leaked.sum(), clean.sum(), i, got[i]))
  by_bound = clean & finite
  if got_clean is not None:
    base = np.asarray(got_clean, np.float64)
    assert base.shape == got.shape and np.all(np.isfinite(base)), (what, 'the unplanted launch is not finite')
    same = np.ascontiguousarray(got).view(np.int64) == np.ascontiguousarray(base).view(np.int64)
    moved = clean & finite & ~touched & ~same
    if moved.any():
      i = _first(moved)
      msgs.append('%d clean elements differ in bits from the unplanted launch, first at %s: %.9g, unplanted %.9g'
                  % (moved.sum(), i, got[i], base[i]))
    by_bound = by_bound & touched
  if by_bound.any():
    assert ref is not None and bound is not None, (what, 'elements on the bound route need the oracle and its bound')
    ref = np.asarray(ref, np.float64)
    bound = np.broadcast_to(np.asarray(bound, np.float64), got.shape)
    assert np.all(np.isfinite(ref[by_bound])) and np.all(bound[by_bound] > 0), (what, 'the reference or its bound is not finite / positive')
    with np.errstate(invalid='ignore', over='ignore'):
      ratio = np.abs(got - ref) / bound
    out = by_bound & ~(ratio <= 1.0)
    if out.any():
      i = _first(out)
      msgs.append('%d of %d clean elements outside their bound, first at %s: got %.9g ref %.9g bound %.3g'
                  % (out.sum(), by_bound.sum(), i, got[i], ref[i], bound[i]))
  assert not msgs, '%s: %s; shape %s' % (what, '; '.join(msgs), got.shape)


# ------------------------------------------------------------------------------------------------ the case tables
class Case(object):
  """One planted operation.  family: the launcher of tests/test_gpu_nonfinite.py that runs it; make(dname) -> {input name:
  float64 array, as stored}; plants(inputs, dname) -> [(input name, index)], all planted at once; oracle(inputs) -> {output
  name: float64 array}; storage: outputs not stored in the activations' type; units: the axis whose indices are an output's
  units (default 0); bound(inputs, sets, dname) -> {output name: bound}, needed by the outputs in `atomic` (their launch meets
  in atomics, so bit-equality is not theirs to give) and by cases with `touched` elements; par: what the launcher needs
  besides the tensors.  whats: the special values the case is run with ('big' runs in fp16 alone: elsewhere it is finite)."""

  def __init__(self, family, name, dnames, whats, make, plants, oracle, storage=None, units=None, bound=None, atomic=(), par=None,
               fast=False):
    self.family, self.name, self.dnames, self.whats = family, name, tuple(dnames), tuple(whats)
    self.make, self.plants, self.oracle = make, plants, oracle
    self.storage, self.units, self.bound, self.atomic, self.par, self.fast = storage or {}, units or {}, bound, tuple(atomic), par or {}, fast
    self.id = '%s-%s' % (family, name)

  def triples(self):
    return [(self, d, w) for d in self.dnames for w in self.whats if w != 'big' or d == 'f16']

  def planted(self, inputs, dname, what):
    out = dict(inputs)
    where = {}
    for name, idx in self.plants(inputs, dname):
      if idx is not None:
        where.setdefault(name, []).append(idx)
    assert where, 'the case plants nothing'
    for name, idxs in where.items():
      out[name] = storage_round(plant(inputs[name], idxs, what), 'f32' if name in self.par.get('f32_inputs', ()) else dname)
    return out

  def expected(self, inputs, planted, dname):
    return expected_sets(self.oracle, planted, dname, clean_inputs=inputs, storage=self.storage)


def _rand(shape, dname, seed, scale=1.0, offset=0.0):
  return storage_round(np.random.RandomState(seed).standard_normal(shape) * scale + offset, dname)


CASES = []


def _add(*a, **k):
  CASES.append(Case(*a, **k))


# ---- loss tail (csrc/reduce.hip).  Scalar losses are run as three independent launches, one per row, the plant in row 1: the
# output of the case is the vector of the three losses and the matrix of their gradients.
PRED_MODES = [('hinge_real', 1, 1.0, -1.0), ('hinge_fake', 1, 1.0, 1.0), ('xent_1', 2, 1.0, 0.0), ('xent_0', 2, 0.0, 0.0), ('square', 3, 0.0, 0.0),
              ('wgan', 0, 0.0, 0.0)]
PRED_N, PRED_W, PRED_G = 257, 0.3, 2.5      # 257: a second trip of the 256-thread workgroup


def _pred_oracle(mode, a, b):
  def oracle(inp):
    x = inp['x']
    k = PRED_W / x.shape[1]
    return dict(loss=k * N.pred_loss_term(x, mode, a, b).sum(axis=1), gx=PRED_G * k * N.pred_loss_term_grad(x, mode, a, b))
  return oracle


def _pred_bound(mode, a, b):
  def bound(inp, sets, dname):
    x = inp['x']
    n = x.shape[1]
    with np.errstate(all='ignore'):
      f, df, parts, term_ops, sig = E.pred_loss_reference(x, mode, a, b)
      g = PRED_G * PRED_W / n
      return dict(loss=np.array([E.pred_loss_fwd_bound(parts[r].sum(), n, PRED_W / n, term_ops) for r in range(x.shape[0])]),
                  gx=E.pred_loss_bwd_bound(sets['gx'].ref, abs(g), sig))
  return bound


for _name, _mode, _a, _b in PRED_MODES:
  _add('pred_loss', _name, ('f32',), SPECIALS, lambda d: dict(x=_rand((3, PRED_N), 'f32', 11, 2.0)),
       lambda inp, d: [('x', (1, 0)), ('x', (1, PRED_N - 1))], _pred_oracle(_mode, _a, _b), storage=dict(loss='f32', gx='f32'),
       bound=_pred_bound(_mode, _a, _b), par=dict(mode=_mode, a=_a, b=_b), fast=_name in ('hinge_real', 'xent_0'))

PRED_JOBS = [      # (group, term, mode, a, b, coef): every mode, two groups into term 0, term 3 fed by nobody, term 4 without a gradient
    (0, 0, 1, 1.0, -1.0, 0.5), (2, 0, 1, 1.0, 1.0, 0.5), (1, 1, 2, 1.0, 0.0, 0.7), (1, 2, 2, 0.0, 0.0, 0.3),
    (0, 2, 3, 0.0, 0.0, 1e-3), (2, 1, 0, 0.0, 0.0, -1.0), (1, 4, 1, 1.0, 1.0, 2.0), (0, 4, 0, 0.0, 0.0, 1.0)]
PRED_GTS = [1.5, -0.5, 2.0, None, None]


def _pred_losses_oracle(inp):
  x = inp['x']
  groups, gs = x.shape
  terms, gx = np.zeros(5), np.zeros_like(x)
  for grp, t, mode, a, b, coef in PRED_JOBS:
    terms[t] += coef * N.pred_loss_term(x[grp], mode, a, b).sum() / gs
    if PRED_GTS[t] is not None:
      gx[grp] += PRED_GTS[t] * coef / gs * N.pred_loss_term_grad(x[grp], mode, a, b)
  return dict(terms=terms, gx=gx)


def _pred_losses_bound(inp, sets, dname):
  x = inp['x']
  groups, gs = x.shape
  tb, gb = np.zeros(5), np.full_like(x, E.TINY)
  with np.errstate(all='ignore'):
    for grp, t, mode, a, b, coef in PRED_JOBS:
      f, df, parts, term_ops, sig = E.pred_loss_reference(x[grp], mode, a, b)
      tb[t] += E.pred_loss_fwd_bound(parts.sum(), gs, coef / gs, term_ops, extra_ops=3)
      if PRED_GTS[t] is not None:
        k = PRED_GTS[t] * coef / gs
        gb[grp] += E.pred_loss_bwd_bound(k * df, abs(k), sig, ops=6)
  return dict(terms=np.maximum(tb, E.TINY), gx=gb)


# a plant in group 2 taints terms 0 and 1 (its jobs) and its own gradient element; terms 2, 3, 4 and the other groups stay
for _grp, _pos in ((2, 'last'), (0, 'first')):
  _add('pred_losses', 'group%d_%s' % (_grp, _pos), ('f32',), SPECIALS, lambda d: dict(x=_rand((3, 257), 'f32', 12, 2.0)),
       (lambda g, p: lambda inp, d: [('x', (g, 256 if p == 'last' else 0))])(_grp, _pos), _pred_losses_oracle,
       storage=dict(terms='f32', gx='f32'), bound=_pred_losses_bound, fast=_grp == 2)

ABS_SHAPE, ABS_W, ABS_G = (3, 5, 7, 3), 0.1, 3.0      # 315 elements: a tail behind the last vector in every type


def _abs_oracle(inp):
  a, b = inp['a'], inp['b']
  gb, ga = N.absolute_difference_grad(b, a, ABS_W)
  return dict(loss=np.array([N.absolute_difference(b, a, ABS_W)]), ga=ABS_G * ga, gb=ABS_G * gb)


_add('abs_diff', 'vector_edges', DNAMES, SPECIALS,
     lambda d: dict(a=_rand(ABS_SHAPE, d, 13), b=_rand(ABS_SHAPE, d, 14)),
     lambda inp, d: [('a', first(ABS_SHAPE)), ('a', last_lane_of_vector(ABS_SHAPE, d, 1)), ('b', behind_last_vector(ABS_SHAPE, d)),
                     ('b', last(ABS_SHAPE))],
     _abs_oracle, storage=dict(loss='f32'), fast=True)

GP_LAM, GP_G = 10.0, 2.0


def _gp_oracle(inp):
  g = inp['g']
  b = g.shape[0]
  coef = N.gradient_penalty_coef((g.reshape(b, -1) ** 2).sum(axis=1), GP_LAM)
  return dict(loss=np.array([N.gradient_penalty(g, GP_LAM)]), gg=GP_G * coef.reshape((b,) + (1,) * (g.ndim - 1)) * g)


for _shape, _where in (((4, 3, 5, 5), 'last'), ((4, 4, 4, 4), 'first')):      # per = 75: samples off the 16-byte boundary; 64: on it
  _add('gradient_penalty', 'per%d_%s' % (int(np.prod(_shape[1:])), _where), DNAMES, SPECIALS,
       (lambda s: lambda d: dict(g=_rand(s, d, 15, 1.0 / np.sqrt(np.prod(s[1:])))))(_shape),
       (lambda s, w: lambda inp, d: [('g', last(s) if w == 'last' else (1,) + (0,) * 3)])(_shape, _where),
       _gp_oracle, storage=dict(loss='f32'), fast=_where == 'last')

VAR_SHAPE = (3, 2, 5, 5, 3)      # three launches of [2, 5, 5, 3]


def _var_oracle(inp):
  x, noise, alpha = inp['x'], inp['noise'], inp['alpha']
  var = np.array([np.var(x[r]) for r in range(x.shape[0])])
  return dict(var=var, interp=x + 0.5 * alpha[:, :, None, None, None] * noise * var[:, None, None, None, None])


_add('variance', 'dragan', DNAMES, SPECIALS,
     lambda d: dict(x=_rand(VAR_SHAPE, d, 16), noise=_rand(VAR_SHAPE, d, 17), alpha=storage_round(np.random.RandomState(18).rand(3, 2), 'f32')),
     lambda inp, d: [('x', (1, 1, 4, 4, 2))], _var_oracle, storage=dict(var='f32'), par=dict(f32_inputs=('alpha',)), fast=True)

SUM_SHAPE = (3, 4, 5, 9)      # three launches of a [4, 5, 9] mean; three tf.add_n of four terms


def _sums_oracle(inp):
  x, t, g = inp['x'], inp['t'], inp['g']
  k = -1.0 / x[0].size
  return dict(mean=k * x.reshape(3, -1).sum(axis=1), gmean=np.broadcast_to((k * g).reshape(3, 1, 1, 1), x.shape).copy(), add_n=t.sum(axis=1))


_add('sums', 'mean_fill_add_n', DNAMES, SPECIALS,
     lambda d: dict(x=_rand(SUM_SHAPE, d, 19), t=_rand((3, 4), 'f32', 20), g=_rand((3,), 'f32', 21)),
     lambda inp, d: [('x', (1, 3, 4, 8)), ('t', (1, 3)), ('g', (1,))], _sums_oracle, storage=dict(mean='f32', add_n='f32'),
     par=dict(f32_inputs=('t', 'g')), fast=True)


# ---- streaming ops (csrc/pointwise.hip, norm.hip, reduce.hip): exact images of the plant
ST_SHAPE = (3, 6, 10, 5)      # 900 elements, c = 5: the scalar paths, a tail behind the last vector in 16 bit
ST_VEC = (3, 4, 6, 8)         # c = 8: the 16-byte paths
AXPBY = (float(np.float32(0.3)), float(np.float32(-1.7)))
ALPHA = float(np.float32(0.2))


def _up2(a):
  return a.repeat(2, axis=1).repeat(2, axis=2)


def _sum4(a):
  n, h, w, c = a.shape
  return a.reshape(n, h // 2, 2, w // 2, 2, c).sum(axis=(2, 4))


def _edges(shape, name):
  return lambda inp, d: [(name, first(shape)), (name, last_lane_of_vector(shape, d, 2)), (name, behind_last_vector(shape, d)), (name, last(shape))]


_add('axpby', 'vector_edges', DNAMES, SPECIALS, lambda d: dict(x=_rand(ABS_SHAPE, d, 30), y=_rand(ABS_SHAPE, d, 31)), _edges(ABS_SHAPE, 'y'),
     lambda inp: dict(out=AXPBY[0] * inp['x'] + AXPBY[1] * inp['y']), fast=True)
_add('lerp', 'fade_in', DNAMES, SPECIALS, lambda d: dict(x=_rand(ST_SHAPE, d, 30), y=_rand(ST_SHAPE, d, 31)),
     lambda inp, d: [('x', last(ST_SHAPE)), ('y', first(ST_SHAPE))], lambda inp: dict(out=N.lerp(inp['x'], inp['y'], 0.25)), fast=True)
_add('axpby', 'big_sum', ('f16',), ('big',), lambda d: dict(x=_rand(ABS_SHAPE, d, 30), y=_rand(ABS_SHAPE, d, 31)),
     lambda inp, d: [('x', (1, 2, 3, 1)), ('y', (1, 2, 3, 1)), ('x', last(ABS_SHAPE))], lambda inp: dict(out=inp['x'] + inp['y']),
     bound=lambda inp, sets, d: dict(out=E.conv_bound(sets['out'].ref, np.abs(inp['x']) + np.abs(inp['y']), 3, d)), par=dict(ab=(1.0, 1.0)))
_add('sample_lerp', 'last', DNAMES, SPECIALS,
     lambda d: dict(x=_rand(ST_SHAPE, d, 32), y=_rand(ST_SHAPE, d, 33), alpha=storage_round(np.random.RandomState(34).rand(3), 'f32')),
     lambda inp, d: [('y', last(ST_SHAPE)), ('x', (1, 0, 0, 0))],
     lambda inp: dict(out=inp['x'] + inp['alpha'].reshape(-1, 1, 1, 1) * (inp['y'] - inp['x'])), par=dict(f32_inputs=('alpha',)))
# a plant in one image's alpha taints that image alone
_add('sample_lerp', 'alpha', DNAMES, SPECIALS,
     lambda d: dict(x=_rand(ST_SHAPE, d, 32), y=_rand(ST_SHAPE, d, 33), alpha=storage_round(np.random.RandomState(34).rand(3), 'f32')),
     lambda inp, d: [('alpha', (2,))], lambda inp: dict(out=inp['x'] + inp['alpha'].reshape(-1, 1, 1, 1) * (inp['y'] - inp['x'])),
     par=dict(f32_inputs=('alpha',)))
GDROP_S = float(np.float32(0.37))
_add('gdrop', 'noise', DNAMES, SPECIALS, lambda d: dict(x=_rand(ST_VEC, d, 35), noise=_rand((3, 8), 'f32', 36)),
     lambda inp, d: [('noise', (1, 7)), ('x', last(ST_VEC))],
     lambda inp: dict(out=inp['x'] * (inp['noise'] * (GDROP_S * float(np.sqrt(np.float32(8)))) + 1.0)[:, None, None, :]),
     par=dict(f32_inputs=('noise',)))
# cast: fp32 -> 16 bit.  The launcher doubles the fp32 input on the host (exact), so that `big` arrives as 120000
_add('cast', 'from_f32', ('bf16', 'f16'), SPECIALS + ('big',), lambda d: dict(x=_rand((3, 35), 'f32', 37)),
     lambda inp, d: [('x', (0, 0)), ('x', (1, 7)), ('x', (1, 32)), ('x', (1, 34))], lambda inp: dict(out=2.0 * inp['x']),
     par=dict(f32_inputs=('x',)), fast=True)
_add('cast', 'to_f32', ('bf16', 'f16'), SPECIALS, lambda d: dict(x=_rand((3, 35), d, 38)),
     lambda inp, d: [('x', (1, 7)), ('x', (2, 34))], lambda inp: dict(out=inp['x']), storage=dict(out='f32'), par=dict(to_f32=True))


def _lrelu_oracle(inp):
  slope = np.where(inp['z'] > 0, 1.0, ALPHA)      # np.where: a NaN in the mask source selects alpha
  return dict(out=inp['g'] * slope)


def _lrelu_pos(inp):
  return at(ST_SHAPE, int(np.argmax(inp['z'].reshape(-1) > 0.5)))      # a mask element whose slope the NaN changes


_add('lrelu_bwd', 'gradient_and_mask_source', DNAMES, ('nan',), lambda d: dict(g=_rand(ST_SHAPE, d, 39), z=_rand(ST_SHAPE, d, 40)),
     lambda inp, d: [('g', last(ST_SHAPE)), ('g', first(ST_SHAPE)), ('z', _lrelu_pos(inp))], _lrelu_oracle,
     bound=lambda inp, sets, d: dict(out=E.conv_bound(sets['out'].ref, np.abs(sets['out'].ref), 1, d)), fast=True)
_add('lrelu_bwd', 'gradient', DNAMES, ('+inf', '-inf'), lambda d: dict(g=_rand(ST_SHAPE, d, 39), z=_rand(ST_SHAPE, d, 40)),
     lambda inp, d: [('g', last(ST_SHAPE)), ('g', behind_last_vector(ST_SHAPE, d))], _lrelu_oracle)


def _lrelu_pool_oracle(inp):
  c = inp['z'].shape[3]
  g = (inp['gz'] + 0.25 * _up2(inp['gzp'])) * np.where(inp['z'] > 0, 1.0, ALPHA)
  return dict(g=g, gb=g.reshape(-1, c).sum(axis=0))


def _lrelu_pool_bound(inp, sets, d):
  """tests/test_gpu_ops.py test_lrelu_backward_family_elementwise: two fp32 operations per element; the bias gradient is the
  fp32 sum of the STORED g over P pixels: wgrad_bound plus the sum of the elements' own bounds."""
  c = inp['z'].shape[3]
  slope = np.where(inp['z'] > 0, 1.0, ALPHA)
  ref = np.nan_to_num(sets['g'].ref, nan=0.0, posinf=0.0, neginf=0.0)
  mag = np.nan_to_num((np.abs(inp['gz']) + 0.25 * _up2(np.abs(inp['gzp']))) * slope, nan=0.0, posinf=0.0, neginf=0.0)
  gbound = E.conv_bound(ref, mag, 2, d)
  P = ref.size // c
  return dict(g=gbound, gb=E.wgrad_bound(ref.reshape(-1, c).sum(axis=0), np.abs(ref).reshape(-1, c).sum(axis=0), P) + gbound.reshape(-1, c).sum(axis=0))


for _shape in (ST_SHAPE, ST_VEC):      # a pooled-gradient plant: its 2x2 block, and the bias gradient of its channel alone
  _add('lrelu_pool_bwd', 'c%d' % _shape[3], DNAMES, SPECIALS,
       (lambda s: lambda d: dict(gz=_rand(s, d, 41), z=_rand(s, d, 42), gzp=_rand((s[0], s[1] // 2, s[2] // 2, s[3]), d, 43)))(_shape),
       (lambda s: lambda inp, d: [('gzp', (s[0] - 1, s[1] // 2 - 1, s[2] // 2 - 1, s[3] - 1))])(_shape), _lrelu_pool_oracle,
       storage=dict(gb='f32'), units=dict(gb=0), bound=_lrelu_pool_bound, atomic=('gb',), fast=_shape is ST_SHAPE)


def _pool_oracle(inp):
  return dict(y=0.25 * _sum4(inp['x']), gx=0.25 * _up2(inp['gy']))


for _shape in (ST_SHAPE, ST_VEC):      # forward: the pooled pixel; backward: the 2x2 block
  _add('pool', 'c%d' % _shape[3], DNAMES, SPECIALS,
       (lambda s: lambda d: dict(x=_rand(s, d, 44), gy=_rand((s[0], s[1] // 2, s[2] // 2, s[3]), d, 45)))(_shape),
       (lambda s: lambda inp, d: [('x', last(s)), ('x', (1, 1, 2, 0)), ('gy', (s[0] - 1, s[1] // 2 - 1, s[2] // 2 - 1, s[3] - 1)), ('gy', (0, 0, 0, 1))])(_shape),
       _pool_oracle, fast=_shape is ST_SHAPE)
_add('pool', 'big_c5', ('f16',), ('big',), lambda d: dict(x=_rand(ST_SHAPE, d, 44), gy=_rand((3, 3, 5, 5), d, 45)),
     lambda inp, d: [('x', (1, 2, 4, 3)), ('x', (1, 2, 5, 3)), ('x', (1, 3, 4, 3)), ('x', (1, 3, 5, 3)), ('x', (1, 4, 4, 3)), ('x', (2, 5, 9, 4))],
     lambda inp: dict(y=_sum4(inp['x'])), par=dict(scale=1.0, fwd_only=True),
     # a 60000 next to values of size 1: the fp32 sum of four stored values is not exact here -- three additions round
     bound=lambda inp, sets, d: dict(y=E.conv_bound(sets['y'].ref, _sum4(np.abs(inp['x'])), 3, d)))


def _upcat_oracle(inp):
  c0 = inp['x0'].shape[3]
  return dict(out=np.concatenate([_up2(inp['x0']), inp['x1']], axis=3), g0=_sum4(inp['go'][..., :c0]), g1=inp['go'][..., c0:].copy())


_add('upsample_concat', 'c5_c8', DNAMES, SPECIALS,
     lambda d: dict(x0=_rand((3, 3, 5, 5), d, 46), x1=_rand((3, 6, 10, 8), d, 47), go=_rand((3, 6, 10, 13), d, 48)),
     lambda inp, d: [('x0', (2, 2, 4, 4)), ('x1', (0, 0, 0, 0)), ('x1', (2, 5, 9, 7)), ('go', (1, 3, 3, 2)), ('go', (2, 5, 9, 12))],
     _upcat_oracle, fast=True)


# ---- fused normalisers (csrc/norm.hip).  3 images of 8 x 8: four pixel blocks of 16 in pass 1 and in the streaming passes
# (norm_chunking), one block of 16 2x2 units in the pooled forward.  The plants sit in ONE (image, channel): on both sides of
# the first block edge (pixels 15 | 16), and at the last pixel -- of the last image, the one a clamped dead lane re-reads.
NORM_N, NORM_H, NORM_W, NORM_C = 3, 8, 8, 16
NORM_VARIANTS = [      # name, layer norm, pixel norm, pool, split
    ('instance_pn', False, True, False, None), ('instance_split1', False, False, False, 1), ('instance_pn_pool_split2', False, True, True, 2),
    ('layer_pn', True, True, False, None), ('layer_split1', True, False, False, 1)]


def _norm_make(pool, shape=None, rows=False):
  def make(d):
    rng = np.random.RandomState(50)
    s = shape or (NORM_N, NORM_H, NORM_W, NORM_C)
    n, h, w, c = s
    inp = dict(y=storage_round(rng.randn(*s) * 1.5 + 0.7, d), gz=storage_round(rng.randn(*s), d))
    for k, (o, sc) in zip(('gamma', 'beta', 'gamma2', 'beta2'), ((1.0, 0.2), (0.0, 0.1)) * 2):
      inp[k] = storage_round(o + sc * (rng.randn(n, c) if rows else rng.randn(c)), 'f32')
    if pool:
      inp['gzp'] = storage_round(rng.randn(n, h // 2, w // 2, c), d)
    return inp
  return make


def _norm_refs(inp, layer, pn, pool, split, dt):
  import torch
  t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
  two = split is not None
  r = E.norm_act_reference(t(inp['y']).to(dt), t(inp['gamma']), t(inp['beta']), t(inp['gz']), t(inp['gamma2']) if two else None,
                           t(inp['beta2']) if two else None, split=split, lrelu=True, pixel_norm=pn, pool=pool,
                           gzp=t(inp['gzp']) if pool else None, layer=layer, eps=1e-12 if layer else 1e-6)
  out = dict(z=r['z'], gy=r['gy'], ggamma=r['grads'][0], gbeta=r['grads'][1])
  if pool:
    out['zp'] = r['zp']
  if two:
    out.update(ggamma2=r['grads'][2], gbeta2=r['grads'][3])
  return {k: v.double().numpy() for k, v in out.items()}


def _norm_oracle(layer, pn, pool, split):
  import torch
  return lambda inp: _norm_refs(inp, layer, pn, pool, split, torch.float64)


def _norm_bound(layer, pn, pool, split):
  def bound(inp, sets, d):
    """u |ref| + 16 E32 (elementwise.e32_bound), E32 over the elements the oracle leaves finite."""
    import torch
    r32 = _norm_refs(inp, layer, pn, pool, split, torch.float32)
    out = {}
    for k, s in sets.items():
      ok = s.clean & np.isfinite(r32[k])
      out[k] = E.e32_bound(np.where(s.clean, s.ref, 0.0), E.e32(r32[k][ok], s.ref[ok]), 'f32' if k.startswith('g') and k != 'gy' else d)
    return out
  return bound


def _norm_plants(tensor, image, shape=None):
  def plants(inp, d):
    n, h, w, _ = shape or (NORM_N, NORM_H, NORM_W, NORM_C)
    (_, ppb), (_, ppb2) = norm_chunking(n, h * w)
    px = list(block_edge_pixels(h, w, ppb)) + (list(block_edge_pixels(h, w, ppb2)) if ppb2 != ppb else []) + [last_pixel(h, w)]
    return [(tensor, (image,) + p + (3,)) for p in px]
  return plants


# ---- row softmax and the batched GEMM (csrc/attention.hip)
SM_SHAPE = (6, 100)      # rows of 100 scores: wider than a wave, no multiple of a vector in fp32


def _softmax_fwd(s, dt=np.float64):
  s = np.asarray(s, dt)
  e = np.exp(s - s.max(-1, keepdims=True))      # +inf: inf - inf; NaN: the maximum itself -- the whole row is NaN either way
  return e / e.sum(-1, keepdims=True, dtype=dt)


def _softmax_bwd(p, dp, dt=np.float64):
  p, dp = np.asarray(p, dt), np.asarray(dp, dt)
  return p * (dp - (dp * p).sum(-1, keepdims=True, dtype=dt))


def _softmax_bound(inp, sets, d):
  """e32_bound, each kernel on the operands it reads (elementwise.softmax_kernels_reference's formulas), E32 over the rows the
  oracle leaves finite."""
  with np.errstate(all='ignore'):
    r32 = dict(p=_softmax_fwd(inp['s'], np.float32), ds=_softmax_bwd(inp['p'], inp['dp'], np.float32))
  out = {}
  for k, s in sets.items():
    ok = s.clean & np.isfinite(r32[k])
    out[k] = E.e32_bound(np.where(s.clean, s.ref, 0.0), E.e32(r32[k][ok], s.ref[ok]), d)
  return out


def _softmax_make(d):
  rng = np.random.RandomState(70)
  return dict(s=storage_round(rng.randn(*SM_SHAPE) * 2.0, d), p=storage_round(_softmax_fwd(rng.randn(*SM_SHAPE)), d),
              dp=storage_round(rng.randn(*SM_SHAPE), d))


_softmax_oracle = lambda inp: dict(p=_softmax_fwd(inp['s']), ds=_softmax_bwd(inp['p'], inp['dp']))
# +inf or NaN in one score: the whole row of p; in one incoming gradient: the whole row of ds (through the row sum)
_add('softmax_rows', 'row', DNAMES, ('+inf', 'nan'), _softmax_make, lambda inp, d: [('s', (2, 99)), ('s', (5, 0)), ('dp', (0, 50))],
     _softmax_oracle, bound=_softmax_bound, fast=True)
# -inf in one score is an ordinary score: probability 0, the row stays finite (touched); the taint of this case is the row of
# ds whose incoming gradient holds the -inf
_add('softmax_rows', 'minus_inf_score', DNAMES, ('-inf',), _softmax_make, lambda inp, d: [('s', (4, 7)), ('s', (5, 99)), ('dp', (1, 5))],
     _softmax_oracle, bound=_softmax_bound, fast=True)

GEMM_BMNK = (3, 33, 9, 40)      # ragged m, n and k tiles


def _gemm_oracle(inp):
  nn = 0.5 * np.einsum('bmk,bkn->bmn', inp['a'], inp['b'])
  return dict(c=nn, ct=0.5 * np.einsum('bkm,bnk->bmn', inp['at'], inp['bt']), cnt=0.5 * np.einsum('bmk,bnk->bmn', inp['a'], inp['bt']),
              ctn=0.5 * np.einsum('bkm,bkn->bmn', inp['at'], inp['b']), cabi=inp['c0'] + nn)


def _gemm_make(d):
  b, m, n, k = GEMM_BMNK
  rng = np.random.RandomState(71)
  a, bb = storage_round(rng.randn(b, m, k), d), storage_round(rng.randn(b, k, n), d)
  return dict(a=a, b=bb, at=np.ascontiguousarray(a.transpose(0, 2, 1)), bt=np.ascontiguousarray(bb.transpose(0, 2, 1)),
              c0=storage_round(rng.randn(b, m, n), d))


# a plant in one row of A: that output row; in one column of B: that output column; batch entry 0 keeps its bits.  Plain and
# with both operands transposed, and (cabi) through the C ABI: rows three elements apart from each other with NaN between
# them, accumulate = 1 into a C that holds finite values
_add('bgemm', 'row_and_column', DNAMES, SPECIALS, _gemm_make,
     lambda inp, d: [('a', (1, 32, 39)), ('b', (2, 0, 8)), ('at', (1, 39, 32)), ('bt', (2, 8, 0))], _gemm_oracle, fast=True)


# ---- convolutions, forward and backward-data with their masked forms (csrc/conv_small.hip, conv_mfma.hip, conv_tile.hip).
# Shapes and symbols: the smallest recorded rows of tests/golden/dispatch_edge_kernels.json per kernel.  The oracle runs on the
# planted images and image 0 alone (the returned arrays hold 0 elsewhere: never read -- those images are clean, untouched, and
# take the bit-equality with the unplanted launch; these kernels have no atomics).  x is also the mask source of the masked
# backward-data and gy the mask source of the masked forward: a plant there selects the slope alpha (np.where) and leaves the
# output finite -- `touched`, held to the family's bound.
CONV_SHAPES = [      # name, k, padding, hw, cin, cout, n, the kernel family tg_last_kernel() must name
    ('small_k1_hw8_n64', 1, 'SAME', 8, 32, 32, 64, 'conv_small_kernel<1,'),
    ('mfma_k1_hw8_n65', 1, 'SAME', 8, 32, 32, 65, 'conv_fwd_mfma<1,1,'),
    ('small_k3_hw8_c24_n64', 3, 'SAME', 8, 24, 40, 64, 'conv_small_kernel<9,'),
    ('mfma_k3_hw8_c24_n65', 3, 'SAME', 8, 24, 40, 65, 'conv_fwd_mfma<3,3,'),
    ('tile_k3_hw128_c48_n7', 3, 'SAME', 128, 48, 64, 7, 'conv_tile_kernel<3,'),           # 32-channel output blocks
    ('tile_bn64_k3_hw128_c48_n8', 3, 'SAME', 128, 48, 64, 8, 'conv_tile_kernel<3,'),      # 64-channel output blocks
    ('tile_mt2_k3_hw128_c64_n8', 3, 'SAME', 128, 64, 32, 8, 'conv_tile_kernel<3,'),       # two sub-tiles per wave
    ('tile_wres32_k3_hw128_n16', 3, 'SAME', 128, 32, 32, 16, 'conv_tile_wres_kernel<3,'),
    ('thin16_k3_hw128_n16', 3, 'SAME', 128, 16, 16, 16, 'conv_thin16_kernel<16'),
    ('small_k3_hw4_n256', 3, 'SAME', 4, 32, 32, 256, 'conv_small_kernel<9,'),             # a 4x4 map
    ('dense_k4_valid_hw4_n4096', 4, 'VALID', 4, 8, 8, 4096, 'conv_small_kernel<1,'),      # the dense 4x4-VALID rewrite
    ('img_k3_hw8_c32_n5', 3, 'SAME', 8, 32, 32, 5, 'conv_img_kernel<'),
    ('img_k3_hw8_c512_c256_n3', 3, 'SAME', 8, 512, 256, 3, 'conv_img_kernel<'),           # its LDS-above-64-KB variant
    ('direct_k3_hw6_c5_c7_n3', 3, 'SAME', 6, 5, 7, 3, 'direct'),                          # channel counts the MFMA kernels refuse
]


def _conv_make(k, hw, cin, cout, n, ones=False):
  def make(d):
    rng = np.random.RandomState(60 + k + cin)
    w = np.ones((k, k, cin, cout)) if ones else storage_round(rng.randn(k, k, cin, cout) / np.sqrt(k * k * cin), d)
    ho = hw if k % 2 else hw - k + 1      # SAME for the odd kernels, VALID for the 4x4
    return dict(x=storage_round(rng.randn(n, hw, hw, cin), d), gy=storage_round(rng.randn(n, ho, ho, cout), d), w=w,
                b=storage_round(0.1 * rng.randn(cout), 'f32'))
  return make


def _conv_sel(n):
  return sorted({0, 1, n - 1})


def _conv_terms(inp, k, pad, absolute=False):
  """The four outputs on the selected images (and, absolute: the magnitude terms of their bounds).  A stacked kernel
  [2, k, k, cin, cout] holds two weight sets: the first half of the batch takes set 0, the second set 1."""
  n, hw = inp['x'].shape[0], inp['x'].shape[1]
  sel = _conv_sel(n)
  f = np.abs if absolute else (lambda a: a)
  x, gy, w = inp['x'][sel], inp['gy'][sel], inp['w']
  if w.ndim == 5:
    sets = [2 * i // n for i in sel]
    lin = np.concatenate([N.conv2d_gemm(f(x[j:j + 1]), f(w[g]), pad) for j, g in enumerate(sets)])
    back = np.concatenate([N.conv2d_bwd_data_gemm(f(gy[j:j + 1]), f(w[g]), (hw, hw), pad) for j, g in enumerate(sets)])
  else:
    lin = N.conv2d_gemm(f(x), f(w), pad)
    back = N.conv2d_bwd_data_gemm(f(gy), f(w), (hw, hw), pad)
  return sel, lin, back, np.where(gy > 0, 1.0, ALPHA), np.where(x > 0, 1.0, ALPHA)


def _conv_bias(inp, sel):
  b, n = inp['b'], inp['x'].shape[0]
  return b if b.ndim == 1 else np.stack([b[2 * i // n] for i in sel])[:, None, None, :]


def sign_bytes(z, taint=None):
  """The sign bytes of conv_fwd_pool_signs: bit j of byte [.., c // 8] is z[.., 8 (c // 8) + j] > 0; NaN where one of the
  byte's eight channels is non-finite (`taint`, default: z itself) -- such a byte is not pinned."""
  bits = (z > 0).reshape(z.shape[:-1] + (z.shape[-1] // 8, 8))
  by = (bits * (1 << np.arange(8))).sum(axis=-1).astype(np.float64)
  bad = (~np.isfinite(z) if taint is None else taint).reshape(bits.shape).any(axis=-1)
  return np.where(bad, np.nan, by)


def _conv_oracle(k, pad, extras=False):
  def oracle(inp):
    sel, lin, back, ms_f, ms_b = _conv_terms(inp, k, pad)
    pre = lin + _conv_bias(inp, sel)
    act = np.where(pre > 0, pre, ALPHA * pre)
    outs = dict(fwd=act, fwd_masked=lin * ms_f, bwd=back, bwd_masked=back * ms_b)
    if extras:      # the statistics, pooled-output and sign-byte epilogues (every image selected)
      m, h, w, c = lin.shape
      outs.update(stats_y=lin, part_sum=np.stack([lin.sum(axis=(1, 2)), (lin * lin).sum(axis=(1, 2))], axis=1), pool_z=act,
                  zp=0.25 * _sum4(act), signs=sign_bytes(act), signs_zp=0.25 * _sum4(act))
    full = {}
    for name, v in outs.items():
      full[name] = np.zeros((inp['x'].shape[0],) + v.shape[1:])
      full[name][sel] = v
    return full
  return oracle


def _conv_bound(k, pad):
  def bound(inp, sets, d):
    """conv_bound with K = k k cin (+ 2: bias, slope) forward and k k cout backward (+ 1: the mask), and the second storage
    rounding of a masked element (tests/test_gpu_ops.py _twice) -- on the selected images; 1 elsewhere (never read)."""
    sel, lmag, bmag, ms_f, ms_b = _conv_terms(inp, k, pad, absolute=True)
    KF, KB = k * k * inp['x'].shape[3], k * k * inp['gy'].shape[3]
    u = E.unit_roundoff(d)
    twice = lambda ref, slope: (1 + u) * (u * np.abs(ref) + E.tiny(d)) * (slope != 1.0)
    r = {name: np.nan_to_num(s.ref[sel], nan=0.0, posinf=0.0, neginf=0.0) for name, s in sets.items()}
    lmag, bmag = (np.nan_to_num(m, nan=0.0, posinf=0.0, neginf=0.0) for m in (lmag, bmag))
    part = dict(fwd=E.conv_bound(r['fwd'], lmag + np.abs(_conv_bias(inp, sel)), KF + 2, d),
                fwd_masked=E.conv_bound(r['fwd_masked'], lmag * ms_f, KF + 1, d, twice(r['fwd_masked'], ms_f)),
                bwd=E.conv_bound(r['bwd'], bmag, KB, d),
                bwd_masked=E.conv_bound(r['bwd_masked'], bmag * ms_b, KB + 1, d, twice(r['bwd_masked'], ms_b)))
    full = {}
    for name in sets:
      full[name] = np.ones(sets[name].ref.shape)
      if name in part:
        full[name][sel] = part[name]
    return full
  return bound


def _conv_plants(hw, cin, cout, n, k):
  def plants(inp, d):
    i = interior_pixel(hw, hw, max(k, 3))
    ho = inp['gy'].shape[1]
    return [('x', (1,) + i + (cin - 1,)), ('x', (n - 1,) + last_pixel(hw, hw) + (0,)),
            ('gy', (1,) + corner_pixel(ho, ho) + (0,)), ('gy', (n - 1,) + border_pixel(ho, ho) + (cout - 1,))]
  return plants


for _name, _k, _pad, _hw, _cin, _cout, _n, _sym in CONV_SHAPES:
  _add('conv', _name, ('bf16', 'f16'), ('nan',) if _hw > 8 else SPECIALS, _conv_make(_k, _hw, _cin, _cout, _n), _conv_plants(_hw, _cin, _cout, _n, _k),
       _conv_oracle(_k, _pad), bound=_conv_bound(_k, _pad), par=dict(k=_k, pad=_pad, symbol=_sym, f32_inputs=('w', 'b')),
       fast=_name.startswith('small_k1'))

# two weight sets in one call (a stacked kernel and bias): the plants sit in the first half of the batch, the second half
# -- the other set's images -- keeps its bits
def _grouped_make(d):
  inp = _conv_make(3, 8, 32, 32, 4)(d)
  rng = np.random.RandomState(61)
  inp['w'] = storage_round(rng.randn(2, 3, 3, 32, 32) / 17.0, d)
  inp['b'] = storage_round(0.1 * rng.randn(2, 32), 'f32')
  return inp


_add('conv', 'grouped_k3_hw8_c32_n4', ('bf16', 'f16'), SPECIALS, _grouped_make,
     lambda inp, d: [('x', (1, 4, 4, 31)), ('x', (0, 7, 7, 0)), ('gy', (1, 0, 0, 0)), ('gy', (0, 0, 4, 31))],
     _conv_oracle(3, 'SAME'), bound=_conv_bound(3, 'SAME'), par=dict(k=3, pad='SAME', symbol='conv_img_kernel<', sets=True, f32_inputs=('w', 'b')))
# the statistics, pooled-output and sign-byte epilogues of the block ends: partials of a tainted (image, channel) are
# non-finite, all others keep their bits; the sign bytes of clean pixels are unchanged
_add('conv', 'epilogues_k3_hw16_c32_n3', ('bf16', 'f16'), SPECIALS, _conv_make(3, 16, 32, 32, 3), _conv_plants(16, 32, 32, 3, 3),
     _conv_oracle(3, 'SAME', extras=True), storage=dict(part_sum='f32', signs='f32'), bound=_conv_bound(3, 'SAME'),
     par=dict(k=3, pad='SAME', symbol='conv_', extras=True, f32_inputs=('w', 'b')))


# fp16 alone: two 60000s, in neighbouring pixels of one channel, under a 3x3 kernel of ones: every window that holds both is
# past 65504 and must be stored as Inf, a window that holds one stays finite (touched)
# a non-finite in the bias: its output channel in every image (the unit of this case is the channel); three images, all selected
_add('conv', 'bias_k3_hw8_c32_n3', ('bf16', 'f16'), SPECIALS, _conv_make(3, 8, 32, 32, 3), lambda inp, d: [('b', (31,))],
     _conv_oracle(3, 'SAME'), units=dict(fwd=3, fwd_masked=3, bwd=3, bwd_masked=3), bound=_conv_bound(3, 'SAME'),
     par=dict(k=3, pad='SAME', symbol='conv_img_kernel<', f32_inputs=('w', 'b')))
_add('conv', 'big_ones_k3_hw8_n4', ('f16',), ('big',), _conv_make(3, 8, 32, 32, 4, ones=True),
     lambda inp, d: [('x', (1, 3, 3, 5)), ('x', (1, 3, 4, 5)), ('gy', (3, 6, 6, 31)), ('gy', (3, 7, 6, 31))],
     _conv_oracle(3, 'SAME'), bound=_conv_bound(3, 'SAME'), par=dict(k=3, pad='SAME', symbol='conv_img_kernel<8,', f32_inputs=('w', 'b')))


NORM_GRADS = ('ggamma', 'gbeta', 'ggamma2', 'gbeta2')
for _name, _layer, _pn, _pool, _split in NORM_VARIANTS:
  for _tensor, _image in (('y', last_image(NORM_N)), ('gz', 0)):
    _add('norm_act', '%s-%s' % (_name, _tensor), DNAMES, SPECIALS if _name == 'instance_pn' else ('nan',), _norm_make(_pool), _norm_plants(_tensor, _image),
         _norm_oracle(_layer, _pn, _pool, _split), storage={k: 'f32' for k in NORM_GRADS}, bound=_norm_bound(_layer, _pn, _pool, _split),
         atomic=NORM_GRADS, par=dict(layer=_layer, pn=_pn, pool=_pool, split=_split), fast=_name in ('instance_pn', 'layer_split1'))

# per-image parameter rows (batch renorm: the caller's statistics) and the cross-replica route with one replica
for _name, _par in (('rows_pn', dict(rows=True)), ('one_replica_pn', dict(replicas=True))):
  for _tensor, _image in (('y', last_image(NORM_N)), ('gz', 0)):
    _add('norm_act', '%s-%s' % (_name, _tensor), DNAMES, ('nan',), _norm_make(False, None, 'rows' in _par), _norm_plants(_tensor, _image),
         _norm_oracle(False, True, False, None), storage={k: 'f32' for k in NORM_GRADS}, units=dict(ggamma=1, gbeta=1) if 'rows' in _par else None,
         bound=_norm_bound(False, True, False, None), atomic=NORM_GRADS, par=dict(layer=False, pn=True, pool=False, split=None, **_par),
         fast=_tensor == 'gz')

# 33 images of 64 x 64: pass 1 walks blocks of 128 pixels, the streaming passes blocks of 66 -- plants on both sides of BOTH edges
NORM_BIG = (33, 64, 64, 8)
for _tensor, _image in (('y', 32), ('gz', 0)):
  _add('norm_act', 'instance_pn_two_edges-%s' % _tensor, DNAMES, ('nan',), _norm_make(False, NORM_BIG), _norm_plants(_tensor, _image, NORM_BIG),
       _norm_oracle(False, True, False, None), storage={k: 'f32' for k in NORM_GRADS}, bound=_norm_bound(False, True, False, None),
       atomic=NORM_GRADS, par=dict(layer=False, pn=True, pool=False, split=None))


# ---- filter gradients (csrc/conv_wgrad_tile.hip, conv_mfma.hip): the paired launch into a sink that holds finite values
# (accumulate = 1), the smallest paired launch of each kernel (tests/test_gpu_wgrad_split.py PLANT_CASES), and the single
# launch with the bias gradient riding along.  x is planted in the LAST image of the second segment (its last pixel-split
# slice, one pixel in from the corner), gy at an interior pixel of the first segment's last image.  The slabs meet in atomics / a split reduction: bound route.
WGRAD_CASES = [      # name, n, nb, h, w, cin, cout, symbol
    ('pair', 1, 3, 8, 8, 32, 32, 'conv_wgrad_tile_kernel'), ('tile4', 1, 1, 24, 16, 32, 32, 'conv_wgrad_tile_kernel'),
    ('tile8', 1, 1, 16, 32, 32, 32, 'conv_wgrad_tile_kernel<8 waves>'), ('quad', 2, 1, 8, 16, 128, 64, 'conv_wgrad_quad_kernel'),
    ('thin', 1, 1, 64, 32, 16, 16, 'conv_wgrad_thin_kernel<16>'),
    ('single_bias_tile8', 5, 0, 16, 32, 24, 40, 'conv_wgrad_tile_kernel<8 waves>'), ('single_bias_mfma_k3_12x12', 3, 0, 12, 12, 32, 32, 'conv_wgrad_mfma<3,3>')]


def _wgrad_make(n, nb, h, w, cin, cout):
  def make(d):
    rng = np.random.RandomState(80 + h + cin)
    inp = dict(xa=storage_round(rng.randn(n, h, w, cin), d), ga=storage_round(rng.randn(n, h, w, cout), d),
               sink=storage_round(rng.randint(-8, 9, (3, 3, cin, cout)), 'f32'))
    if nb:
      inp.update(xb=storage_round(rng.randn(nb, h, w, cin), d), gb=storage_round(rng.randn(nb, h, w, cout), d))
    return inp
  return make


def _wgrad_sum(inp, f=lambda a: a):
  gw = N.conv2d_bwd_weight_gemm(f(inp['xa']), f(inp['ga']), (3, 3))
  bias = f(inp['ga']).sum(axis=(0, 1, 2))
  if 'xb' in inp:
    gw = gw + N.conv2d_bwd_weight_gemm(f(inp['xb']), f(inp['gb']), (3, 3))
    bias = bias + f(inp['gb']).sum(axis=(0, 1, 2))
  return gw, bias


def _wgrad_oracle(inp):
  gw, bias = _wgrad_sum(inp)
  out = dict(gw=inp['sink'] + gw)
  if 'xb' not in inp:
    out['gbias'] = bias
  return out


def _wgrad_bound(inp, sets, d):
  """wgrad_bound over P = (n + nb) h w pixels; into the sink one more fp32 rounding (tests/test_gpu_wgrad_split.py):
  (1 + 2^-24) B + 2^-24 (|sink| + |ref|)."""
  with np.errstate(all='ignore'):
    gw, bias = _wgrad_sum(inp)
    mw, mb = _wgrad_sum(inp, np.abs)
  P = sum(inp[k].shape[0] for k in ('xa', 'xb') if k in inp) * inp['xa'].shape[1] * inp['xa'].shape[2]
  z = lambda a: np.nan_to_num(a, nan=0.0, posinf=0.0, neginf=0.0)
  B = E.wgrad_bound(z(gw), z(mw), P)
  out = dict(gw=(1 + E.U32) * B + E.U32 * (np.abs(inp['sink']) + np.abs(z(gw))))
  if 'xb' not in inp:
    out['gbias'] = E.wgrad_bound(z(bias), z(mb), P)
  return out


for _name, _n, _nb, _h, _w, _cin, _cout, _sym in WGRAD_CASES:
  for _which in ('x', 'gy'):      # one plant per case: x[.., ci0] taints gw[:, :, ci0, :], gy[.., co0] taints gw[:, :, :, co0] and gb[co0]
    _add('wgrad', '%s-%s' % (_name, _which), ('bf16', 'f16'), SPECIALS if _name == 'pair' else ('nan',), _wgrad_make(_n, _nb, _h, _w, _cin, _cout),
         (lambda n, nb, h, w, cin, cout, which: lambda inp, d:
          [('xb' if nb else 'xa', ((nb or n) - 1, h - 2, w - 2, cin - 1))] if which == 'x' else [('ga', (n - 1,) + interior_pixel(h, w) + (1,))])(
              _n, _nb, _h, _w, _cin, _cout, _which),
         _wgrad_oracle, storage=dict(gw='f32', gbias='f32'), units=dict(gw=2 if _which == 'x' else 3, gbias=0), bound=_wgrad_bound,
         atomic=('gw', 'gbias'), par=dict(symbol=_sym, f32_inputs=('sink',)), fast=_name in ('pair', 'single_bias_mfma_k3_12x12'))

# the same launches in deterministic mode: the slab reduction is ordered, the launch bit-reproducible, and containment is
# bit-equality with the unplanted launch (sink + clean gradient included)
for _name, _n, _nb, _h, _w, _cin, _cout, _sym in WGRAD_CASES:
  if _name in ('pair', 'thin', 'tile8', 'single_bias_tile8'):
    _add('wgrad', '%s-deterministic' % _name, ('bf16', 'f16'), ('nan',), _wgrad_make(_n, _nb, _h, _w, _cin, _cout),
         (lambda n, nb, h, w, cin: lambda inp, d: [('xb' if nb else 'xa', ((nb or n) - 1, h - 2, w - 2, cin - 1))])(_n, _nb, _h, _w, _cin),
         _wgrad_oracle, storage=dict(gw='f32', gbias='f32'), units=dict(gw=2, gbias=0), par=dict(symbol=_sym, f32_inputs=('sink',), det=True),
         fast=_name == 'pair')


# ---- fromRGB / toRGB (csrc/pointwise.hip): bias, no activation (a mask from a computed sign has no place here).  105 pixels:
# no multiple of a block's pixel count; the plants sit at the last pixel -- the one the clamped quad of the filter-gradient
# kernel re-reads -- and at pixel 0
def _pw_make(cin, cout):
  def make(d):
    rng = np.random.RandomState(90 + cin)
    return dict(x=storage_round(rng.randn(3, 7, 5, cin), d), gy=storage_round(rng.randn(3, 7, 5, cout), d),
                w=storage_round(rng.randn(cin, cout) / np.sqrt(cin), 'f32'), b=storage_round(0.1 * rng.randn(cout), 'f32'))
  return make


def _pw_oracle(inp):
  x, gy, w = inp['x'], inp['gy'], inp['w']
  out = dict(y=x @ w + inp['b'], gx=gy @ w.T, gw=np.einsum('nhwi,nhwo->io', x, gy), gb=gy.sum(axis=(0, 1, 2)))
  if w.shape[0] <= 4:      # the masked forward of the gradient penalty's second pass: gy is the mask source
    out['ym'] = (x @ w) * np.where(gy > 0, 1.0, ALPHA)
  return out


def _pw_bound(inp, sets, d):
  z = lambda a: np.nan_to_num(a, nan=0.0, posinf=0.0, neginf=0.0)
  x, gy, w = z(inp['x']), z(inp['gy']), inp['w']
  cin, cout = w.shape
  u = E.unit_roundoff(d)
  sl = np.where(inp['gy'] > 0, 1.0, ALPHA)
  ym = z(sets['ym'].ref) if 'ym' in sets else 0.0
  extra = dict(ym=E.conv_bound(ym, (np.abs(x) @ np.abs(w)) * sl, cin + 1, d, (1 + u) * (u * np.abs(ym) + E.tiny(d)))) if 'ym' in sets else {}
  return dict(extra, y=E.conv_bound(z(sets['y'].ref), np.abs(x) @ np.abs(w) + np.abs(inp['b']), cin + 1, d),
              gx=E.conv_bound(z(sets['gx'].ref), np.abs(gy) @ np.abs(w).T, cout, d),
              gw=E.wgrad_bound(z(sets['gw'].ref), np.einsum('nhwi,nhwo->io', np.abs(x), np.abs(gy)), 105),
              gb=E.wgrad_bound(z(sets['gb'].ref), np.abs(gy).sum(axis=(0, 1, 2)), 105))


for _cin, _cout in ((3, 16), (16, 3)):
  _add('pointwise', 'c%d_c%d' % (_cin, _cout), DNAMES, SPECIALS, _pw_make(_cin, _cout),
       (lambda ci, co: lambda inp, d: [('x', (2, 6, 4, ci - 1)), ('gy', (2, 6, 4, 0)), ('gy', (0, 0, 0, co - 1))])(_cin, _cout),
       _pw_oracle, storage=dict(gw='f32', gb='f32'), units=dict(gw=0 if _cin > 3 else 1), bound=_pw_bound, atomic=('gw', 'gb'),
       par=dict(f32_inputs=('w', 'b')), fast=True)
  # deterministic mode: the ordered filter / bias gradient, bit-equal to the unplanted launch
  _add('pointwise', 'c%d_c%d-deterministic' % (_cin, _cout), DNAMES, ('nan',), _pw_make(_cin, _cout),
       (lambda ci, co: lambda inp, d: [('x', (2, 6, 4, ci - 1)), ('gy', (2, 6, 4, 0)), ('gy', (0, 0, 0, co - 1))])(_cin, _cout),
       _pw_oracle, storage=dict(gw='f32', gb='f32'), units=dict(gw=0 if _cin > 3 else 1), bound=_pw_bound,
       par=dict(f32_inputs=('w', 'b'), det=True), fast=True)


# ---- concat-input conv (upcat_fwd / upcat_bwd_data): a plant in the low-resolution source taints its 2x2 footprint dilated by
# the kernel; one in the skip source its own 3x3 window.  Image 0 stays clean.
def _upcat_make(d):
  rng = np.random.RandomState(95)
  return dict(x0=storage_round(rng.randn(3, 8, 8, 32), d), x1=storage_round(rng.randn(3, 16, 16, 32), d),
              gy=storage_round(rng.randn(3, 16, 16, 16), d), w=storage_round(rng.randn(3, 3, 64, 16) / 24.0, d))


def _upcat_conv_oracle(inp):
  cat = np.concatenate([_up2(inp['x0']), inp['x1']], axis=3)
  back = N.conv2d_bwd_data_gemm(inp['gy'], inp['w'], (16, 16), 'SAME')
  y = N.conv2d_gemm(cat, inp['w'], 'SAME')
  return dict(y=y, g0=_sum4(back[..., :32]), g1=back[..., 32:], gw=N.conv2d_bwd_weight_gemm(cat, inp['gy'], (3, 3)),
              stats_y=y, part_sum=np.stack([y.sum(axis=(1, 2)), (y * y).sum(axis=(1, 2))], axis=1))


def _upcat_bound(inp, sets, d):
  z = lambda a: np.nan_to_num(a, nan=0.0, posinf=0.0, neginf=0.0)
  cat = np.concatenate([_up2(inp['x0']), inp['x1']], axis=3)
  with np.errstate(all='ignore'):
    mag = N.conv2d_bwd_weight_gemm(np.abs(cat), np.abs(inp['gy']), (3, 3))
  out = {k: np.ones(s.ref.shape) for k, s in sets.items()}
  out['gw'] = E.wgrad_bound(z(sets['gw'].ref), z(mag), 3 * 256)
  return out


for _perm in (False, True):
  _add('upcat_conv', 'perm' if _perm else 'plain', ('bf16', 'f16'), ('nan',), _upcat_make,
       lambda inp, d: [('x0', (1, 3, 3, 31)), ('x1', (2, 14, 14, 0)), ('gy', (1, 8, 8, 15))], _upcat_conv_oracle,
       storage=dict(gw='f32', part_sum='f32'), bound=_upcat_bound, atomic=('gw',), par=dict(perm=_perm, f32_inputs=('w',)))


# ---- minibatch stddev (csrc/reduce.hip): a plant taints the statistic (and the gradient) of its group only
MB = (6, 3, 8)      # images, groups, channels


def _mbstd_refs(inp, d, dt):
  import torch
  t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
  n, groups, c = MB
  r = E.mbstd_reference(t(inp['x']), t(inp['go']), t(inp['v']), groups, 1e-8 if d == 'f32' else 1e-6, dt)
  return dict(out=r[0], gx=r[1], ggo=r[2], gx2=r[3])


def _mbstd_case(d_fixed):
  import torch
  return dict(oracle=lambda inp: {k: np.asarray(v, np.float64) for k, v in _mbstd_refs(inp, d_fixed, torch.float64).items()})


for _d in DNAMES:      # eps depends on the storage type: one case per type
  _add('mbstd', 'group_of_the_plant_' + _d, (_d,), SPECIALS,
       lambda d: dict(x=_rand((MB[0], 4, 4, MB[2]), d, 96), go=_rand((MB[0], 4, 4, MB[2] + 1), d, 97), v=_rand((MB[0], 4, 4, MB[2]), d, 129)),
       lambda inp, d: [('x', (2, 3, 3, MB[2] - 1))], _mbstd_case(_d)['oracle'], fast=_d == 'bf16')


# ---- tanh, dot, fully connected, cosine distance, channel sums, rows
_add('tanh', 'nan', DNAMES, ('nan',), lambda d: dict(x=_rand(ABS_SHAPE, d, 98), gy=_rand(ABS_SHAPE, d, 99)), _edges(ABS_SHAPE, 'x'),
     lambda inp: dict(y=np.tanh(inp['x'])), fast=True)
# tg_tanh_bwd and tg_mul3 (the tanh backward's own backward) on stored operands: g (1 - y^2) and -2 y g v
_add('tanh_bwd_mul3', 'operands', DNAMES, SPECIALS,
     lambda d: dict(y=storage_round(np.tanh(np.random.RandomState(98).randn(*ABS_SHAPE)), d), g=_rand(ABS_SHAPE, d, 99), v=_rand(ABS_SHAPE, d, 128)),
     lambda inp, d: [('g', first(ABS_SHAPE)), ('v', behind_last_vector(ABS_SHAPE, d)), ('y', last(ABS_SHAPE))],
     lambda inp: dict(gx=inp['g'] * (1.0 - inp['y'] ** 2), gy=-2.0 * inp['y'] * inp['g'] * inp['v']), fast=True)
_add('dot', 'one_nan', DNAMES, SPECIALS, lambda d: dict(a=_rand((3, 4099), d, 100), b=_rand((3, 4099), d, 101)),
     lambda inp, d: [('a', (1, 4098))], lambda inp: dict(out=(inp['a'] * inp['b']).sum(axis=1), ga=1.5 * inp['b'], gb=1.5 * inp['a']),
     storage=dict(out='f32'), fast=True)
FC = (6, 3, 40)      # rows, outputs, inputs


def _fc_oracle(inp):
  x, w, g = inp['x'], inp['w'], inp['g']
  return dict(y=x @ w + inp['b'], gx=g @ w.T, gw=x.T @ g, gb=g.sum(axis=0))


_add('fully_connected', 'row', DNAMES, SPECIALS,
     lambda d: dict(x=_rand((FC[0], FC[2]), d, 102), w=_rand((FC[2], FC[1]), 'f32', 103, 0.2), b=_rand((FC[1],), 'f32', 104), g=_rand((FC[0], FC[1]), 'f32', 105)),
     lambda inp, d: [('x', (FC[0] - 1, FC[2] - 1)), ('g', (1, 2))], _fc_oracle, storage=dict(y='f32', gw='f32', gb='f32'),
     par=dict(f32_inputs=('w', 'b', 'g')), fast=True)


def _cosine_oracle(inp):
  import torch
  t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
  r = E.cosine_formulas(t(inp['e']), t(inp['p']), 0.7, 1.5, torch.float64)
  rows = np.array([E.cosine_formulas(t(inp['e'][b:b + 1]), t(inp['p'][b:b + 1]), 0.7, 1.5, torch.float64)['out'] for b in range(inp['e'].shape[0])])
  return dict(rows=rows, gp=r['gp'])


# the loss of each row as a launch of its own (the scalar of the whole batch would be all taint), the gradient of the batch
_add('cosine_distance', 'row', ('f32',), SPECIALS, lambda d: dict(e=_rand((4, 257), 'f32', 106), p=_rand((4, 257), 'f32', 107)),
     lambda inp, d: [('p', (3, 256))], _cosine_oracle, storage=dict(rows='f32', gp='f32'), fast=True)


def _csum_bound(inp, sets, d):
  g = np.nan_to_num(inp['g'], nan=0.0, posinf=0.0, neginf=0.0).reshape(-1, inp['g'].shape[3])
  b = E.wgrad_bound(g.sum(axis=0), np.abs(g).sum(axis=0), g.shape[0])
  return dict(atomic=b, ordered=b)


_add('channel_sum', 'atomic_and_ordered', DNAMES, SPECIALS, lambda d: dict(g=_rand(ST_SHAPE, d, 108)),
     lambda inp, d: [('g', last(ST_SHAPE)), ('g', (0, 0, 0, 1))],
     lambda inp: dict(atomic=inp['g'].reshape(-1, 5).sum(axis=0), ordered=inp['g'].reshape(-1, 5).sum(axis=0)),
     storage=dict(atomic='f32', ordered='f32'), bound=_csum_bound, atomic=('atomic',), fast=True)
_add('cat_rows', 'copy', DNAMES, SPECIALS, lambda d: dict(a=_rand((2, 3, 5), d, 109), b=_rand((3, 3, 5), d, 110)),
     lambda inp, d: [('a', (1, 2, 4)), ('b', (2, 2, 4))], lambda inp: dict(out=np.concatenate([inp['a'], inp['b']], axis=0)), fast=True)
_add('lrelu_bwd_bias', 'c5', DNAMES, SPECIALS, lambda d: dict(g=_rand(ST_SHAPE, d, 111), z=_rand(ST_SHAPE, d, 112)),
     lambda inp, d: [('g', last(ST_SHAPE))],
     lambda inp: dict(out=_lrelu_oracle(inp)['out'], gb=_lrelu_oracle(inp)['out'].reshape(-1, 5).sum(axis=0)), storage=dict(gb='f32'),
     bound=lambda inp, sets, d: dict(out=E.conv_bound(np.nan_to_num(sets['out'].ref), np.abs(np.nan_to_num(sets['out'].ref)), 1, d),
                                     gb=E.wgrad_bound(np.nan_to_num(sets['out'].ref).reshape(-1, 5).sum(axis=0),
                                                      np.abs(np.nan_to_num(sets['out'].ref)).reshape(-1, 5).sum(axis=0), 180)
                                     + E.conv_bound(np.nan_to_num(sets['out'].ref), np.abs(np.nan_to_num(sets['out'].ref)), 1, d).reshape(-1, 5).sum(axis=0)),
     atomic=('gb',), fast=True)


# ---- spectral norm (csrc/sn.hip): three kernels, each a launch of its own; a plant in one kernel's w taints that kernel alone
def _sn_oracle(inp):
  import torch
  t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
  rs = [E.sn_formulas(t(inp['w'][i]), t(inp['u'][i]), t(np.ones_like(inp['w'][i])), torch.float64) for i in range(3)]
  return dict(w_bar=np.stack([r['w_bar'] for r in rs]), u_new=np.stack([r['u_new'] for r in rs]), gw=np.stack([r['gw'] for r in rs]))


_add('spectral_norm', 'one_kernel_of_three', ('f32',), SPECIALS, lambda d: dict(w=_rand((3, 72, 16), 'f32', 113, 0.1), u=_rand((3, 16), 'f32', 114)),
     lambda inp, d: [('w', (1, 71, 15))], _sn_oracle, storage=dict(w_bar='f32', u_new='f32', gw='f32'), fast=True)

def _sn_multi_oracle(inp):
  import torch
  t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
  rs = [E.sn_formulas(t(inp['w'][i]), t(inp['u'][i]), t(np.ones_like(inp['w'][i])), torch.float64) for i in range(inp['w'].shape[0])]
  return dict(w_bar=np.stack([r['w_bar'] for r in rs]), u_new=np.stack([r['u_new'] for r in rs]))


# the multi-kernel launch: 33 jobs in one table, one planted; the other 32 keep their bits
_add('spectral_norm_multi', 'job_17_of_33', ('f32',), SPECIALS, lambda d: dict(w=_rand((33, 24, 16), 'f32', 116, 0.1), u=_rand((33, 16), 'f32', 117)),
     lambda inp, d: [('w', (17, 23, 15))], _sn_multi_oracle, storage=dict(w_bar='f32', u_new='f32'), fast=True)


# ---- flash attention (csrc/flash.hip): a plant in a query row taints that row of O and of dQ (and, through the sums over
# queries, dK and dV of its batch entry); a plant in a key row every row of its batch entry; no other batch entry
FLASH = (3, 256, 8, 64)


def _flash_oracle(inp):
  q, k, v, go = inp['q'], inp['k'], inp['v'], inp['go']
  o, _ = N.attention_forward(q, k, v)
  dq, dk, dv = N.attention_backward(q, k, v, go)
  s_ = np.einsum('nid,njd->nij', q, k)
  m = s_.max(-1)
  lse = m + np.log(np.exp(s_ - m[..., None]).sum(-1))
  return dict(o=o, lse=lse, dq=dq, dk=dk, dv=dv)


def _flash_make(d):
  n, ln, dk, dv = FLASH
  rng = np.random.RandomState(115)
  return dict(q=storage_round(np.tanh(rng.randn(n, ln, dk)), d), k=storage_round(np.tanh(rng.randn(n, ln, dk) * 2), d),
              v=storage_round(rng.randn(n, ln, dv), d), go=storage_round(rng.randn(n, ln, dv), d))


_add('flash_attention', 'query_row', ('bf16', 'f16'), ('nan', '+inf'), _flash_make, lambda inp, d: [('q', (2, 255, 7))], _flash_oracle, storage=dict(lse='f32'))
_add('flash_attention', 'key_row', ('bf16', 'f16'), ('nan',), _flash_make, lambda inp, d: [('k', (1, 100, 0))], _flash_oracle, storage=dict(lse='f32'))
_add('flash_attention', 'value_row', ('bf16', 'f16'), ('nan',), _flash_make, lambda inp, d: [('v', (1, 255, 63))], _flash_oracle, storage=dict(lse='f32'))


# ---- small GEMM (fp32, csrc/reduce.hip tg_small_gemm) forward and both gradients, plain and with both operands transposed;
# scale_dev (x times a device scalar: three launches, one scalar planted); the second-order softmax kernel
_add('small_gemm', 'row_and_column', ('f32',), SPECIALS,
     lambda d: dict(a=_rand((5, 31), 'f32', 120), b=_rand((31, 3), 'f32', 121), g=_rand((5, 3), 'f32', 122)),
     lambda inp, d: [('a', (4, 30)), ('b', (0, 2))],
     lambda inp: dict(c=inp['a'] @ inp['b'], ga=inp['g'] @ inp['b'].T, gb=inp['a'].T @ inp['g'], ctt=inp['a'] @ inp['b']),
     storage=dict(c='f32', ga='f32', gb='f32', ctt='f32'), fast=True)
_add('scale_dev', 'scalar', DNAMES, SPECIALS, lambda d: dict(x=_rand((3, 315), d, 123), s=_rand((3,), 'f32', 124)),
     lambda inp, d: [('s', (1,))], lambda inp: dict(out=inp['x'] * inp['s'][:, None]), par=dict(f32_inputs=('s',)), fast=True)
_add('softmax_bwd_bwd', 'row', DNAMES, ('nan', '+inf'),
     lambda d: dict(p=storage_round(_softmax_fwd(np.random.RandomState(125).randn(*SM_SHAPE)), d), dp=_rand(SM_SHAPE, d, 126), v=_rand(SM_SHAPE, d, 127)),
     lambda inp, d: [('v', (2, 99)), ('dp', (5, 0))],
     lambda inp: dict(gp=inp['v'] * (inp['dp'] - (inp['dp'] * inp['p']).sum(-1, keepdims=True)) - inp['dp'] * (inp['v'] * inp['p']).sum(-1, keepdims=True)),
     fast=True)


# ---- flash attention, second order (the gradient penalty's pattern: the backward of the create_graph backward).  A plant in
# one cotangent row of dQ stays inside its batch entry
def _flash2_oracle(inp):
  r = N.attention_backward_backward(*(inp[k] for k in ('q', 'k', 'v', 'go', 'aq', 'ak', 'av')))
  return dict(adj_q=r[0], adj_k=r[1], adj_v=r[2], adj_go=r[3])


def _flash2_make(d):
  inp = _flash_make(d)
  n, ln, dk, dv = FLASH
  rng = np.random.RandomState(130)
  inp.update(aq=storage_round(rng.randn(n, ln, dk), d), ak=storage_round(rng.randn(n, ln, dk), d), av=storage_round(rng.randn(n, ln, dv), d))
  return inp


_add('flash_second_order', 'cotangent_row', ('bf16', 'f16'), ('nan',), _flash2_make, lambda inp, d: [('aq', (2, 255, 7))], _flash2_oracle,
     par=dict(f32_inputs=('aq', 'ak', 'av')))


# ---- the backward-data that unpools (conv_bwd_data_unpool: sign bytes and the pooled gradient in, the producer's mask in the
# epilogue).  The plants sit in the pooled gradient alone: its 2x2 block of the kept gradient, the window around it of gx
def _unpool_oracle(inp):
  x, w = inp['x'], inp['w']
  pre = N.conv2d_gemm(x, w, 'SAME') + inp['b']
  g2 = 0.25 * _up2(inp['gzp']) * np.where(pre > 0, 1.0, ALPHA)
  return dict(kept=g2, gx=N.conv2d_bwd_data_gemm(g2, w, x.shape[1:3], 'SAME') * np.where(x > 0, 1.0, ALPHA))


def _unpool_make(d):
  inp = _conv_make(3, 16, 32, 32, 3)(d)
  inp['gzp'] = _rand((3, 8, 8, 32), d, 131)
  del inp['gy']
  return inp


_add('unpool', 'k3_hw16_c32_n3', ('bf16', 'f16'), SPECIALS, _unpool_make, lambda inp, d: [('gzp', (1, 3, 3, 5)), ('gzp', (2, 7, 7, 31))],
     _unpool_oracle, par=dict(f32_inputs=('w', 'b')))


# ---- the normaliser fed by the conv's statistics epilogue (conv2d_stats -> norm_act(conv_stats=)): a plant in the conv's input
# taints its window of y in every channel, and with it the whole image of z and gy; the other images keep their bits
def _ncs_oracle(inp):
  y = N.conv2d_gemm(inp['x'], inp['w'], 'SAME')
  r = _norm_refs(dict(inp, y=y), False, True, False, None, __import__('torch').float64)
  return dict(y=y, z=r['z'], gy=r['gy'])


_add('norm_conv_stats', 'k3_hw16_c16_n3', ('bf16', 'f16'), ('nan',),
     lambda d: dict(_norm_make(False, (3, 16, 16, 16))(d), x=_rand((3, 16, 16, 16), d, 132), w=storage_round(np.random.RandomState(133).randn(3, 3, 16, 16) / 12.0, d)),
     lambda inp, d: [('x', (1, 8, 8, 3))], _ncs_oracle, par=dict(f32_inputs=('w',)))


# ---- rows (tg_rows_assemble): a range as a view, several ranges one after the other as a new tensor; a copy either way
_add('rows', 'ranges', DNAMES, SPECIALS, lambda d: dict(x=_rand((5, 3, 5), d, 134)), lambda inp, d: [('x', (3, 2, 4))],
     lambda inp: dict(head=inp['x'][0:2].copy(), picked=np.concatenate([inp['x'][1:2], inp['x'][3:5]])), fast=True)
