"""Guard bands and poison round the tensors a wrapper allocates and the tensors it is given (a test helper, not a conftest).

``Guarded(device)`` is a TorchFunctionMode.  While it is active every tensor factory call made from twingan_amd/ops.py
(``empty``, ``empty_like``, ``zeros``, ``zeros_like``, ``ones``, ``full``, the ``new_*`` forms) for the test device is served
from a buffer of its own:

    [ front guard, 0xA5 bytes ][ the tensor, base 256-byte aligned ][ rear guard, 0xA5 bytes, from the tensor's last byte + 1 ]

The interior of an ``empty*`` result is filled with 0xFF bytes -- a NaN in fp32, bf16 and fp16 -- so that an element the kernel
never writes, and a value computed from one, is not finite; ``zeros*`` / ``ones`` / ``full`` keep their value.  The buffers live
until the mode is dropped, so no allocation is handed the block that a previous call just filled with the right answer.
``damage()`` returns, per allocation, the offsets of the guard bytes that changed, with the call site and the shape, and says
whether they lie before or after the tensor.

``guarded_input(t)`` gives a copy of ``t`` with 0xFF bytes (NaN again) directly before and after it and a pristine clone of the
whole buffer: a read past either end that reaches the result makes it non-finite, a write to the input or its surrounds shows
in ``intact()``.

The guard on each side is at least 64 KiB and at least the bytes of one image of a 4-d tensor, capped at 1 MiB.  LIMITS: a
store further from the tensor than that goes unseen; so does a read outside a tensor whose value is discarded, and a read that
stays inside the caching allocator's block is no fault on the device either way (the sanitized driver of
tests/test_bounds_cpu.py sees those, on the CPU).
"""
import os
import sys

import torch
from torch.overrides import TorchFunctionMode

GUARD_BYTE = 0xA5
POISON_BYTE = 0xFF
MIN_GUARD = 64 << 10
MAX_GUARD = 1 << 20
ALIGN = 256

_EMPTY = {torch.empty, torch.empty_like, torch.Tensor.new_empty}
_VALUED = {torch.zeros, torch.zeros_like, torch.ones, torch.ones_like, torch.full, torch.full_like, torch.Tensor.new_zeros,
           torch.Tensor.new_ones, torch.Tensor.new_full}
_HERE = os.path.abspath(__file__)


def guard_bytes(shape, itemsize):
  """Per side: >= 64 KiB and >= one image of a 4-d tensor, <= 1 MiB, a multiple of the alignment."""
  g = MIN_GUARD
  if len(shape) == 4:
    image = itemsize
    for d in shape[1:]:
      image *= int(d)
    g = max(g, image)
  g = min(g, MAX_GUARD)
  return (g + ALIGN - 1) // ALIGN * ALIGN


def _banded(nbytes, guard, device, band_byte):
  """-> (uint8 buffer filled with band_byte, offset of a 256-byte aligned interior of nbytes)."""
  raw = torch.empty(2 * guard + nbytes + ALIGN, dtype=torch.uint8, device=device)
  shift = (-raw.data_ptr()) % ALIGN
  buf = raw[shift:shift + 2 * guard + nbytes]
  buf.fill_(band_byte)
  return buf, guard


def _changed(region, byte):
  """Offsets (up to 8, and the count) of the bytes of a uint8 region that differ from `byte`."""
  bad = (region != byte).nonzero().flatten()
  return [int(i) for i in bad[:8]], int(bad.numel())


class _Alloc:
  def __init__(self, buf, off, nbytes, site, shape, dtype):
    self.buf, self.off, self.nbytes, self.site, self.shape, self.dtype = buf, off, nbytes, site, shape, dtype


class Guarded(TorchFunctionMode):
  def __init__(self, device, files=(os.path.join('twingan_amd', 'ops.py'),)):
    super().__init__()
    self.device = torch.device(device)
    self.files = tuple(files)
    self.allocs = []

  def _site(self):
    """The nearest caller that is one of the watched files, as 'file:line in function' (None: somebody else's call)."""
    f = sys._getframe(2)
    while f is not None:
      name = f.f_code.co_filename
      if name != _HERE and os.sep + 'torch' + os.sep not in name:
        if name.endswith(self.files):
          return '%s:%d in %s' % (os.path.basename(name), f.f_lineno, f.f_code.co_name)
        return None
      f = f.f_back
    return None

  def __torch_function__(self, func, types, args=(), kwargs=None):
    kwargs = kwargs or {}
    if func not in _EMPTY and func not in _VALUED:
      return func(*args, **kwargs)
    site = self._site()
    proto = func(*args, **kwargs)      # torch's own reading of the arguments: shape, dtype, device, value
    if site is None or not isinstance(proto, torch.Tensor) or proto.device.type != self.device.type or proto.numel() == 0 or \
        not proto.is_contiguous() or proto.requires_grad:
      return proto
    nbytes = proto.numel() * proto.element_size()
    guard = guard_bytes(tuple(proto.shape), proto.element_size())
    buf, off = _banded(nbytes, guard, proto.device, GUARD_BYTE)
    inner = buf[off:off + nbytes]
    if func in _EMPTY:
      inner.fill_(POISON_BYTE)
    else:
      inner.copy_(proto.view(-1).view(torch.uint8))
    self.allocs.append(_Alloc(buf, off, nbytes, site, tuple(proto.shape), proto.dtype))
    return inner.view(proto.dtype).view(proto.shape)

  def damage(self):
    """-> list of reports, one per allocation with a changed guard byte (empty: every guard is intact)."""
    out = []
    for i, a in enumerate(self.allocs):
      for side, region, base in (('before', a.buf[:a.off], -a.off), ('after', a.buf[a.off + a.nbytes:], 0)):
        where, count = _changed(region, GUARD_BYTE)
        if count:
          out.append(dict(index=i, site=a.site, shape=a.shape, dtype=a.dtype, side=side, count=count,
                          offsets=[base + w for w in where],
                          text='allocation %d (%s %s at %s): %d guard byte(s) written %s the tensor, first at byte %+d from its %s'
                               % (i, tuple(a.shape), a.dtype, a.site, count, side, base + where[0], 'start' if side == 'before' else 'end')))
    return out


class GuardedInput:
  def __init__(self, t, name=''):
    t = t.detach().contiguous()
    self.name = name
    self.nbytes = t.numel() * t.element_size()
    guard = guard_bytes(tuple(t.shape), t.element_size())
    self.buf, self.off = _banded(self.nbytes, guard, t.device, POISON_BYTE)
    self.buf[self.off:self.off + self.nbytes].copy_(t.view(-1).view(torch.uint8))
    self.t = self.buf[self.off:self.off + self.nbytes].view(t.dtype).view(t.shape)
    self.pristine = self.buf.clone()

  def intact(self, interior=True):
    """None when the tensor (unless interior=False: an in/out operand) and its surrounds are byte-equal to the pristine clone,
    else a message that says where they are not."""
    lo, hi = self.off, self.off + self.nbytes
    for side, sl, base in (('before', slice(0, lo), -lo), ('inside', slice(lo, hi), 0), ('after', slice(hi, None), 0)):
      if side == 'inside' and not interior:
        continue
      bad = (self.buf[sl] != self.pristine[sl]).nonzero().flatten()
      if bad.numel():
        return 'input %s %s: %d byte(s) written %s the tensor, first at byte %+d' % (self.name, tuple(self.t.shape), int(bad.numel()),
                                                                                  side, base + int(bad[0]))
    return None


def guarded_input(t, name=''):
  return GuardedInput(t, name)


def flatten(out):
  """The tensors of a (nested) result, in order."""
  if isinstance(out, torch.Tensor):
    return [out]
  if isinstance(out, (tuple, list)):
    return [t for o in out for t in flatten(o)]
  if hasattr(out, '__slots__'):      # small result records (ops.ConvStats)
    return [t for name in out.__slots__ for t in flatten(getattr(out, name, None))]
  return []


def check(run, inputs, device, inout=(), exact=True, finite=True, files=None, sync=None, ordinary=True, served=None):
  """Runs ``run(*inputs)`` the ordinary way (A, on clones of the in/out operands), then under the guarded allocator with
  guarded inputs (B), and asserts in this order: guards intact; inputs and their surrounds untouched (``inout``: indices of
  operands the call updates in place -- their surrounds only); B finite everywhere (outputs and in/out operands);
  ``torch.equal(A, B)`` when ``exact``.  ``ordinary=False`` skips run A (the harness's own test: its planted faults exist only
  inside guarded buffers).  ``served``: a list that receives the call site of every guarded allocation.  Returns (A, B)."""
  sync = sync or (lambda: None)
  a_in = [t.clone() if i in inout else t for i, t in enumerate(inputs)]
  A = run(*a_in) if ordinary else None
  sync()
  gin = [guarded_input(t, 'operand %d' % i) if isinstance(t, torch.Tensor) else None for i, t in enumerate(inputs)]
  g = Guarded(device, **({'files': files} if files else {}))
  with g:
    B = run(*[x.t if x is not None else t for x, t in zip(gin, inputs)])
  sync()
  if served is not None:
    served.extend(a.site for a in g.allocs)
  dmg = g.damage()
  assert not dmg, '\n'.join(d['text'] for d in dmg)
  for i, x in enumerate(gin):
    if x is not None:
      msg = x.intact(interior=i not in inout)
      assert msg is None, msg
  fb = flatten(B) + [gin[i].t for i in inout]
  fa = flatten(A) + [a_in[i] for i in inout] if ordinary else fb
  assert len(fa) == len(fb)
  for k, (ta, tb) in enumerate(zip(fa, fb)):
    if finite and tb.is_floating_point():
      ok = torch.isfinite(tb)
      assert bool(ok.all()), 'result %d %s: %d element(s) not finite under the guarded run (poison read, or never written), first at flat ' \
                             'index %d' % (k, tuple(tb.shape), int((~ok).sum()), int((~ok).flatten().nonzero()[0]))
    if exact and ordinary:
      assert torch.equal(ta, tb), 'result %d %s differs between the ordinary and the guarded run' % (k, tuple(tb.shape))
  return A, B
