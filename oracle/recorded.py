"""TEST INFRASTRUCTURE -- recorded runs of the reference's own code.

The tests that pin the oracle against the reference call ``oracle/ref_runner.py`` (the reference's graph code executed on
the TensorFlow stand-in).  What those calls returned is stored under ``tests/golden/reference/<name>.npz``, so the tests
need nothing outside the repository:

    with recorded('live_gan') as rec:
      ref = rec(ref_runner.run, flags, sources, targets, seed=1)

replays the results of the calls the recording holds, in order (``replay(name, fn, ...)``: a recording of one call).
Each recorded call carries a fingerprint of its arguments (structure and scalars exactly, every array by shape, dtype and
two weighted sums); a call whose arguments do not match the recording is an error, never a silent pass.  ``TG_RECORD_REFERENCE=1`` executes the calls instead (the
reference tree must be importable by oracle/tf_shim/loader.py) and rewrites the files.

A file is one .npz (no pickles): ``__meta__`` holds a JSON skeleton of every call (fingerprint and result), whose arrays
are the other members.
"""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden', 'reference')
RECORD = os.environ.get('TG_RECORD_REFERENCE') == '1'
# what ref_runner.run returns that no test reads (every intermediate tensor, the is_training=False images): not recorded
DROP = ('end_points', 'custom')


def own_gradients(res):
  """For the loss / gradient pins: the names of the variables the reference created (not their values, the preset), the
  generator loss's gradients of the non-discriminator variables and the discriminator loss's of the discriminators' --
  the pairs the tests compare; the cross terms (d generator loss / d discriminator weights, ...) are not recorded."""
  res = dict(res)
  res['variables'] = {k: None for k in res['variables']}
  res['g_grads'] = {k: v for k, v in res['g_grads'].items() if not k.startswith('discriminator')}
  res['d_grads'] = {k: v for k, v in res['d_grads'].items() if k.startswith('discriminator')}
  return res


def _numpy(x):
  if hasattr(x, 'detach') and hasattr(x, 'numpy'):      # torch tensor
    return x.detach().cpu().numpy()
  return x


def _fingerprint(x):
  """JSON-able summary of a call argument: exact for the structure and Python scalars, arrays by shape / dtype / sums."""
  x = _numpy(x)
  if isinstance(x, dict):
    return {'d': [[str(k), _fingerprint(v)] for k, v in sorted(x.items(), key=lambda kv: str(kv[0]))]}
  if isinstance(x, (list, tuple)):
    return {'l': [_fingerprint(v) for v in x]}
  if isinstance(x, (np.ndarray, np.generic)):
    a = np.asarray(x)
    if a.dtype.kind in 'biuf':
      f = a.astype(np.float64).ravel()
      w = np.arange(1, f.size + 1, dtype=np.float64) / max(f.size, 1)
      return {'a': [list(a.shape), a.dtype.str, float(f.sum()), float((f * w).sum())]}
    return {'a': [list(a.shape), a.dtype.str, a.ravel().tolist()]}
  if x is None or isinstance(x, (bool, int, float, str)):
    return {'v': x}
  if callable(x):
    return {'f': getattr(x, '__qualname__', repr(x))}
  raise TypeError('cannot fingerprint %r' % type(x))


def _same(a, b, path='args'):
  """Fingerprints equal: structure and scalars exactly, array sums to 1e-9 relative (CPU libm may differ in the last bit)."""
  if a.keys() != b.keys():
    return '%s: %s vs %s' % (path, sorted(a), sorted(b))
  (k, va), vb = next(iter(a.items())), b[next(iter(a))]
  if k == 'a' and len(va) == 4:
    if va[:2] != vb[:2] or len(vb) != 4:
      return '%s: array %s vs %s' % (path, va[:2], vb[:2])
    for x, y in zip(va[2:], vb[2:]):
      if abs(x - y) > 1e-9 * max(1.0, abs(x), abs(y)):
        return '%s: array sums %r vs %r' % (path, va[2:], vb[2:])
    return None
  if k in ('d', 'l'):
    if len(va) != len(vb):
      return '%s: %d vs %d entries' % (path, len(va), len(vb))
    for i, (x, y) in enumerate(zip(va, vb)):
      if k == 'd':
        if x[0] != y[0]:
          return '%s: key %r vs %r' % (path, x[0], y[0])
        err = _same(x[1], y[1], '%s[%r]' % (path, x[0]))
      else:
        err = _same(x, y, '%s[%d]' % (path, i))
      if err:
        return err
    return None
  return None if va == vb else '%s: %r vs %r' % (path, va, vb)


def _encode(x, arrays):
  """Result -> JSON skeleton; arrays go to ``arrays`` (types are kept: tuple / list / set, NumPy scalar / Python scalar)."""
  x = _numpy(x)
  if isinstance(x, dict):
    return {'d': [[_encode(k, arrays), _encode(v, arrays)] for k, v in x.items()]}
  if isinstance(x, tuple):
    return {'t': [_encode(v, arrays) for v in x]}
  if isinstance(x, list):
    return {'l': [_encode(v, arrays) for v in x]}
  if isinstance(x, (set, frozenset)):
    return {'s': [_encode(v, arrays) for v in sorted(x, key=repr)]}
  if isinstance(x, (np.ndarray, np.generic)):
    key = 'a%d' % len(arrays)
    arrays[key] = np.asarray(x)
    return {'n' if isinstance(x, np.generic) else 'a': key}
  if x is None or isinstance(x, (bool, int, float, str)):
    return {'v': x}
  raise TypeError('cannot record %r' % type(x))


def _decode(e, arrays):
  (k, v), = e.items()
  if k == 'd':
    return {_decode(a, arrays): _decode(b, arrays) for a, b in v}
  if k == 't':
    return tuple(_decode(a, arrays) for a in v)
  if k == 'l':
    return [_decode(a, arrays) for a in v]
  if k == 's':
    return {_decode(a, arrays) for a in v}
  if k == 'a':
    return arrays[v]
  if k == 'n':
    return arrays[v][()]
  return v


class recorded:
  """Context manager: ``rec(fn, *args, **kwargs)`` returns the next recorded result of ``fn`` for these arguments
  (or, under TG_RECORD_REFERENCE=1, runs ``fn`` and records it).  ``drop``: keys of a dict result left out; ``prune``:
  applied to the result before it is recorded (own_gradients)."""

  def __init__(self, name, drop=DROP, prune=None):
    self.path = os.path.join(GOLDEN, name + '.npz')
    self.drop, self.prune = tuple(drop), prune
    self.calls, self.arrays, self.i = [], {}, 0
    if not RECORD:
      if not os.path.exists(self.path):
        raise FileNotFoundError('%s: no recording (make it with TG_RECORD_REFERENCE=1 where the reference tree is '
                                'importable)' % os.path.relpath(self.path))
      with np.load(self.path, allow_pickle=False) as z:
        self.arrays = {k: z[k] for k in z.files if k != '__meta__'}
        self.calls = json.loads(str(z['__meta__']))

  def __enter__(self):
    return self

  def __call__(self, fn, *args, **kwargs):
    fp = _fingerprint([fn, list(args), kwargs])
    if RECORD:
      out = fn(*args, **kwargs)
      if isinstance(out, dict):
        out = {k: v for k, v in out.items() if k not in self.drop}
      if self.prune is not None:
        out = self.prune(out)
      self.calls.append(dict(args=fp, result=_encode(out, self.arrays)))
      return out
    assert self.i < len(self.calls), '%s holds %d calls, the test makes more' % (self.path, len(self.calls))
    call = self.calls[self.i]
    self.i += 1
    err = _same(call['args'], fp)
    assert err is None, '%s, call %d: the arguments differ from the recorded ones (%s)' % (self.path, self.i - 1, err)
    return _decode(call['result'], self.arrays)

  def __exit__(self, exc_type, *_):
    if exc_type is None:
      self.close()
    return False

  def close(self):
    """Writes the recording (TG_RECORD_REFERENCE=1), else checks that every recorded call was replayed."""
    if RECORD:
      os.makedirs(GOLDEN, exist_ok=True)
      np.savez_compressed(self.path, __meta__=np.array(json.dumps(self.calls)), **self.arrays)
    else:
      assert self.i == len(self.calls), '%s holds %d calls, the test made %d' % (self.path, len(self.calls), self.i)


def replay(name, fn, *args, drop=DROP, prune=None, **kwargs):
  """One recorded call: ``replay('live_gan', ref_runner.run, flags, s, t)``."""
  with recorded(name, drop, prune) as rec:
    return rec(fn, *args, **kwargs)
