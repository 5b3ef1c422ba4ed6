"""Float64 restatement of the training summaries for the tests (tests/test_monitor_cpu.py, tests/test_gpu_monitor.py): the
TensorFlow default histogram limits by their defining loop, the bucket of a value by np.searchsorted(limits, v, 'right'),
the moments, the proto's collapse rule, the image grid's byte rule and a PNG decoder.  NumPy only; shares no code with twingan_amd."""
import struct
import zlib

import numpy as np

DBL_MAX = float(np.finfo(np.float64).max)
FLT_MAX = np.float32(np.finfo(np.float32).max)


def positive_limits():
  """TF 1.8 core/lib/histogram/histogram.cc InitDefaultBuckets, in double."""
  out = []
  v = 1e-12
  while v < 1e20:
    out.append(v)
    v *= 1.1
  return np.array(out, dtype=np.float64)


def limits():
  pos = positive_limits()
  return np.concatenate([[-DBL_MAX], -pos[::-1], [0.0], pos, [DBL_MAX]])


def round_up_f32(x):
  """Each double rounded UP to the nearest float32."""
  x = np.asarray(x, dtype=np.float64)
  f = x.astype(np.float32)
  low = f.astype(np.float64) < x
  return np.where(low, np.nextafter(f, np.float32(np.inf)), f).astype(np.float32)


def values(x, scale=1.0, scale_dev=None):
  """v = float(x) * scale (* scale_dev) in float32, as the kernel defines it; scale == 1 without scale_dev is float(x)."""
  v = np.asarray(x).astype(np.float32).reshape(-1)
  with np.errstate(over='ignore', invalid='ignore'):
    if not (scale == 1.0 and scale_dev is None):
      v = v * np.float32(scale)
      if scale_dev is not None:
        v = v * np.float32(scale_dev)
  return v.astype(np.float32)


def summarize(v):
  """The result of one tensor over float32 values ``v``: dict(num, zeros, nonfinite, min, max, sum, sum_squares, abs_sum,
  bucket[1551]); abs_sum = sum |v| for the reordering bound of ``sum``."""
  v = np.asarray(v, dtype=np.float32).reshape(-1)
  fin = np.isfinite(v)
  f = v[fin].astype(np.float64)
  lim = limits()
  idx = np.searchsorted(lim, f, side='right')
  assert f.size == 0 or (idx.min() >= 1 and idx.max() <= lim.size - 1)
  return dict(num=int(f.size), zeros=int((f == 0).sum()), nonfinite=int((~fin).sum()),
              min=np.float32(f.min()) if f.size else FLT_MAX, max=np.float32(f.max()) if f.size else -FLT_MAX,
              sum=float(np.sum(f)), sum_squares=float(np.sum(f * f)), abs_sum=float(np.sum(np.abs(f))),
              bucket=np.bincount(idx, minlength=lim.size).astype(np.uint32))


def collapse(lim, buckets):
  """Histogram::EncodeToProto, as its loop reads."""
  out_l, out_b = [], []
  i, n = 0, len(buckets)
  while i < n:
    end, count = lim[i], buckets[i]
    i += 1
    if count <= 0:
      while i < n and buckets[i] <= 0:
        end, count = lim[i], buckets[i]
        i += 1
    out_l.append(float(end))
    out_b.append(float(count))
  if not out_b:
    out_l, out_b = [DBL_MAX], [0.0]
  return np.array(out_l), np.array(out_b)


def grid_bytes(x):
  """clip(trunc(float32(x) * 255), 0, 255) with this project's definition of what astype(int32) leaves to the platform:
  NaN -> 0, products >= 255 (+inf included) -> 255, negative ones -> 0."""
  with np.errstate(over='ignore', invalid='ignore'):
    f = np.asarray(x).astype(np.float32) * np.float32(255.0)
  out = np.zeros(f.shape, dtype=np.uint8)
  mid = (f > 0) & (f < 255)
  out[mid] = np.trunc(f[mid]).astype(np.int32).astype(np.uint8)
  out[f >= 255] = 255
  return out


def image_grid(batches, rows, cols, h, w):
  """``batches``: [(array [n, h, w, c], column slot)] -> uint8 [rows * h, cols * w, 3]; of two batches with one slot the
  earlier wins, images beyond ``rows`` are dropped."""
  grid = np.zeros((rows * h, cols * w, 3), dtype=np.uint8)
  done = set()
  for x, col in batches:
    b = grid_bytes(x)
    if b.shape[-1] == 1:
      b = np.repeat(b, 3, axis=-1)
    for i in range(min(b.shape[0], rows)):
      if (i, col) not in done:
        done.add((i, col))
        grid[i * h:(i + 1) * h, col * w:(col + 1) * w] = b[i]
  return grid


def decode_png(data):
  """-> uint8 [h, w, 3] of a colour-type-2, 8-bit PNG whose rows all use filter 0; the chunk CRCs are verified."""
  assert data[:8] == b'\x89PNG\r\n\x1a\n'
  pos, chunks = 8, []
  while pos < len(data):
    (n,), kind = struct.unpack_from('>I', data, pos), data[pos + 4:pos + 8]
    body = data[pos + 8:pos + 8 + n]
    assert struct.unpack_from('>I', data, pos + 8 + n)[0] == zlib.crc32(kind + body) & 0xffffffff
    chunks.append((kind, body))
    pos += 12 + n
  assert [k for k, _ in chunks][0] == b'IHDR' and chunks[-1] == (b'IEND', b'')
  w, h, depth, colour, comp, filt, lace = struct.unpack('>IIBBBBB', chunks[0][1])
  assert (depth, colour, comp, filt, lace) == (8, 2, 0, 0, 0)
  raw = np.frombuffer(zlib.decompress(b''.join(b for k, b in chunks if k == b'IDAT')), dtype=np.uint8).reshape(h, 1 + 3 * w)
  assert not raw[:, 0].any()
  return raw[:, 1:].reshape(h, w, 3).copy()
