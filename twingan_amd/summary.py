"""TensorFlow event files (``events.out.tfevents.<secs>.<host>``): the writer behind tf.summary.FileWriter as slim.learning.train
runs it every --save_summaries_secs (model/model_inheritor.py:1094-1126), and a reader that verifies the checksums.

Format, from TF 1.8's sources (core/lib/io/record_writer.cc, core/util/event.proto, core/framework/summary.proto,
core/lib/histogram/histogram.cc); the files have not been opened in TensorBoard, which is not installed where this was written:

  record     uint64 length | masked crc32c(length bytes) | data | masked crc32c(data)            (little endian)
  Event      wall_time = 1 (double), step = 2 (int64), file_version = 3 (string), summary = 5 (Summary)
  Summary    value = 1 (repeated Value);  Value: tag = 1 (string), simple_value = 2 (float), histo = 5 (HistogramProto)
  Histogram  min = 1, max = 2, num = 3, sum = 4, sum_squares = 5 (double), bucket_limit = 6, bucket = 7 (packed double)

The first record of a file is Event{wall_time, file_version = 'brain.Event:2'}.  Scalar fields that are zero are left out, as
proto3 serialises them.  The checksum, varint and field helpers are checkpoint.py's.
"""
import os
import socket
import struct
import time

import numpy as np

from .checkpoint import _field, _parse_message, _put_varint, crc32c, mask_crc

FILE_VERSION = 'brain.Event:2'
DBL_MAX = float(np.finfo(np.float64).max)


def _double(num, v):
  b = struct.pack('<d', float(v))
  return b'' if b == b'\0' * 8 else _field(num, 1, b)


def _bytes(num, payload):
  return _field(num, 2, _put_varint(len(payload)) + payload)


def _packed_doubles(num, values):
  values = np.asarray(values, dtype='<f8')
  return _bytes(num, values.tobytes()) if values.size else b''


def collapse_buckets(limits, buckets):
  """Histogram::EncodeToProto: a run of empty buckets becomes ONE entry that carries the last limit of the run (and its
  count, 0); a histogram without entries gets (DBL_MAX, 0).  -> (bucket_limit, bucket) as float64 arrays."""
  limits, buckets = np.asarray(limits, dtype=np.float64), np.asarray(buckets, dtype=np.float64)
  keep = buckets > 0
  # an empty bucket is written only where the next one is not empty, or where it is the last of all
  last_of_run = np.ones(len(buckets), dtype=bool)
  last_of_run[:-1] = keep[1:]
  sel = keep | last_of_run
  if not sel.any():
    return np.array([DBL_MAX]), np.array([0.0])
  return limits[sel], buckets[sel]


def histogram_proto(mn, mx, num, total, sum_squares, limits, buckets):
  """HistogramProto bytes; an empty histogram (num == 0) is num = 0, min = DBL_MAX, max = -DBL_MAX as TF's Histogram::Clear."""
  if not num:
    mn, mx, total, sum_squares = DBL_MAX, -DBL_MAX, 0.0, 0.0
  lim, cnt = collapse_buckets(limits, buckets)
  return (_double(1, mn) + _double(2, mx) + _double(3, num) + _double(4, total) + _double(5, sum_squares) +
          _packed_doubles(6, lim) + _packed_doubles(7, cnt))


def scalar_value(tag, value):
  return _bytes(1, tag.encode()) + _field(2, 5, struct.pack('<f', float(value)))


def histogram_value(tag, proto):
  return _bytes(1, tag.encode()) + _bytes(5, proto)


def event(wall_time, step=0, values=None, file_version=None):
  """Event bytes: ``values`` are Summary.Value payloads (scalar_value / histogram_value)."""
  out = _double(1, wall_time)
  if step:
    out += _field(2, 0, _put_varint(int(step)))
  if file_version is not None:
    out += _bytes(3, file_version.encode())
  if values is not None:
    out += _bytes(5, b''.join(_bytes(1, v) for v in values))
  return out


def record(data):
  head = struct.pack('<Q', len(data))
  return head + struct.pack('<I', mask_crc(crc32c(head))) + data + struct.pack('<I', mask_crc(crc32c(data)))


class EventWriter:
  """Appends records to <logdir>/events.out.tfevents.<secs>.<host>; every add is flushed."""

  def __init__(self, logdir, wall_time=None, host=None):
    os.makedirs(logdir, exist_ok=True)
    now = time.time() if wall_time is None else wall_time
    self.path = os.path.join(logdir, 'events.out.tfevents.%010d.%s' % (int(now), host or socket.gethostname()))
    self._fh = open(self.path, 'ab')
    self._write(event(now, file_version=FILE_VERSION))

  def _write(self, data):
    self._fh.write(record(data))
    self._fh.flush()

  def add(self, step, values, wall_time=None):
    self._write(event(time.time() if wall_time is None else wall_time, step, values))

  def close(self):
    if self._fh is not None:
      self._fh.close()
      self._fh = None


def _one(msg, num, kind, default):
  if num not in msg:
    return default
  v = msg[num][-1]
  if kind == 'd':
    return struct.unpack('<d', struct.pack('<Q', v))[0]
  if kind == 'f':
    return struct.unpack('<f', struct.pack('<I', v))[0]
  return v


def _parse_histogram(buf):
  m = _parse_message(buf)
  out = {k: _one(m, i, 'd', 0.0) for i, k in enumerate(('min', 'max', 'num', 'sum', 'sum_squares'), 1)}
  out['bucket_limit'] = np.frombuffer(b''.join(m.get(6, [])), dtype='<f8').copy()
  out['bucket'] = np.frombuffer(b''.join(m.get(7, [])), dtype='<f8').copy()
  return out


def read_events(path, verify=True):
  """-> [dict(wall_time, step, file_version | None, values = {tag: float | histogram dict})] of an event file.  ``verify``:
  both checksums of every record; a mismatch or a cut-off record raises ValueError."""
  data = open(path, 'rb').read()
  pos, out = 0, []
  while pos < len(data):
    if pos + 12 > len(data):
      raise ValueError('%s: record header cut off at byte %d' % (path, pos))
    head = data[pos:pos + 8]
    (n,), (crc,) = struct.unpack('<Q', head), struct.unpack_from('<I', data, pos + 8)
    if verify and crc != mask_crc(crc32c(head)):
      raise ValueError('%s: length checksum mismatch at byte %d' % (path, pos))
    if pos + 12 + n + 4 > len(data):
      raise ValueError('%s: record cut off at byte %d' % (path, pos))
    body = data[pos + 12:pos + 12 + n]
    (crc,) = struct.unpack_from('<I', data, pos + 12 + n)
    if verify and crc != mask_crc(crc32c(body)):
      raise ValueError('%s: data checksum mismatch in the record at byte %d' % (path, pos))
    pos += 12 + n + 4
    m = _parse_message(body)
    ev = dict(wall_time=_one(m, 1, 'd', 0.0), step=_one(m, 2, 'i', 0),
              file_version=m[3][-1].decode() if 3 in m else None, values={})
    for summ in m.get(5, []):
      for val in _parse_message(summ).get(1, []):
        v = _parse_message(val)
        tag = v[1][-1].decode()
        ev['values'][tag] = _parse_histogram(v[5][-1]) if 5 in v else _one(v, 2, 'f', 0.0)
    out.append(ev)
  return out


def find_event_files(logdir):
  return sorted(os.path.join(logdir, f) for f in os.listdir(logdir) if f.startswith('events.out.tfevents.'))
