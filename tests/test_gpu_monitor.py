"""Training summaries and sample grids on the device (include/twingan_hip_summary.h, twingan_amd/monitor.py) against the
float64 restatement tests/summary_ref.py: every bucket edge of TensorFlow's histogram, every bit pattern of the two 16-bit
formats, sizes and layouts with canaries round every output and the workspace, the sums' reordering bound and their
reproducibility, the grid's byte rule, and the monitor on a small trainer -- what it reports, and that it leaves training
bit-identical.

Counts, buckets, minima and maxima are compared for EQUALITY.  The two sums are held to n * 2^-52 * (sum of |terms|): the
bound for reordering a double sum whose terms (double(v), double(v)^2 of a float v) are exact."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import summary_ref as R      # noqa: E402

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
GUARD = 256          # canary bytes on either side of every output (keeps the view 256-byte aligned)
FILL = 0x5A
NB = 1551
EPS52 = 2.0 ** -52
DTYPES = {'fp32': torch.float32, 'bf16': torch.bfloat16, 'fp16': torch.float16}
STATS_DT = np.dtype([('sum', '<f8'), ('sum_squares', '<f8'), ('min', '<f4'), ('max', '<f4'), ('num', '<u4'), ('zeros', '<u4'),
                     ('nonfinite', '<u4'), ('reserved', '<u4')])


def _stream():
  return torch.cuda.current_stream().cuda_stream


def _guarded(nbytes):
  buf = torch.full((nbytes + 2 * GUARD,), FILL, dtype=torch.uint8, device=DEV)
  return buf, buf[GUARD:GUARD + nbytes]


def _intact(buf, nbytes):
  return bool((buf[:GUARD] == FILL).all()) and bool((buf[GUARD + nbytes:] == FILL).all())


def _limits_dev():
  from twingan_amd import ops
  return torch.from_numpy(ops.summary_limits()[1].copy()).to(DEV)


def _run(jobs, scale=1.0, scale_dev=None, nout=None, out_of=None):
  """``jobs``: [(tensor whose data_ptr is the base, rows, row_valid, row_stride)] -> (stats record array, buckets [n, 1551], raw
  stats bytes).  Results, buckets and workspace lie between canaries, which must be intact afterwards."""
  import ctypes
  from twingan_amd import _lib, ops
  lib = _lib.load()
  n = len(jobs)
  nout = nout or n
  host = ctypes.create_string_buffer(lib.tg_summary_table_bytes(n))
  blocks = ctypes.c_int32(0)
  for k, (t, rows, valid, stride) in enumerate(jobs):
    _lib.call('tg_summary_table_fill', t.data_ptr(), ops._dt(t), rows, valid, stride, out_of[k] if out_of else k, k, ctypes.addressof(host),
              ctypes.byref(blocks))
  table = torch.frombuffer(bytearray(host.raw), dtype=torch.uint8).to(DEV)
  ws_bytes = lib.tg_summary_workspace_bytes(blocks.value)
  wbuf, ws = _guarded(ws_bytes)
  sbuf, stats = _guarded(nout * 40)
  bbuf, buckets = _guarded(nout * NB * 4)
  lim = _limits_dev()
  sd = None if scale_dev is None else torch.tensor([scale_dev], dtype=torch.float32, device=DEV)
  _lib.call('tg_summary_multi', table.data_ptr(), n, blocks.value, nout, float(scale), None if sd is None else sd.data_ptr(),
            lim.data_ptr(), stats.data_ptr(), buckets.data_ptr(), ws.data_ptr(), ws_bytes, _stream())
  torch.cuda.synchronize()
  assert _intact(wbuf, ws_bytes), 'the workspace was overrun'
  assert _intact(sbuf, nout * 40), 'the results were overrun'
  assert _intact(bbuf, nout * NB * 4), 'the buckets were overrun'
  raw = stats.cpu().numpy().tobytes()
  return np.frombuffer(raw, dtype=STATS_DT).copy(), buckets.cpu().numpy().view(np.uint32).reshape(nout, NB).copy(), raw


def _check(st, bk, want, what=''):
  """One result row against the restatement: equality of everything but the two sums, which get the reordering bound."""
  for f in ('num', 'zeros', 'nonfinite'):
    assert int(st[f]) == want[f], (what, f, int(st[f]), want[f])
  diff = np.nonzero(bk != want['bucket'])[0]
  assert diff.size == 0, (what, 'buckets differ at', diff[:8].tolist(), bk[diff[:8]].tolist(), want['bucket'][diff[:8]].tolist())
  assert np.float32(st['min']) == want['min'] and np.float32(st['max']) == want['max'], (what, st['min'], st['max'], want['min'], want['max'])
  n = want['num']
  assert abs(float(st['sum']) - want['sum']) <= n * EPS52 * want['abs_sum'], (what, 'sum', float(st['sum']), want['sum'])
  assert abs(float(st['sum_squares']) - want['sum_squares']) <= n * EPS52 * want['sum_squares'], (what, 'sum_squares',
                                                                                                  float(st['sum_squares']), want['sum_squares'])


def _dense(t):
  return (t, 1, t.numel(), t.numel())


# ------------------------------------------------------------------------------------------------ every bucket edge
def test_every_bucket_edge_fp32():
  up = R.round_up_f32(R.positive_limits())
  assert up.size == 774
  edges = np.concatenate([np.nextafter(up, np.float32(0)), up, np.nextafter(up, np.float32(np.inf))])
  edges = np.concatenate([edges, -edges])
  assert edges.size == 2 * 774 * 3 and np.isfinite(edges).all()
  fmax, tiny = np.finfo(np.float32).max, np.finfo(np.float32).tiny
  extra = np.array([0.0, -0.0, 1e-13, -1e-13, fmax, -fmax, 1e20, 1.0000001e20, tiny, -tiny], dtype=np.float32)
  v = np.concatenate([edges, extra]).astype(np.float32)
  want = R.summarize(v)
  # the edges are edges: below a limit and at it lie in different buckets, for every limit
  lim = R.limits()
  idx = np.searchsorted(lim, edges[:3 * 774].astype(np.float64), side='right').reshape(3, 774)
  assert np.all(idx[1] == idx[0] + 1) and np.all(idx[2] == idx[1])
  st, bk, _ = _run([_dense(torch.from_numpy(v).to(DEV))])
  _check(st[0], bk[0], want, 'edges')
  # both zeros, 1e-13, the smallest normal and the float below 1e-12 | their negatives but the zeros
  assert int(st[0]['zeros']) == 2 and bk[0][776] == 5 and bk[0][775] == 3


@pytest.mark.parametrize('fmt', ['bf16', 'fp16'])
def test_every_bit_pattern_of_the_16_bit_formats(fmt):
  bits = torch.arange(65536, dtype=torch.int32).to(torch.int16)
  t = bits.view(DTYPES[fmt]).to(DEV)
  v = t.float().cpu().numpy()
  want = R.summarize(v)
  assert want['nonfinite'] == (2 * 128 if fmt == 'bf16' else 2 * 1024) and want['zeros'] == 2
  st, bk, _ = _run([_dense(t)])
  _check(st[0], bk[0], want, fmt)


# ------------------------------------------------------------------------------------------------ sizes and layouts
def _values(numel, seed, dtype=torch.float32):
  """Normal draws over many magnitudes with zeros of both signs and a few non-finite values."""
  g = torch.Generator().manual_seed(seed)
  x = torch.randn(numel, generator=g) * torch.pow(10.0, torch.randint(-9, 9, (numel,), generator=g).float())
  k = torch.arange(numel)
  x[k % 11 == 3] = 0.0
  x[k % 53 == 7] = -0.0
  x[k % 997 == 5] = float('nan')
  x[k % 1499 == 9] = float('-inf')
  return x.to(dtype)


SIZES = [(1, 0), (3, 0), (255, 0), (257, 0), (1027, 0), (1027, 1), (300000, 0)]


@pytest.mark.parametrize('fmt', ['fp32', 'bf16', 'fp16'])
@pytest.mark.parametrize('size', SIZES, ids=lambda p: '%d+%d' % p)
def test_sizes(size, fmt):
  numel, off = size
  shift = off * (1 if fmt == 'fp32' else 2)      # elements in 4 bytes: the view starts 4 bytes behind a 16-byte boundary
  buf = torch.full((numel + shift + 8,), float('nan'), dtype=DTYPES[fmt], device=DEV)
  t = buf[shift:shift + numel]
  t.copy_(_values(numel, numel + off, DTYPES[fmt]))
  assert t.data_ptr() % 16 == (4 if off else 0)
  before = buf.clone()
  st, bk, raw = _run([_dense(t)])
  _check(st[0], bk[0], R.summarize(t.float().cpu().numpy()), '%s %d+%d' % (fmt, numel, off))
  assert torch.equal(buf.view(torch.uint8), before.view(torch.uint8)), 'the input was written'
  # two launches on the same input: bit-identical
  st2, bk2, raw2 = _run([_dense(t)])
  assert raw2 == raw and np.array_equal(bk2, bk)


def test_five_million_elements_fp32():
  """More than one sweep of any grid: 306 workgroups' partials added in order."""
  numel = 5000000
  t = _values(numel, 77).to(DEV)
  st, bk, raw = _run([_dense(t)])
  _check(st[0], bk[0], R.summarize(t.cpu().numpy()), '5M')
  assert _run([_dense(t)])[2] == raw


@pytest.mark.parametrize('fmt', ['fp32', 'bf16', 'fp16'])
def test_strided_rows_never_read_the_padding(fmt):
  rows, valid, stride = 9, 15, 20
  x = torch.empty(rows, stride, dtype=DTYPES[fmt])
  x[:, :valid] = _values(rows * valid, 3, DTYPES[fmt]).reshape(rows, valid)
  x[:, valid::2] = float('nan')
  x[:, valid + 1::2] = 1e30
  t = x.to(DEV)
  st, bk, _ = _run([(t, rows, valid, stride)])
  _check(st[0], bk[0], R.summarize(x[:, :valid].float().numpy()), 'strided ' + fmt)


def test_table_of_mixed_jobs():
  g = [_values(5, 1).to(DEV), _values(40000, 2, torch.bfloat16).to(DEV), _values(16384, 3, torch.float16).to(DEV),
       _values(16385, 4).to(DEV), _values(3 * 7 * 6, 5).reshape(3, 7, 6).to(DEV), _values(1, 6).to(DEV), _values(70000, 7).to(DEV)]
  jobs = [_dense(t) for t in g]
  jobs[4] = (g[4], 3, 5 * 6, 7 * 6)      # [3, 5, 6] inside [3, 7, 6]
  # the result rows in another order than the jobs, one row of the eight left alone
  order = [6, 0, 3, 7, 1, 2, 4]
  st, bk, _ = _run(jobs, nout=8, out_of=order)
  for k, t in enumerate(g):
    v = t.float().cpu().numpy()
    if k == 4:
      v = v[:, :5, :]
    _check(st[order[k]], bk[order[k]], R.summarize(v), 'job %d' % k)
  assert st[5].tobytes() == bytes([FILL]) * 40, 'a result row that no job names was written'
  assert not bk[5].any()      # ... but its buckets are zeroed with the rest


def test_all_zero_all_nan_and_empty_after_exclusion():
  fmax = float(np.finfo(np.float32).max)
  zeros = torch.zeros(1000)
  zeros[::2] = -0.0
  nans = torch.full((1000,), float('nan'))
  big = torch.tensor([fmax, -fmax, fmax / 2, float('inf')] * 10)      # times 4: all of it overflows
  st, bk, _ = _run([_dense(zeros.to(DEV)), _dense(nans.to(DEV)), _dense(big.to(DEV))], scale=4.0)
  for k, v in enumerate((zeros, nans, big)):
    _check(st[k], bk[k], R.summarize(R.values(v.numpy(), 4.0)), 'case %d' % k)
  assert (int(st[0]['num']), int(st[0]['zeros']), int(bk[0][776])) == (1000, 1000, 1000)
  for k, n in ((1, 1000), (2, 40)):
    assert (int(st[k]['num']), int(st[k]['nonfinite'])) == (0, n) and not bk[k].any()
    assert st[k]['min'] == R.FLT_MAX and st[k]['max'] == -R.FLT_MAX and st[k]['sum'] == 0 and st[k]['sum_squares'] == 0


@pytest.mark.parametrize('how', ['value', 'pointer', 'both'])
def test_scale(how):
  """1 / 128 by value, through the device scalar, and both: exact for a power of two.  The inputs stay at or above
  2^-126 * 2^14, so no product is subnormal."""
  g = torch.Generator().manual_seed(11)
  x = torch.randn(5000, generator=g) * torch.pow(2.0, torch.randint(-100, 100, (5000,), generator=g).float())
  x[::7] = 0.0
  assert float(x[x != 0].abs().min()) >= 2.0 ** -112
  s, d = {'value': (1 / 128, None), 'pointer': (1.0, 1 / 128), 'both': (1 / 128, 1 / 128)}[how]
  st, bk, _ = _run([_dense(x.to(DEV))], scale=s, scale_dev=d)
  want = R.summarize(R.values(x.numpy(), s, d))
  _check(st[0], bk[0], want, how)
  exact = x.double().numpy() * s * (d or 1.0)
  assert np.array_equal(R.values(x.numpy(), s, d).astype(np.float64), exact)


def test_wrapper_from_a_flat_buffer():
  """ops.tensor_summaries over (offset, shape, phys) entries of a flat buffer, rows appended to a shared SummaryBuffer."""
  from twingan_amd import ops
  flat = _values(4096, 21).to(DEV)
  entries = [(0, (3, 3, 5, 4), (3, 3, 8, 4)), (320, (7,), (7,)), (1024, (64, 40), (64, 40)), (4000, (), ())]
  buf = ops.SummaryBuffer(6, DEV, extra=2)
  ops.tensor_summaries([flat[100:200].contiguous()], out=buf, row=0)
  ops.tensor_summaries(flat=flat, entries=entries, scale=0.5, out=buf, row=2)
  buf.extra_view().copy_(torch.tensor([1.5, -2.0], device=DEV))
  st, bk, extra = buf.read(extra=True)
  f = flat.cpu().numpy()
  wants = [f[100:200], None, f[:288].reshape(3, 3, 8, 4)[:, :, :5, :] * np.float32(0.5), f[320:327] * np.float32(0.5),
           f[1024:1024 + 2560] * np.float32(0.5), f[4000:4001] * np.float32(0.5)]
  for k, w in enumerate(wants):
    if w is not None:
      _check(st[k], bk[k], R.summarize(w), 'row %d' % k)
  assert int(st[1]['num']) == 0 and not bk[1].any() and extra.tolist() == [1.5, -2.0]
  with pytest.raises(Exception):
    ops.summary_rows((3, 3, 5, 4), (3, 4, 8, 4))


# ------------------------------------------------------------------------------------------------ grids
def _grid(batches, rows, cols):
  """ops.image_grid into a grid between canaries -> uint8 numpy [rows * h, cols * w, 3]."""
  from twingan_amd import ops
  h, w = batches[0][0].shape[1:3]
  n = rows * h * cols * w * 3
  buf, view = _guarded(n)
  out = ops.image_grid(batches, rows, cols, out=view.view(rows * h, cols * w, 3))
  torch.cuda.synchronize()
  assert _intact(buf, n), 'the launch wrote outside the grid'
  return out.cpu().numpy()


def test_grid_byte_rule_fp32():
  k = np.arange(256, dtype=np.float32) / np.float32(255.0)
  v = np.concatenate([np.nextafter(k, np.float32(-1)), k, np.nextafter(k, np.float32(2)),
                      np.array([-0.5, 1.5, np.nan, np.inf, -np.inf], dtype=np.float32)])
  x = np.zeros(16 * 17 * 3, dtype=np.float32)
  x[:v.size] = v
  x = x.reshape(1, 16, 17, 3)
  got = _grid([(torch.from_numpy(x).to(DEV), 0)], 1, 1)
  want = R.image_grid([(x, 0)], 1, 1, 16, 17)
  assert np.array_equal(got, want), np.argwhere(got != want)[:5]
  # k / 255 * 255 in float32 is k or just below it: the rule truncates, as the reference's astype(int32) does
  assert want.reshape(-1)[256:512].tolist() == np.trunc(k * np.float32(255.0)).astype(int).tolist()


@pytest.mark.parametrize('fmt', ['bf16', 'fp16'])
def test_grid_every_bit_pattern_of_the_16_bit_formats(fmt):
  bits = torch.zeros(4 * 64 * 86 * 3, dtype=torch.int16)
  bits[:65536] = torch.arange(65536, dtype=torch.int32).to(torch.int16)
  t = bits.view(DTYPES[fmt]).reshape(4, 64, 86, 3).to(DEV)
  got = _grid([(t, 0)], 4, 1)
  want = R.image_grid([(t.float().cpu().numpy(), 0)], 4, 1, 64, 86)
  assert np.array_equal(got, want), np.argwhere(got != want)[:5]


@pytest.mark.parametrize('c', [1, 3])
@pytest.mark.parametrize('slots', [1, 2, 16])
@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('hw', [4, 16])
def test_grid_layouts(hw, n, slots, c):
  """Every slot but one filled (with 2 and 16 slots: slot 1 stays empty), batches of mixed dtypes, one batch shorter than the
  grid's rows when n > 1."""
  g = torch.Generator().manual_seed(hw + 10 * n + 100 * slots + c)
  batches = []
  for s in range(slots):
    if slots > 1 and s == 1:
      continue
    dt = (torch.float32, torch.bfloat16, torch.float16)[s % 3]
    count = n - 1 if (n > 1 and s == 0) else n
    batches.append(((torch.rand(count, hw, hw, c, generator=g) * 1.4 - 0.2).to(dt).to(DEV), s))
  got = _grid(batches, n, slots)
  want = R.image_grid([(t.float().cpu().numpy(), s) for t, s in batches], n, slots, hw, hw)
  assert got.shape == (n * hw, slots * hw, 3) and np.array_equal(got, want)
  if slots > 1:
    assert not got[:, hw:2 * hw].any()
  if n > 1:
    assert not got[(n - 1) * hw:, :hw].any()


# ------------------------------------------------------------------------------------------------ the monitor on a trainer
HW, B = 16, 2


def _pair(precision):
  g = torch.Generator().manual_seed(8)
  s, t = torch.rand(B, HW, HW, 3, generator=g), torch.rand(B, HW, HW, 3, generator=g)
  dt = torch.float16 if precision == 'fp16' else torch.float32
  return s.to(DEV).to(dt), t.to(DEV).to(dt)


def _config(mode, **kw):
  from twingan_amd import Config
  if mode == 'fp32':
    return Config(hw=HW, max_ch=8, precision='fp32', **kw)
  return Config(hw=HW, max_ch=8, precision='fp16', loss_scale=128.0, dynamic_loss_scale=mode == 'fp16-dynamic', **kw)


def _check_histogram(got, v, what):
  want = R.summarize(v)
  st = dict(num=got['num'], zeros=want['zeros'], nonfinite=want['nonfinite'], min=got['min'], max=got['max'], sum=got['sum'],
            sum_squares=got['sum_squares'])
  _check(st, got['bucket'], want, what)
  return want


@pytest.mark.parametrize('mode', ['fp32', 'fp16', 'fp16-dynamic'])
def test_monitor_reports_gradients_variables_and_losses(mode, tmp_path):
  from twingan_amd.monitor import Monitor
  from twingan_amd.twingan import Trainer
  tr = Trainer(_config(mode), device=DEV, seed=0)
  s, t = _pair(mode[:4])
  mon = Monitor(sample_fn=lambda hw, b: (s, t), save_summaries_steps=1, log_image_every_n_iter=0).begin(tr, str(tmp_path), B)
  store = tr.store
  padded = [k for k, sp in store.specs.items() if sp['phys'] != sp['shape']]
  assert padded, 'this size has a conv kernel stored with padded input channels'
  try:
    for group in ('g', 'd'):
      loss, terms = tr.run(s, t)
      vals = mon.values(*mon.collect())
      torch.cuda.synchronize()
      inv = 1.0 / (tr.loss_scale_state()[group]['scale'] if mode == 'fp16-dynamic' else tr.cfg.loss_scale)
      assert inv == (1.0 if mode == 'fp32' else 1.0 / 128)
      names = [k for k, sp in store.specs.items() if sp['group'] == group]
      assert names and sorted(k[len('gradients/'):] for k in vals if k.startswith('gradients/')) == sorted(names)
      for k in names:
        g = store._logical(store.P[k].grad, store.specs[k]).float().cpu().numpy()
        want = _check_histogram(vals['gradients/' + k], R.values(g, inv), 'gradients/' + k)
        assert want['nonfinite'] == 0 and ('nonfinite/gradients/' + k) not in vals
        norm, ref = vals['gradient_norms/' + k], math.sqrt(want['sum_squares'])
        assert norm['num'] == 1 and norm['min'] == norm['max'] == norm['sum']
        assert abs(norm['sum'] - ref) <= (want['num'] + 1) * EPS52 * ref, (k, norm['sum'], ref)
        assert norm['bucket'].sum() == 1 and norm['bucket'][np.searchsorted(R.limits(), norm['sum'], side='right')] == 1
      assert any(vals['gradients/' + k]['sum_squares'] > 0 for k in names)
      sd = store.state_dict()
      for k in store.specs:
        _check_histogram(vals[k], sd[k].float().cpu().numpy(), k)
      tag = {'g': 'generator_loss', 'd': 'discriminator_loss'}[group]
      assert vals[tag] == float(loss.float().reshape(-1)[0]) and terms
      for k, v in terms.items():
        assert vals['losses/' + k] == float(v.float().reshape(-1)[0]), k
      assert vals['learning_rate'] == float(tr.cfg.learning_rate)
      if mode == 'fp16-dynamic':
        assert vals['loss_scale/g'] == vals['loss_scale/d'] == 128.0
      acts = sorted(k[len('activations/'):] for k in vals if k.startswith('activations/'))
      assert acts == sorted(['sources', 'targets', 's_prime_output', 't_prime_output', 's_cycle_output', 't_cycle_output',
                             'encoded_source_content_before_classification', 'encoded_target_content_before_classification'])
      _check_histogram(vals['activations/sources'], s.float().cpu().numpy(), 'activations/sources')
      assert vals['sparsity/sources'] == float((s == 0).sum()) / s.numel() and 0.0 <= vals['sparsity/s_prime_output'] <= 1.0
    assert 'generator_loss' in vals and 'discriminator_loss' in vals      # the second read-out carries both groups' last losses
  finally:
    mon.end()
    tr.close()


def _train(cfg, use_graph, monitor_dir):
  """Two G+D pairs on a fixed pair of batches, then the losses of a third pair -> every tensor training owns, cloned."""
  from twingan_amd.monitor import Monitor
  from twingan_amd.twingan import Trainer
  tr = Trainer(cfg, device=DEV, seed=3, use_graph=use_graph)
  s, t = _pair(cfg.precision)
  mon = None
  if monitor_dir is not None:
    mon = Monitor(sample_fn=lambda hw, b: (s, t), save_summaries_steps=1, log_image_every_n_iter=1).begin(tr, monitor_dir, B)
    mon.step(tr, 0)
  try:
    for step in range(2):
      tr.run(s, t)
      tr.run(s, t)
      if mon is not None:
        mon.step(tr, step + 1)
    torch.cuda.synchronize()
    st = tr.store
    out = {'flat/' + g: st.flat[g].clone() for g in st.GROUPS}
    out.update({'m/' + g: st.slots[g][0].clone() for g in st.GROUPS})
    out.update({'v/' + g: st.slots[g][1].clone() for g in st.GROUPS})
    out.update({'grad/' + g: st.grad[g].clone() for g in st.GROUPS})
    out.update({'state/' + k: v.clone() for k, v in st.state.items()})
    out['draws'] = tr._rng_state.clone()
    out['adam_step'] = tr._adam_step_dev.clone()
    for name in ('next_g', 'next_d'):
      loss, terms = tr.run(s, t)
      out[name] = loss.clone()
      out.update({name + '/' + k: v.clone() for k, v in terms.items()})
    torch.cuda.synchronize()
    assert use_graph == (tr._graphs is not None), tr.graph_fallback_reason
    return out
  finally:
    if mon is not None:
      mon.end()
    tr.close()


def _assert_same_training(a, b):
  assert sorted(a) == sorted(b)
  for k in a:
    assert torch.equal(a[k].contiguous().view(torch.uint8), b[k].contiguous().view(torch.uint8)), '%s differs with the monitor attached' % k


def _check_files(d):
  """The event file parses and holds the expected tags at steps 1 and 2; the eight PNGs of steps 0, 1, 2 decode."""
  from twingan_amd import summary
  files = summary.find_event_files(d)
  assert len(files) == 1 and os.path.basename(files[0]).startswith('events.out.tfevents.')
  evs = summary.read_events(files[0])
  assert evs[0]['file_version'] == 'brain.Event:2' and [e['step'] for e in evs[1:]] == [1, 2]
  for e in evs[1:]:
    tags = set(e['values'])
    assert {'generator_loss', 'discriminator_loss', 'learning_rate', 'activations/sources', 'sparsity/t_cycle_output',
            'losses/l_cyc_s'} <= tags, sorted(tags)[:40]
    grads = [k for k in tags if k.startswith('gradients/')]
    assert grads and all(k.startswith('gradients/discriminator_') for k in grads)      # the group the last run applied
    assert {'gradient_norms/' + k[len('gradients/'):] for k in grads} <= tags
    h = e['values']['generator/block_4x4x8/Conv/weights']
    assert h['num'] == 3 * 3 * 8 * 8 and h['bucket'].sum() == h['num'] and h['min'] < 0 < h['max']
    assert h['bucket_limit'].size == h['bucket'].size < 600 and np.all(np.diff(h['bucket_limit']) > 0)
  names = ['source', 'target', 's_prime', 't_prime', 's_cycle', 't_cycle', 'target_s_prime', 'source_t_prime']
  got = sorted(os.listdir(os.path.join(d, 'generated_samples')))
  assert got == sorted('%d_%s.png' % (step, n) for step in (0, 1, 2) for n in names)
  imgs = {n: R.decode_png(open(os.path.join(d, 'generated_samples', '2_%s.png' % n), 'rb').read()) for n in names}
  for n in names[:6]:
    assert imgs[n].shape == (B * HW, 8 * HW, 3)
  for n in names[6:]:
    assert imgs[n].shape == (B * HW, 16 * HW, 3)
  s, t = _pair('fp32')
  src = R.grid_bytes(s.cpu().numpy())
  assert np.array_equal(imgs['source'][:HW, :HW], src[0]) and np.array_equal(imgs['source'][HW:, 7 * HW:], src[1])
  # the reference's quirk: 'target_s_prime' pairs SOURCES with t', 'source_t_prime' TARGETS with s'; even columns are the originals
  inter = imgs['target_s_prime'].reshape(B * HW, 16, HW, 3)
  assert np.array_equal(inter[:, 0::2].reshape(B * HW, 8 * HW, 3), imgs['source'])
  assert np.array_equal(inter[:, 1::2].reshape(B * HW, 8 * HW, 3), imgs['t_prime'])
  inter = imgs['source_t_prime'].reshape(B * HW, 16, HW, 3)
  assert np.array_equal(inter[:, 0::2].reshape(B * HW, 8 * HW, 3), imgs['target'])
  assert np.array_equal(inter[:, 1::2].reshape(B * HW, 8 * HW, 3), imgs['s_prime'])


def test_monitor_leaves_training_bit_identical(tmp_path):
  cfg = _config('fp32')
  plain = _train(cfg, False, None)
  watched = _train(cfg, False, str(tmp_path))
  _assert_same_training(plain, watched)
  _check_files(str(tmp_path))


def test_monitor_leaves_training_bit_identical_eager_and_graph(tmp_path):
  cfg = _config('fp32')
  plain = _train(cfg, True, None)
  watched = _train(cfg, True, str(tmp_path))
  _assert_same_training(plain, watched)
  _check_files(str(tmp_path))


def test_monitor_restores_batch_norm_moving_statistics(tmp_path):
  cfg = _config('fp32', generator_norm_type='batch_norm')
  plain = _train(cfg, False, None)
  moving = [k for k in plain if k.startswith('state/') and 'moving_' in k]
  assert moving and any(float(plain[k].abs().sum()) not in (0.0, float(plain[k].numel())) for k in moving)
  watched = _train(cfg, False, str(tmp_path))
  _assert_same_training(plain, watched)


def test_pggan_trainer_gets_summaries_and_no_grids(tmp_path):
  """image_generation.PgganTrainer: variables, gradients and losses, no TwinGAN end points, no sample pass, no grids."""
  from twingan_amd import Config, summary
  from twingan_amd.image_generation import PgganTrainer
  from twingan_amd.monitor import Monitor
  tr = PgganTrainer(Config(hw=HW, max_ch=8, precision='fp32'), device=DEV, seed=0)
  t = _pair('fp32')[1]
  calls = []
  mon = Monitor(sample_fn=lambda hw, b: calls.append(hw), save_summaries_steps=1, log_image_every_n_iter=1).begin(tr, str(tmp_path), B)
  try:
    mon.step(tr, 0)
    loss_g = tr.run(None, t)[0]
    loss_d = tr.run(None, t)[0]
    mon.step(tr, 1)
    torch.cuda.synchronize()
  finally:
    mon.end()
    tr.close()
  assert not calls and not os.path.exists(os.path.join(str(tmp_path), 'generated_samples'))
  evs = summary.read_events(summary.find_event_files(str(tmp_path))[0])
  assert [e['step'] for e in evs[1:]] == [1]
  vals = evs[1]['values']
  assert vals['generator_loss'] == float(loss_g.float().reshape(-1)[0]) and vals['discriminator_loss'] == float(loss_d.float().reshape(-1)[0])
  assert not [k for k in vals if k.startswith(('activations/', 'sparsity/'))]
  names = list(tr.store.specs)
  assert all(k in vals for k in names) and all(('gradients/' + k in vals) == (tr.store.specs[k]['group'] == 'd') for k in names)


def test_run_progressive_writes_events_and_grids(tmp_path):
  from twingan_amd import Config, runner, summary
  from twingan_amd.monitor import Monitor
  g = torch.Generator().manual_seed(4)

  def batch_fn(hw, b):
    return torch.rand(b, hw, hw, 3, generator=g).to(DEV), torch.rand(b, hw, hw, 3, generator=g).to(DEV)

  mon = Monitor(sample_fn=batch_fn, save_summaries_steps=1, log_image_every_n_iter=2, log_image_n_per_hw=2)
  _, hist = runner.run_progressive(Config(max_ch=8, precision='fp32'), batch_fn, start_hw=8, max_hw=16, device=DEV,
                                   hw_to_batch_size={8: 2, 16: 2}, max_steps_per_stage=2, train_dir=str(tmp_path), monitor=mon)
  assert [h['stage'] for h in hist] == ['8', '8to16', '16']
  for h in hist:
    d = os.path.join(str(tmp_path), h['stage'])
    files = summary.find_event_files(d)
    assert len(files) == 1
    assert [e['step'] for e in summary.read_events(files[0])[1:]] == [1, 2]
    pngs = sorted(os.listdir(os.path.join(d, 'generated_samples')))
    assert len(pngs) == 16 and len([p for p in pngs if p.startswith('0_')]) == 8 and len([p for p in pngs if p.startswith('2_')]) == 8
    img = R.decode_png(open(os.path.join(d, 'generated_samples', '2_source_t_prime.png'), 'rb').read())
    assert img.shape == (2 * h['hw'], 4 * h['hw'], 3)
  with pytest.raises(ValueError):
    runner.run_progressive(Config(max_ch=8), batch_fn, start_hw=8, max_hw=8, device=DEV, monitor=mon)
