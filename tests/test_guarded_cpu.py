"""CPU: tests/guarded.py finds what it is for.  Stand-in "kernels" written in torch, each with ONE planted fault, run through
guarded.check on CPU tensors: a store one element past an output, one before it, a last row never written, a result that
takes in 0 * the element after an input, an input scribbled on.  Each must be reported against the right allocation and side;
the clean stand-in must pass.  (These are ordinary stores inside the harness's own buffers: nothing faults.)"""
import os

import pytest
import torch

import guarded as G

FILES = (os.path.abspath(__file__),)
ROWS, COLS = 5, 7


def _past(t, k):
  """The element k places from the start of t's memory (k = numel: one past the end, k = -1: one before the start)."""
  return torch.as_strided(t, (1,), (1,), t.storage_offset() + k)


def kernel_clean(x):
  scratch = torch.zeros(3, dtype=torch.float32)
  out = torch.empty(ROWS, COLS, dtype=x.dtype)
  out.copy_(x * 2 + scratch[0])
  return out


def kernel_writes_past_the_end(x):
  scratch = torch.zeros(3, dtype=torch.float32)
  out = torch.empty(ROWS, COLS, dtype=x.dtype)
  out.copy_(x * 2 + scratch[0])
  _past(out, out.numel()).fill_(1.0)
  return out


def kernel_writes_before_the_start(x):
  scratch = torch.zeros(3, dtype=torch.float32)
  out = torch.empty(ROWS, COLS, dtype=x.dtype)
  out.copy_(x * 2 + scratch[0])
  _past(scratch, -1).fill_(1.0)
  return out


def kernel_skips_the_last_row(x):
  out = torch.empty(ROWS, COLS, dtype=x.dtype)
  out[:-1].copy_(x[:-1] * 2)
  return out


def kernel_reads_past_an_input(x):
  out = torch.empty(ROWS, COLS, dtype=x.dtype)
  out.copy_(x * 2)
  out[-1, -1] += 0 * _past(x, x.numel())[0]      # "masked" by a multiply where a select was needed
  return out


def kernel_scribbles_on_its_input(x):
  out = torch.empty(ROWS, COLS, dtype=x.dtype)
  out.copy_(x * 2)
  x[2, 3] = 9.0
  return out


def kernel_scribbles_before_its_input(x):
  out = torch.empty(ROWS, COLS, dtype=x.dtype)
  out.copy_(x * 2)
  _past(x, -1).fill_(0.0)
  return out


def _x(dtype=torch.float32):
  return (torch.arange(ROWS * COLS, dtype=torch.float32).reshape(ROWS, COLS) / 8).to(dtype)


def _check(kernel, dtype=torch.float32, **kw):
  return G.check(kernel, [_x(dtype)], 'cpu', files=FILES, **kw)


def _planted(kernel, **kw):
  """A planted fault reaches outside its tensor, which only a guarded buffer has room for: the guarded run alone."""
  return _check(kernel, ordinary=False, **kw)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, torch.float16])
def test_a_clean_kernel_passes(dtype):
  A, B = _check(kernel_clean, dtype)
  assert torch.equal(A, _x(dtype) * 2)


def test_poison_is_nan_in_every_storage_type_and_guards_sit_where_they_should():
  with G.Guarded('cpu', files=FILES) as g:
    outs = [torch.empty(3, 5, dtype=dt) for dt in (torch.float32, torch.bfloat16, torch.float16)]
    z = torch.zeros(4, 4, 4, 4, dtype=torch.float32)
    f = torch.full((9,), 2.5)
    big = torch.empty(2, 256, 256, 8, dtype=torch.float32)      # one image is 2 MiB: the guard is capped at 1 MiB
  for o in outs:
    assert bool(torch.isnan(o).all()) and o.data_ptr() % 256 == 0
  assert bool((z == 0).all()) and bool((f == 2.5).all())
  assert len(g.allocs) == 6 and not g.damage()
  for a in g.allocs:
    assert a.off >= 64 << 10 and a.buf.numel() - a.off - a.nbytes >= 64 << 10
    assert bool((a.buf[:a.off] == G.GUARD_BYTE).all()) and bool((a.buf[a.off + a.nbytes:] == G.GUARD_BYTE).all())
    assert a.site.startswith('test_guarded_cpu.py:')
  assert g.allocs[5].off == 1 << 20
  assert G.guard_bytes((3, 100, 100, 8), 4) == 320000 + (-320000) % 256      # one image of a 4-d tensor
  other = torch.empty(4)      # outside the mode: an ordinary tensor
  assert other.numel() == 4


def test_a_store_past_the_end_is_reported_after_the_right_allocation():
  with pytest.raises(AssertionError) as e:
    _planted(kernel_writes_past_the_end)
  msg = str(e.value)
  assert 'allocation 1 ' in msg and '(5, 7)' in msg and 'after the tensor' in msg and 'byte +0 from its end' in msg, msg
  assert 'kernel_writes_past_the_end' in msg and 'allocation 0' not in msg


def test_a_store_before_the_start_is_reported_before_the_right_allocation():
  with pytest.raises(AssertionError) as e:
    _planted(kernel_writes_before_the_start)
  msg = str(e.value)
  assert 'allocation 0 ' in msg and '(3,)' in msg and 'before the tensor' in msg and 'byte -4 from its start' in msg, msg
  assert 'allocation 1' not in msg


def test_an_unwritten_row_is_reported():
  with pytest.raises(AssertionError) as e:
    _planted(kernel_skips_the_last_row)
  assert '7 element(s) not finite' in str(e.value) and 'first at flat index 28' in str(e.value), str(e.value)


def test_a_read_past_an_input_that_reaches_the_result_is_reported():
  with pytest.raises(AssertionError) as e:
    _planted(kernel_reads_past_an_input)
  assert '1 element(s) not finite' in str(e.value) and 'first at flat index 34' in str(e.value), str(e.value)


def test_a_write_to_an_input_or_its_surrounds_is_reported():
  with pytest.raises(AssertionError) as e:
    _planted(kernel_scribbles_on_its_input)
  assert 'operand 0' in str(e.value) and 'inside the tensor' in str(e.value), str(e.value)
  assert int(str(e.value).rsplit('byte ', 1)[1]) // 4 == 2 * COLS + 3, str(e.value)      # a byte of element [2, 3]
  with pytest.raises(AssertionError) as e:
    _planted(kernel_scribbles_before_its_input)
  assert 'operand 0' in str(e.value) and 'before the tensor' in str(e.value), str(e.value)
  assert -4 <= int(str(e.value).rsplit('byte ', 1)[1]) < 0, str(e.value)
  # an in/out operand may change inside, never around
  _check(kernel_scribbles_on_its_input, inout=(0,))
  with pytest.raises(AssertionError):
    _planted(kernel_scribbles_before_its_input, inout=(0,))
