"""Dynamic loss scaling, the parts that need no GPU: Config validation, the state struct's layout against the header, the new
symbols in the header and in the library's table, and the apply count a checkpoint is restored with."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('tg_loss_scale_state_bytes', 'tg_nonfinite_check', 'tg_loss_scale_tick', 'tg_adam_step_guarded',
               'tg_adam_ema_step_guarded')


def _header():
  with open(os.path.join(ROOT, 'include', 'twingan_hip.h')) as fh:
    return fh.read()


def test_config_validation():
  """Under the flag the initial scale is a power of two in [1, 2**24] and the growth interval at least 1; without the flag
  any loss_scale is accepted, as before."""
  from twingan_amd import Config
  c = Config()
  assert c.dynamic_loss_scale is False and c.loss_scale_growth_interval == 2000
  for scale in (1.0, 2.0, 128.0, 2.0 ** 24, 128):
    assert Config(dynamic_loss_scale=True, loss_scale=scale).loss_scale == scale
  for scale in (3.0, 100.0, 127.999, 0.5, 0.0, -2.0, 2.0 ** 25, float('inf'), float('nan')):
    with pytest.raises(ValueError):
      Config(dynamic_loss_scale=True, loss_scale=scale)
    Config(loss_scale=scale)
  for interval in (0, -1, 2.5):
    with pytest.raises(ValueError):
      Config(dynamic_loss_scale=True, loss_scale_growth_interval=interval)
    Config(loss_scale_growth_interval=interval)
  assert Config(dynamic_loss_scale=True, loss_scale_growth_interval=1).loss_scale_growth_interval == 1


def test_loss_scale_state_layout_matches_header():
  """The ctypes mirror has the header's fields, in its order and with its types; 32 bytes, the 64-bit total at offset 24;
  the library agrees."""
  from twingan_amd import _lib
  body = re.search(r'typedef struct TgLossScaleState \{(.*?)\} TgLossScaleState;', _header(), re.S).group(1)
  body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
  fields = re.findall(r'(float|int32_t|int64_t)\s+(\w+);', body)
  ctype = {'float': ctypes.c_float, 'int32_t': ctypes.c_int32, 'int64_t': ctypes.c_int64}
  assert [(name, ctype[t]) for t, name in fields] == list(_lib.TgLossScaleState._fields_)
  assert [name for _, name in fields] == ['scale', 'seed', 'inv_scale', 'found', 'skip', 'good_steps', 'skipped']
  S = _lib.TgLossScaleState
  assert ctypes.sizeof(S) == 32 and S.skipped.offset == 24 and S.seed.offset == 4 and S.found.offset == 12
  assert _lib.load().tg_loss_scale_state_bytes() == 32


def test_new_symbols_are_declared_and_exported():
  from twingan_amd import _lib
  header, lib = _header(), _lib.load()
  for name in NEW_SYMBOLS:
    assert re.search(r'\b%s\(' % name, header), '%s is not declared in the header' % name
    assert name in _lib.SIGNATURES and hasattr(lib, name)
    ret, args = _lib.SIGNATURES[name]
    decl = re.search(r'\b%s\((.*?)\);' % name, header, re.S).group(1)
    count = 0 if decl.strip() in ('', 'void') else decl.count(',') + 1
    assert len(args) == count, '%s: %d arguments in the table, %d in the header' % (name, len(args), count)
  # the entry points this mode stands in for keep their signatures
  assert len(_lib.SIGNATURES['tg_adam_step'][1]) == 13 and len(_lib.SIGNATURES['tg_adam_tick'][1]) == 6
  assert len(_lib.SIGNATURES['tg_adam_ema_step'][1]) == 13 and len(_lib.SIGNATURES['tg_ema_update'][1]) == 5


def test_refused_calls_without_gpu():
  """Argument validation happens before any launch."""
  from twingan_amd import _lib
  lib = _lib.load()
  assert lib.tg_nonfinite_check(None, 16, 16, None) == -1 and b'null' in lib.tg_last_error()
  assert lib.tg_nonfinite_check(16, 0, 16, None) == -1 and b'numel' in lib.tg_last_error()
  assert lib.tg_loss_scale_tick(16, 16, 16, 1e-4, 0.5, 0.99, 0, 2.0 ** 24, 1, None) == -1 and b'growth_interval' in lib.tg_last_error()


def test_adam_applies_prefers_the_device_count():
  """A checkpoint written under dynamic loss scaling carries the applies actually made; n_critic_counter counts the attempted
  ones, the beta powers come after both."""
  from twingan_amd import Config
  from twingan_amd import checkpoint as ckpt
  cfg = Config()
  arrays = {ckpt.ADAM_APPLIES_KEY: np.int64(7), 'n_critic_counter': np.int32(30), 'beta2_power': np.float32(cfg.adam_beta2 ** 20)}
  assert ckpt._adam_applies(arrays, cfg, 99) == 7
  del arrays[ckpt.ADAM_APPLIES_KEY]
  assert ckpt._adam_applies(arrays, cfg, 99) == 30
  del arrays['n_critic_counter']
  assert ckpt._adam_applies(arrays, cfg, 99) == 19
  assert ckpt.ADAM_APPLIES_KEY.startswith('twingan_amd/') and ckpt.LOSS_SCALE_PREFIX.startswith('twingan_amd/')
