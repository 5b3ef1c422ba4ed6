"""Host side of the moving averages (Config.moving_average_decay; model/model_inheritor.py:53-56,1063-1092,1150-1155): the
restore map of the eval branch and the flag's validation.  The kernels and the trainer are tests/test_gpu_ema.py's."""
import pytest
import torch

from twingan_amd import Config
from twingan_amd import checkpoint as ckpt
from twingan_amd.params import ParamStore, declare_twingan, is_model_variable

EMA = '/ExponentialMovingAverage'


def test_variables_to_restore_maps_model_variables_from_their_shadows():
  """tf.train.ExponentialMovingAverage.variables_to_restore over a declared store (self-attention and batch norm on, so that
  sa_gamma and non-trainable state are among the names): model variables -- state included -- are read from
  '<var>/ExponentialMovingAverage', sa_gamma from its own name; without moving_average the map is the identity."""
  cfg = Config(hw=16, max_ch=16, generator_norm_type='batch_norm', do_self_attention=True, self_attention_hw=8)
  store = declare_twingan(ParamStore(torch.device('cpu')), cfg)
  names = list(store.specs) + list(store.state_specs)
  gates = [k for k in names if k.endswith('/sa_gamma')]
  state = [k for k in store.state_specs if 'moving_mean' in k]
  assert gates and state and len(set(names)) == len(names)
  m = ckpt.variables_to_restore(names, True)
  assert sorted(m.values()) == sorted(names) and len(m) == len(names)
  for key, name in m.items():
    assert key == (name + EMA if is_model_variable(name) else name)
  for k in gates:
    assert m[k] == k and k + EMA not in m
  for k in state + ['generator/block_4x4x16/Conv/weights']:
    assert m[k + EMA] == k and k not in m
  assert ckpt.variables_to_restore(names, False) == {k: k for k in names}
  assert ckpt.variables_to_restore([], True) == {}


@pytest.mark.parametrize('v', [0.0, 1.0, -0.5, 1.5, 0, 1])
def test_moving_average_decay_outside_the_open_interval_is_refused(v):
  with pytest.raises(ValueError):
    Config(moving_average_decay=v)


def test_moving_average_decay_default_and_valid_values():
  assert Config().moving_average_decay is None
  assert Config(moving_average_decay=0.999).moving_average_decay == 0.999
  import dataclasses
  assert dataclasses.replace(Config(moving_average_decay=0.5), hw=32).moving_average_decay == 0.5
