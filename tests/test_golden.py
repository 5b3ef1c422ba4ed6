"""Golden fixtures (tests/golden/*.npz, written by tools/make_golden.py).

The twingan_*.npz model fixtures are REFERENCE-generated: one G+D step of the reference's own graph code
(the reference's twingan.py, image_generation.py, nets/pggan*.py, libs/*) executed on the TensorFlow-API stand-in of
oracle/tf_shim (oracle/ref_runner.py) -- weights, inputs, the reference's random draws, generated images, every loss
term, every gradient.  primitives.npz holds single TensorFlow ops restated in float64 NumPy (oracle/np_ops.py).

CPU (not gpu): the float64 oracle reproduces the reference's numbers to 1e-9 (this is what pins the oracle), the
float32 oracle within fp32 round-off; a second execution of the reference on the fixtures' weights and inputs (recorded
in tests/golden/reference/, oracle/recorded.py) must come out bit-identical.
GPU: the HIP path (fp32 direct kernels; bf16 MFMA kernels with a looser bound) hits the same vectors
through the C ABI.  Tolerances: fp32 primitives rel-L2 <= 1e-5; fp32 whole-network outputs rel-L2 <= 2e-5, losses 1e-4
relative, whole-model gradients rel-L2 <= 1e-2 (every variable of non-negligible norm <= 3e-2); bf16 outputs rel-L2 <= 5e-2, losses 5e-2.
"""
import os

import numpy as np
import pytest
import torch

from oracle import np_ops as N          # checker only
from oracle import torch_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
MODELS = {'twingan_hw16_c8': dict(hw=16, max_ch=8), 'twingan_hw64_c8': dict(hw=64, max_ch=8),
          'twingan_hw16_c8_growing': dict(hw=16, max_ch=8, is_growing=True, alpha_grow=0.3),
          'twingan_hw16_c8_hinge_eqlr_res': dict(hw=16, max_ch=8, loss='hinge', equalized=True, res_block=True),
          'twingan_hw16_c8_batch_norm': dict(hw=16, max_ch=8, norm='batch_norm'),
          'twingan_hw16_c8_style': dict(hw=16, max_ch=8, use_style_embedding=True, style_embed_size=8),
          'twingan_hw16_c8_style_bn': dict(hw=16, max_ch=8, use_style_embedding=True, style_embed_size=8,
                                           norm='batch_norm'),
          'twingan_hw16_c8_dragan': dict(hw=16, max_ch=8, loss='dragan'),
          'twingan_hw16_c16_sn_att': dict(hw=16, max_ch=16, spectral_norm=True, do_self_attention=True,
                                          self_attention_hw=8)}
# oracle Config field -> product Config field where the names differ
PRODUCT_FIELD = dict(loss='loss_architecture', equalized='equalized_learning_rate', res_block='use_res_block',
                     norm='generator_norm_type', sn_non_disc='spectral_norm_in_non_discriminator')


def product_kw(name):
  return {PRODUCT_FIELD.get(k, k): v for k, v in MODELS[name].items()}


def out_tol(name, k, tol):
  """The style encoder ends in an instance norm over ONE pixel (4x4 VALID conv output): in the reference's
  tf.nn.batch_normalization form x * inv + (beta - mean * inv), inv = gamma / sqrt(0 + 1e-6), the two ~1000 * x terms
  cancel, which costs fp32 ~1e-3 of the embedding -- and of the cycle images generated from it."""
  return 1e-2 if (name.endswith('_style') and 'cycle' in k) else tol


def oracle_cfg(name, g, dtype=torch.float32):
  cfg = R.Config(**MODELS[name])
  if 'in/style_noise' in g:
    cfg.style_noise = torch.from_numpy(g['in/style_noise']).to(dtype)
  if cfg.spectral_norm:      # the power-iteration vectors are non-trainable variables of the fixture
    cfg.sn_state = {k[len('param/'):]: torch.from_numpy(v).to(dtype) for k, v in g.items()
                    if k.startswith('param/') and k.endswith('/u')}
    cfg.sn_cache = {}
  return cfg


def grown(s, t, cfg):
  """The fixtures' end points are the reference's: at a growing stage its networks see the blended images
  (twingan.py:828-841)."""
  return (R.growing_image(s, cfg.alpha_grow), R.growing_image(t, cfg.alpha_grow)) if cfg.is_growing else (s, t)


def oracle_inputs(g, dtype):
  """(params, sources, targets, gp alphas, DRAGAN noise) of a model fixture as torch tensors of `dtype`."""
  P = {k[len('param/'):]: torch.from_numpy(v).to(dtype) for k, v in g.items()
       if k.startswith('param/') and not k.endswith('/u')}
  s, t = torch.from_numpy(g['in/sources']).to(dtype), torch.from_numpy(g['in/targets']).to(dtype)
  a_s = torch.from_numpy(g['in/gp_alpha_s']).to(dtype).reshape(-1, 1, 1, 1)
  a_t = torch.from_numpy(g['in/gp_alpha_t']).to(dtype).reshape(-1, 1, 1, 1)
  n_s = torch.from_numpy(g['in/dragan_noise_s']).to(dtype) if 'in/dragan_noise_s' in g else None
  n_t = torch.from_numpy(g['in/dragan_noise_t']).to(dtype) if 'in/dragan_noise_t' in g else None
  return P, s, t, a_s, a_t, n_s, n_t


def load(name):
  return dict(np.load(os.path.join(GOLD, name + '.npz')))


def rel_l2(a, b):
  a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
  assert a.shape == b.shape, (a.shape, b.shape)
  return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))


# ------------------------------------------------------------------------------------------------
# CPU: oracle vs its frozen vectors
# ------------------------------------------------------------------------------------------------
def test_numpy_oracle_reproduces_primitive_fixtures():
  g = load('primitives')
  for tag, k, pad, hw in (('c3', 3, 'SAME', 8), ('c1', 1, 'SAME', 8), ('c4', 4, 'VALID', 4), ('rgb', 1, 'SAME', 8)):
    assert rel_l2(N.conv2d(g[tag + '_x'], g[tag + '_w'], pad), g[tag + '_y']) < 1e-14
    assert rel_l2(N.conv2d_bwd_data(g[tag + '_gy'], g[tag + '_w'], (hw, hw), pad), g[tag + '_gx']) < 1e-14
    assert rel_l2(N.conv2d_bwd_weight(g[tag + '_x'], g[tag + '_gy'], (k, k), pad), g[tag + '_gw']) < 1e-14
  z = N.pixel_norm(N.leaky_relu(N.instance_norm(g['na_x'], g['na_gamma'], g['na_beta'])))
  assert rel_l2(z, g['na_z']) < 1e-14
  assert rel_l2(N.minibatch_state_concat(g['mb_x']), g['mb_y']) < 1e-14
  assert abs(N.absolute_difference(g['l_a'], g['l_b'], 0.7) - float(g['l_abs'])) < 1e-15
  assert abs(N.gradient_penalty(g['gp_g'], 10.0) - float(g['gp'])) < 1e-12
  th, m, v = g['adam_theta0'].copy(), np.zeros(64), np.zeros(64)
  for t in range(3):
    th, m, v = N.adam_step(th, g['adam_g'][t], m, v, t + 1)
  assert rel_l2(th, g['adam_theta3']) < 1e-15


@pytest.mark.parametrize('name', sorted(MODELS))
def test_oracle_f64_matches_the_reference(name):
  """THE PIN: every loss term and every gradient of the float64 oracle against the numbers the reference's own code
  produced for the same weights, inputs and random draws."""
  g = load(name)
  cfg = oracle_cfg(name, g, torch.float64)
  P, s, t, a_s, a_t, n_s, n_t = oracle_inputs(g, torch.float64)
  with torch.no_grad():
    o = R.forward_generators(P, *grown(s, t, cfg), cfg)
    for k in ('es', 's_prime', 't_prime', 's_cycle', 't_cycle'):
      assert np.abs(o[k].numpy() - g['fwd/' + k]).max() < 1e-9, k
    assert np.abs(R.discriminator(P, grown(s, t, cfg)[0], cfg, 'discriminator_s')[0].numpy() - g['fwd/d_s_real']).max() < 1e-9
  cfg.sn_cache = {}      # normalised kernels cached under no_grad carry no graph
  for v in P.values():
    v.requires_grad_(True)
  gl, gterms = R.generator_loss(P, s, t, cfg)
  dl, dterms = R.discriminator_loss(P, s, t, cfg, a_s, a_t, n_s, n_t)
  for grp, total, terms in (('g', gl, gterms), ('d', dl, dterms)):
    assert abs(float(total) - float(g['loss/%s_total' % grp])) < 1e-9
    assert {'loss/%s/%s' % (grp, k) for k in terms} == {k for k in g if k.startswith('loss/%s/' % grp)}
    for k, v in terms.items():
      assert abs(float(v) - float(g['loss/%s/%s' % (grp, k)])) < 1e-9, k
  grads = dict(R.grads_of(gl, P, R.generator_var_names(P)))
  grads.update(R.grads_of(dl, P, R.discriminator_var_names(P)))
  assert set(grads) == {k[len('grad/'):] for k in g if k.startswith('grad/')} == set(P)
  scale = max(float(np.abs(g['grad/' + k]).max()) for k in grads)
  for k, v in grads.items():
    assert np.abs(v.detach().numpy() - g['grad/' + k]).max() < 1e-9 * scale, k
  if cfg.spectral_norm:      # libs/sn.py:84-86: what the run leaves in u
    R.end_run(cfg)
    for k, v in cfg.sn_state.items():
      assert np.abs(v.numpy() - g['state_after/' + k]).max() < 1e-12, k


@pytest.mark.parametrize('name', ['twingan_hw16_c8', 'twingan_hw16_c16_sn_att'])
def test_fixtures_are_what_the_reference_computes(name):
  """The reference's graph code (oracle/ref_runner.py) run again on the fixture's weights and inputs, as recorded in
  tests/golden/reference/ (oracle/recorded.py)."""
  from oracle import ref_runner
  from oracle.recorded import own_gradients, replay
  g = load(name)
  cfg = R.Config(**MODELS[name])
  preset = {k[len('param/'):]: v for k, v in g.items() if k.startswith('param/')}
  ref = replay('fixture_' + name, ref_runner.run, ref_runner.flags_of(cfg), g['in/sources'], g['in/targets'],
               global_step=ref_runner.global_step_of(cfg), seed=0, preset=preset, prune=own_gradients)
  assert set(ref['variables']) - {'global_step'} == set(preset)      # the reference creates exactly these variables
  assert abs(ref['g_loss'] - float(g['loss/g_total'])) < 1e-12 and abs(ref['d_loss'] - float(g['loss/d_total'])) < 1e-12
  for grp in 'gd':
    for k, v in ref[grp + '_terms'].items():
      assert abs(v - float(g['loss/%s/%s' % (grp, ref_runner.term_name(k))])) < 1e-12, k
    for k, v in ref[grp + '_grads'].items():
      if 'grad/' + k in g and (grp == 'd') == k.startswith('discriminator'):
        assert np.abs(v - g['grad/' + k]).max() < 1e-12, k


@pytest.mark.parametrize('name', sorted(MODELS))
def test_torch_oracle_fp32_reproduces_model_fixtures(name):
  g = load(name)
  cfg = oracle_cfg(name, g)
  P, s, t, a_s, a_t, n_s, n_t = oracle_inputs(g, torch.float32)
  with torch.no_grad():
    o = R.forward_generators(P, *grown(s, t, cfg), cfg)
  for k in ('es', 's_prime', 't_prime', 's_cycle', 't_cycle'):
    assert rel_l2(o[k].numpy(), g['fwd/' + k]) < out_tol(name, k, 2e-5), k
  for v in P.values():
    v.requires_grad_(True)
  dl, terms = R.discriminator_loss(P, s, t, cfg, a_s, a_t, n_s, n_t)
  assert abs(float(dl) - float(g['loss/d_total'])) < 1e-4 * max(1.0, abs(float(g['loss/d_total'])))
  for k, v in terms.items():
    assert abs(float(v) - float(g['loss/d/' + k])) < 1e-4 * max(1.0, abs(float(g['loss/d/' + k]))), k
  grads = R.grads_of(dl, P, R.discriminator_var_names(P))
  num = sum(float(((grads[k].double().numpy() - g['grad/' + k]) ** 2).sum()) for k in grads)
  den = sum(float((g['grad/' + k] ** 2).sum()) for k in grads)
  assert (num / den) ** 0.5 < 3e-3      # fp32 round-off through the GP double backward (1e-3 at 64x64)


def test_oracle_training_runs_match_the_reference():
  """tests/golden/train4_hw16_c8.npz: four consecutive session.run(train_op) of the reference's training graph
  (GanModel._add_optimization, image_generation.py:587-662, with Adam from the flags) -- the oracle's train_step must
  leave every variable where the reference left it, and the product's host counters must move the same way."""
  g = load('train4_hw16_c8')
  cfg = R.Config(hw=16, max_ch=8, lr=float(g['meta/lr']), beta1=float(g['meta/beta1']), beta2=float(g['meta/beta2']),
                 adam_eps=float(g['meta/eps']))
  P = {k[len('param/'):]: torch.from_numpy(v).clone() for k, v in g.items() if k.startswith('param/')}      # updated in place
  opt = R.AdamState(P, cfg)
  from twingan_amd import Config
  from twingan_amd.twingan import Trainer
  tr = Trainer(Config(hw=8, max_ch=8), device='cpu')      # host-side counters only
  tr.g_step = lambda s, t: None
  tr.d_step = lambda s, t, a=None, b=None: None
  for i in range(4):
    before = (tr.n_critic_counter, tr.global_step)
    tr.run(None, None)
    assert list(g['run%d/counters' % i]) == [before[0], before[1], tr.n_critic_counter, tr.global_step], i
    out = R.train_step(P, opt, torch.from_numpy(g['run%d/sources' % i]), torch.from_numpy(g['run%d/targets' % i]), cfg,
                       torch.from_numpy(g['run%d/gp_alpha_s' % i]).reshape(-1, 1, 1, 1),
                       torch.from_numpy(g['run%d/gp_alpha_t' % i]).reshape(-1, 1, 1, 1), i)
    assert ('g_loss' in out) == (i % 2 == 0)                       # G apply on even runs, D apply on odd ones
    if 'd_loss' in out:
      assert abs(out['d_loss'] - float(g['run%d/d_loss' % i])) < 1e-9
  for k, v in P.items():
    assert np.abs(v.detach().numpy() - g['after/' + k]).max() < 1e-12, k
  moved = max(np.abs(g['after/' + k] - g['param/' + k]).max() for k in P)
  assert moved > 1e-3                                              # the runs really trained
  assert abs(float(g['after_opt/beta1_power']) - cfg.beta1 ** 5) < 1e-15      # one shared pair of powers, 4 applies


def test_cycle_gan_term_only_from_64():
  """twingan.py:466: the fixtures themselves encode the rule."""
  assert not any('cycle' in k for k in load('twingan_hw16_c8') if k.startswith('loss/d/'))
  assert any('cycle' in k for k in load('twingan_hw64_c8') if k.startswith('loss/d/'))


# ------------------------------------------------------------------------------------------------
# GPU: HIP path vs the frozen vectors
# ------------------------------------------------------------------------------------------------
def _dev(a, dtype=torch.float32):
  return torch.from_numpy(np.ascontiguousarray(a)).float().to('cuda:0').to(dtype).contiguous()


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_gpu_primitives_hit_golden(dtype):
  from twingan_amd import ops
  g = load('primitives')
  tol = 1e-5 if dtype == torch.float32 else 1.5e-2
  for tag, k, pad in (('c3', 3, 'SAME'), ('c1', 1, 'SAME'), ('c4', 4, 'VALID')):
    x, w = _dev(g[tag + '_x'], dtype).requires_grad_(True), _dev(g[tag + '_w']).requires_grad_(True)
    y = ops.conv2d(x, w, None, k, pad)
    assert rel_l2(y.detach().float().cpu().numpy(), g[tag + '_y']) < tol, tag
    y.backward(_dev(g[tag + '_gy'], dtype))
    assert rel_l2(x.grad.float().cpu().numpy(), g[tag + '_gx']) < tol, tag
    assert rel_l2(w.grad.cpu().numpy(), g[tag + '_gw']) < tol, tag
  x, w = _dev(g['rgb_x'], dtype), _dev(g['rgb_w'])
  assert rel_l2(ops.pointwise_conv(x, w).float().cpu().numpy(), g['rgb_y']) < tol
  z = ops.norm_act(_dev(g['na_x'], dtype), _dev(g['na_gamma']), _dev(g['na_beta']))
  assert rel_l2(z.float().cpu().numpy(), g['na_z']) < (1e-5 if dtype == torch.float32 else 1e-2)
  z = ops.norm_act(_dev(g['na_x'], dtype), _dev(g['na_gamma']), _dev(g['na_beta']), lrelu=False, pixel_norm=False)
  assert rel_l2(z.float().cpu().numpy(), g['na_z_rgb']) < (1e-5 if dtype == torch.float32 else 1e-2)
  up = ops.upsample2x_concat(_dev(g['rs_x'], dtype))
  assert rel_l2(up.float().cpu().numpy(), g['rs_up']) < (1e-7 if dtype == torch.float32 else 4e-3)
  if dtype == torch.float32:
    mb = ops.minibatch_state_concat(_dev(g['mb_x']), 24)
    assert rel_l2(mb[..., :17].cpu().numpy(), g['mb_y']) < 1e-6
    assert float(mb[..., 17:].abs().max()) == 0.0
    la = ops.abs_diff_mean(_dev(g['l_a']), _dev(g['l_b']), 0.7)
    assert abs(la.item() - float(g['l_abs'])) < 1e-6
    gp = ops.gradient_penalty(_dev(g['gp_g']), 10.0)
    assert abs(gp.item() - float(g['gp'])) < 1e-5 * float(g['gp'])


@pytest.mark.gpu
def test_gpu_training_runs_hit_the_reference():
  """The HIP path (fp32, eager) through the four training runs of tests/golden/train4_hw16_c8.npz: same inputs and
  alphas, Adam on the device; compares the UPDATE of every variable with the reference's (aggregate rel-L2 <= 5e-2,
  median per variable <= 3e-2 -- Adam's first steps are sign-like, so a near-zero gradient may flip)."""
  from twingan_amd import Config
  from twingan_amd import twingan as T
  g = load('train4_hw16_c8')
  cfg = Config(hw=16, max_ch=8, precision='fp32', learning_rate=float(g['meta/lr']), adam_beta1=float(g['meta/beta1']),
               adam_beta2=float(g['meta/beta2']), opt_epsilon=float(g['meta/eps']))
  tr = T.Trainer(cfg, device='cuda:0', seed=0, use_graph=False)
  tr.store.load_state_dict({k[len('param/'):]: torch.from_numpy(v).float() for k, v in g.items() if k.startswith('param/')})
  for i in range(4):
    tr.run(_dev(g['run%d/sources' % i]), _dev(g['run%d/targets' % i]), _dev(g['run%d/gp_alpha_s' % i]),
           _dev(g['run%d/gp_alpha_t' % i]))
    assert [tr.n_critic_counter, tr.global_step] == list(g['run%d/counters' % i][2:])
  sd = tr.store.state_dict()
  num = den = 0.0
  per_var = []
  for k in sd:
    d_dev = sd[k].double().cpu().numpy() - g['param/' + k]
    d_ref = g['after/' + k] - g['param/' + k]
    num += float(((d_dev - d_ref) ** 2).sum())
    den += float((d_ref ** 2).sum())
    if np.abs(d_ref).max() > 0:
      per_var.append(float(np.linalg.norm(d_dev - d_ref) / (np.linalg.norm(d_ref) + 1e-30)))
  assert np.sqrt(num / den) < 5e-2, np.sqrt(num / den)
  assert np.median(per_var) < 3e-2, np.median(per_var)


@pytest.mark.gpu
@pytest.mark.parametrize('name,precision', [('twingan_hw16_c8', 'fp32'), ('twingan_hw64_c8', 'fp32'),
                                            ('twingan_hw16_c8_growing', 'fp32'), ('twingan_hw64_c8', 'bf16'),
                                            ('twingan_hw16_c8_hinge_eqlr_res', 'fp32'),
                                            ('twingan_hw16_c8_batch_norm', 'fp32'), ('twingan_hw16_c8_style', 'fp32'),
                                            ('twingan_hw16_c8_dragan', 'fp32'), ('twingan_hw16_c16_sn_att', 'fp32'),
                                            ('twingan_hw16_c8_style_bn', 'fp32')])
def test_gpu_model_hits_golden(name, precision):
  from twingan_amd import Config
  from twingan_amd import twingan as T
  g = load(name)
  cfg = Config(precision=precision, **product_kw(name))
  tr = T.Trainer(cfg, device='cuda:0', seed=0)
  noise = _dev(g['in/style_noise']) if 'in/style_noise' in g else None
  tr.store.load_state_dict({k[len('param/'):]: torch.from_numpy(v).float() for k, v in g.items()
                            if k.startswith('param/')})
  adt = torch.bfloat16 if precision == 'bf16' else torch.float32
  s, t = _dev(g['in/sources'], adt), _dev(g['in/targets'], adt)
  a_s, a_t = _dev(g['in/gp_alpha_s']), _dev(g['in/gp_alpha_t'])
  n_s = _dev(g['in/dragan_noise_s'], adt) if 'in/dragan_noise_s' in g else None
  n_t = _dev(g['in/dragan_noise_t'], adt) if 'in/dragan_noise_t' in g else None
  # whole-model fp32 gradients: 1e-6 .. 5e-3 from the fp64 vectors (the 64x64 graph is ill-conditioned: the fp32
  # torch oracle itself is 1e-3 from the fp64 one).  The graph has discontinuities (LeakyReLU masks, L1 signs), but
  # every forward statistic is summed in a fixed order (norm.hip), so there is no run-to-run flip of a unit near
  # zero any more (round 1: 5 of 40 runs at 2.7e-2, hence 8e-2 then).  Aggregate 1e-2, every variable 3e-2.
  otol, ltol, gtol = (2e-5, 1e-4, 1e-2) if precision == 'fp32' else (5e-2, 5e-2, None)
  vtol = 3 * gtol if gtol else None
  if name.endswith('_style'):
    # the style encoder's last layer is an instance norm over ONE pixel (out_tol above): its 1000 * x cancellation
    # costs any fp32 evaluation 1e-3 of the embedding, which flips low-resolution LeakyReLU units of the cycle passes.
    # Measured on this fixture: the plain fp32 torch oracle is 6.58e-2 (worst variable 0.50) from the float64
    # vectors, the fp32 HIP path 6.58e-2 (tools/golden_grad_report.py) -- the bound is what fp32 can do here
    gtol, vtol = 1e-1, None
  with torch.no_grad():
    gs, gt = (T.get_growing_image(s, cfg.alpha_grow), T.get_growing_image(t, cfg.alpha_grow)) if cfg.is_growing else (s, t)
    o = T.forward_generators(tr.P, gs, gt, cfg, noise)
  for k in ('es', 's_prime', 't_prime', 's_cycle', 't_cycle'):
    # bf16 at 8 channels: the fp64 oracle with bf16 storage rounding (tools/bf16_sensitivity.py) predicts rel-L2
    # 0.038 for the encoder output and 0.12-0.20 for the generator outputs (instance-normalised to_rgb); the
    # kernels measure 0.039 / 0.18.  Tight bf16 bounds live in the per-primitive tests.
    tol = out_tol(name, k, otol) if precision == 'fp32' else (0.06 if k == 'es' else 0.3)
    assert rel_l2(o[k].float().cpu().numpy(), g['fwd/' + k]) < tol, k
  for group, fn, args in (('g', T.generator_loss, (s, t, cfg, noise)), ('d', T.discriminator_loss, (s, t, cfg, a_s, a_t, n_s, n_t, noise))):
    tr.store.zero_grad(group)
    tr._set_requires_grad(g=group == 'g', d=group == 'd')
    # both losses belong to ONE reference run: same pre-run spectral-norm u for both (so no end_run() in between),
    # but the normalised kernels cached by the other pass were built without a graph to this pass's variables
    tr.P.__dict__.get('sn_cache', {}).clear()
    loss, terms = fn(tr.P, *args)
    want = float(g['loss/%s_total' % group])
    assert abs(loss.item() - want) < ltol * max(1.0, abs(want)) + (0.0 if precision == 'fp32' else 5e-2), (group, loss.item(), want)
    if precision == 'fp32':
      for k, v in terms.items():
        w = float(g['loss/%s/%s' % (group, k)])
        assert abs(v.item() - w) < ltol * max(1.0, abs(w)), (k, v.item(), w)
    if precision != 'fp32':
      continue          # whole-model bf16 gradients are chaotic at 8 channels (tools/bf16_sensitivity.py: rel-L2 1.2)
    loss.backward()
    gd = tr.store.grad_dict()
    names = tr.store.names(group)
    num = sum(float(((gd[k].double().cpu().numpy() - g['grad/' + k]) ** 2).sum()) for k in names)
    den = sum(float((g['grad/' + k] ** 2).sum()) for k in names)
    assert (num / den) ** 0.5 < gtol, (group, (num / den) ** 0.5)
    top = max(float(np.linalg.norm(g['grad/' + k])) for k in names)
    for k in names if vtol else ():      # ... and no single variable hides in the aggregate
      nb = float(np.linalg.norm(g['grad/' + k]))
      if nb >= 1e-3 * top:
        e = float(np.linalg.norm(gd[k].double().cpu().numpy() - g['grad/' + k])) / nb
        assert e < vtol, (group, k, e)


# ------------------------------------------------------------------------------------------------
# BASELINE configs[0]: the plain PGGAN trainer (image_generation.GanModel), reference-generated fixtures
# ------------------------------------------------------------------------------------------------
PGGAN_MODELS = {'pggan_hw4_c16': dict(hw=4, max_ch=16, norm='batch_norm'),
                'pggan_hw8_c16_in': dict(hw=8, max_ch=16, norm='instance_norm'),
                'pggan_hw8_c16_hinge_grow': dict(hw=8, max_ch=16, norm='batch_norm', loss='hinge', is_growing=True,
                                                 alpha_grow=0.3)}


def _pggan_inputs(g, dtype):
  P = {k[len('param/'):]: torch.from_numpy(v).to(dtype) for k, v in g.items() if k.startswith('param/')}
  t = torch.from_numpy(g['in/targets']).to(dtype)
  noise = torch.from_numpy(g['in/noise']).to(dtype)
  alpha = torch.from_numpy(g['in/gp_alpha']).to(dtype).reshape(-1, 1, 1, 1)
  return P, t, noise, alpha


@pytest.mark.parametrize('name', sorted(PGGAN_MODELS))
def test_pggan_oracle_f64_matches_the_reference(name):
  """THE PIN for configs[0]: the float64 oracle against what image_generation.GanModel._clone_fn computed
  (oracle/ref_runner.run_pggan, tools/make_golden.py --pggan): generated images, every loss term, every gradient."""
  g = load(name)
  cfg = R.Config(use_unet=False, **PGGAN_MODELS[name])
  P, t, noise, alpha = _pggan_inputs(g, torch.float64)
  with torch.no_grad():
    out, _ = R.generator(P, noise, '', cfg, None, 'generator')
    assert np.abs(out.numpy() - g['fwd/generator_output']).max() < 1e-9
  for v in P.values():
    v.requires_grad_(True)
  gl, gt = R.pggan_generator_loss(P, t, cfg, noise)
  dl, dt = R.pggan_discriminator_loss(P, t, cfg, noise, alpha)
  assert {'loss/g/' + k for k in gt} | {'loss/d/' + k for k in dt} == {k for k in g if k.startswith(('loss/g/', 'loss/d/'))}
  for grp, terms in (('g', gt), ('d', dt)):
    for k, v in terms.items():
      assert abs(float(v) - float(g['loss/%s/%s' % (grp, k)])) < 1e-9, k
  grads = dict(R.grads_of(gl, P, [k for k in P if k.startswith('generator')]))
  grads.update(R.grads_of(dl, P, [k for k in P if k.startswith('discriminator')]))
  assert set(grads) == {k[len('grad/'):] for k in g if k.startswith('grad/')}
  scale = max(float(np.abs(g['grad/' + k]).max()) for k in grads)
  for k, v in grads.items():
    assert np.abs(v.detach().numpy() - g['grad/' + k]).max() < 1e-9 * scale, k


@pytest.mark.parametrize('name', sorted(PGGAN_MODELS))
def test_pggan_product_declares_the_reference_variables(name):
  from twingan_amd import Config
  from twingan_amd.params import ParamStore, declare_pggan
  g = load(name)
  st = declare_pggan(ParamStore('cpu'), Config(**product_kw_of(PGGAN_MODELS[name]))).build(0)
  want = {k[len('param/'):]: v.shape for k, v in g.items() if k.startswith('param/')}
  assert {k: tuple(s['shape']) for k, s in st.specs.items()} == {k: tuple(v) for k, v in want.items()}


def product_kw_of(kw):
  return {PRODUCT_FIELD.get(k, k): v for k, v in kw.items()}


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(PGGAN_MODELS))
def test_gpu_pggan_trainer_hits_golden(name):
  """The HIP path (fp32) of the plain PGGAN trainer -- latent noise through the 4x4 VALID first conv, one
  discriminator, add_gan_loss -- against the reference-generated vectors: image, loss terms, every gradient."""
  from twingan_amd import Config
  from twingan_amd import image_generation as IG
  g = load(name)
  cfg = Config(precision='fp32', **product_kw_of(PGGAN_MODELS[name]))
  tr = IG.PgganTrainer(cfg, device='cuda:0', seed=0)
  tr.store.load_state_dict({k[len('param/'):]: torch.from_numpy(v).float() for k, v in g.items() if k.startswith('param/')})
  t, noise, alpha = _dev(g['in/targets']), _dev(g['in/noise']), _dev(g['in/gp_alpha'])
  with torch.no_grad():
    out = IG.generate(tr.P, noise, cfg)
  assert rel_l2(out.float().cpu().numpy(), g['fwd/generator_output']) < 2e-5
  for group, fn, args in (('g', IG.generator_loss, (t, cfg, noise)), ('d', IG.discriminator_loss, (t, cfg, noise, alpha))):
    tr.store.zero_grad(group)
    tr._set_requires_grad(g=group == 'g', d=group == 'd')
    loss, terms = fn(tr.P, *args)
    for k, v in terms.items():
      w = float(g['loss/%s/%s' % (group, k)])
      assert abs(v.item() - w) < 1e-4 * max(1.0, abs(w)), (k, v.item(), w)
    loss.backward()
    gd = tr.store.grad_dict()
    names = tr.store.names(group)
    num = sum(float(((gd[k].double().cpu().numpy() - g['grad/' + k]) ** 2).sum()) for k in names)
    den = sum(float((g['grad/' + k] ** 2).sum()) for k in names)
    assert (num / den) ** 0.5 < 1e-2, (group, (num / den) ** 0.5)
  # and the alternating step runs (device-drawn noise), eagerly and from the captured graphs
  for use_graph in (False, True):
    tr2 = IG.PgganTrainer(Config(precision='bf16', **product_kw_of(PGGAN_MODELS[name])), device='cuda:0', seed=1,
                          use_graph=use_graph and not cfg.is_growing)
    tb = t.to(torch.bfloat16)
    losses = [tr2.run(None, tb)[0].item() for _ in range(4)]
    assert all(np.isfinite(losses)), losses


# ------------------------------------------------------------------------------------------------
# the inference branch (twingan.py:300-363; inference/image_translation_infer.py): is_training=False
# ------------------------------------------------------------------------------------------------
INFER_NORMS = ('instance_norm', 'batch_norm', 'batch_renorm')


def _infer_state(g):
  P = {k[len('param/'):]: torch.from_numpy(v) for k, v in g.items() if k.startswith('param/') and '/moving_' not in k}
  state = {k[len('param/'):]: torch.from_numpy(v) for k, v in g.items() if k.startswith('param/') and '/moving_' in k}
  return P, state


@pytest.mark.parametrize('norm', INFER_NORMS)
def test_oracle_inference_branch_matches_the_reference(norm):
  """`sources_ph -> custom_generated_t_style_source` and `targets_ph -> custom_generated_s_style_target` as the
  reference's graph computed them with fed placeholders and preset moving statistics (tools/make_golden.py --infer)."""
  g = load('infer_hw16_c8_' + norm)
  P, state = _infer_state(g)
  cfg = R.Config(hw=16, max_ch=8, norm=norm, bn_state=state)
  with torch.no_grad():
    assert np.abs(R.translate(P, torch.from_numpy(g['in/sources_ph']), cfg, 't').numpy() -
                  g['out/custom_generated_t_style_source']).max() < 1e-9
    assert np.abs(R.translate(P, torch.from_numpy(g['in/targets_ph']), cfg, 's').numpy() -
                  g['out/custom_generated_s_style_target']).max() < 1e-9


@pytest.mark.gpu
@pytest.mark.parametrize('norm', INFER_NORMS)
@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_gpu_inference_branch_hits_golden(norm, precision):
  """twingan.translate / inference.ImageInferer on the HIP kernels (BatchNorm through the fused kernel's per-image-row
  mode on the MOVING statistics) against the reference's inference outputs; uint8 input through the TF-1.8 resize."""
  from twingan_amd import Config
  from twingan_amd.inference import ImageInferer
  g = load('infer_hw16_c8_' + norm)
  sd = {k[len('param/'):]: torch.from_numpy(v).float() for k, v in g.items() if k.startswith('param/')}
  cfg = Config(hw=16, max_ch=8, precision=precision, generator_norm_type=norm)
  tol = 2e-5 if precision == 'fp32' else 0.25      # bf16 at 8 channels: see test_gpu_model_hits_golden
  for name, key in (('custom_generated_t_style_source', 'in/sources_ph'), ('custom_generated_s_style_target', 'in/targets_ph')):
    inf = ImageInferer(cfg, sd, device='cuda:0', output_tensor_name=name)
    out = inf.infer(g[key].astype(np.float32))
    assert out.shape == g['out/' + name].shape
    assert rel_l2(out / 255.0, g['out/' + name]) < tol, (name, rel_l2(out / 255.0, g['out/' + name]))
  # uint8 images of another size: convert_image_dtype + resize_images in front of the same graph
  u8 = (np.random.RandomState(0).rand(1, 24, 20, 3) * 255).astype(np.uint8)
  out = inf.infer(u8[0])
  assert out.shape == (1, 16, 16, 3) and np.isfinite(out).all()
