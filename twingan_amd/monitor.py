"""Training summaries and sample grids: what the reference's slim.learning.train writes while a stage trains.

  * TensorBoard summaries every --save_summaries_secs (model/model_inheritor.py:1094-1126): a histogram of every variable
    (:1056-1058), of every gradient and of its norm (deployment/model_deploy.py:506-530, image_generation.py:611-619),
    ``activations/<end point>`` and ``sparsity/<end point>`` (model_inheritor.py:721-726), the loss terms, ``generator_loss``,
    ``discriminator_loss``, ``learning_rate`` and ``gdrop_strength`` (:747-749,1094; image_generation.py:585,611-613);
  * sample grids every --log_image_every_n_iter global steps under <train_dir>/generated_samples/ (twingan.py:606-678,
    image_generation.py:694-714, util_io.py:121-142).

Both are computed on the device: the statistics and TensorFlow histograms of all variables and gradients come from
ops.tensor_summaries over the ParamStore's flat buffers (a few launches over job tables built once), a grid is one
ops.image_grid launch.  A read-out is ONE device-to-host copy -- the only synchronisation -- and the monitor adds nothing to
the captured step graphs: it reads between runs and leaves every tensor a run reads exactly as it found it.

This project's names and additions: loss terms are ``losses/<term>`` under Trainer.run's term names (the TF op names are not
recoverable); ``loss_scale/<group>`` under dynamic loss scaling; ``nonfinite/<tag>`` where a tensor holds NaN or inf (TF raises
there; here they are counted and left out of the histogram).  The end points that exist as tensors here are the six images and
the two encoder contents; the fused kernels never materialise the others.
"""
import math
import os
import struct
import time
import zlib

import numpy as np
import torch

from . import ops, summary

END_POINTS = ('sources', 'targets', 's_prime_output', 't_prime_output', 's_cycle_output', 't_cycle_output',
              'encoded_source_content_before_classification', 'encoded_target_content_before_classification')
_IMAGES = (('source', 'sources'), ('target', 'targets'), ('s_prime', 's_prime_output'), ('t_prime', 't_prime_output'),
           ('s_cycle', 's_cycle_output'), ('t_cycle', 't_cycle_output'))
# twingan.py:667-668 pairs image_list[0] (sources) with [3] (t') under the name 'target_s_prime' and [1] (targets) with [2]
# (s') under 'source_t_prime': the reference's file names, kept with their quirk
_INTERLEAVED = (('target_s_prime', 'sources', 't_prime_output'), ('source_t_prime', 'targets', 's_prime_output'))
LOSS_TAG = {'g': 'generator_loss', 'd': 'discriminator_loss'}


def png_bytes(img):
  """PNG file of a uint8 array [h, w, 3]: colour type 2, 8 bit, every row with filter 0."""
  img = np.ascontiguousarray(img, dtype=np.uint8)
  assert img.ndim == 3 and img.shape[2] == 3, img.shape
  h, w = img.shape[:2]
  raw = np.concatenate([np.zeros((h, 1), np.uint8), img.reshape(h, w * 3)], axis=1).tobytes()

  def chunk(kind, data):
    return struct.pack('>I', len(data)) + kind + data + struct.pack('>I', zlib.crc32(kind + data) & 0xffffffff)
  return (b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, 8, 2, 0, 0, 0)) +
          chunk(b'IDAT', zlib.compress(raw, 6)) + chunk(b'IEND', b''))


def write_png(path, img):
  with open(path, 'wb') as fh:
    fh.write(png_bytes(img))


class Monitor:
  """monitor = Monitor(sample_fn); monitor.begin(trainer, train_dir, batch_size); after every global step
  monitor.step(trainer, global_step); monitor.end().  runner.run_progressive(..., monitor=) does exactly that per stage.

  ``sample_fn(hw, batch)`` -> (sources, targets): the batches of the sample pass (activations, grids); None: neither.
  Summaries are due every ``save_summaries_secs`` seconds, or every ``save_summaries_steps`` global steps when that is set;
  grids whenever global_step % log_image_every_n_iter == 0, step 0 included."""

  def __init__(self, sample_fn=None, save_summaries_secs=120, save_summaries_steps=None, log_image_every_n_iter=1000,
               log_image_n_per_hw=8, seed=0):
    self.sample_fn = sample_fn
    self.save_summaries_secs = save_summaries_secs
    self.save_summaries_steps = save_summaries_steps
    self.log_image_every_n_iter = log_image_every_n_iter
    self.log_image_n_per_hw = int(log_image_n_per_hw)
    self._gen = torch.Generator().manual_seed(seed)      # the random style embedding of the sample pass: never torch's global RNG
    self.writer = None
    self.trainer = None

  # ---- per stage --------------------------------------------------------------------------------------------------
  def begin(self, trainer, train_dir, batch_size=None):
    """Opens the stage's event file in ``train_dir`` and builds the job tables over the trainer's flat buffers (their
    addresses hold for the trainer's life)."""
    from .image_generation import PgganTrainer
    self.end()
    self.trainer, self.train_dir, self.batch_size = trainer, train_dir, batch_size
    self.twin = not isinstance(trainer, PgganTrainer)      # the TwinGAN end points and grids
    self.writer = summary.EventWriter(train_dir)
    self._last_summary = time.time()
    s = trainer.store
    self.names = {g: [k for k, sp in s.specs.items() if sp['group'] == g] for g in s.GROUPS}
    with self._device():
      self._var_tables, self._grad_tables = {}, {}
      for g in s.GROUPS:
        entries = [(s.offsets[k], s.specs[k]['shape'], s.specs[k]['phys']) for k in self.names[g]]
        if entries:
          self._var_tables[g] = ops.SummaryTable.of_flat(s.flat[g], entries)
          self._grad_tables[g] = ops.SummaryTable.of_flat(s.grad[g], entries)
    self._limits = ops.summary_limits()[0]
    return self

  def end(self):
    if self.writer is not None:
      self.writer.close()
    self.writer = self.trainer = None
    self._var_tables = self._grad_tables = None

  def _device(self):
    import contextlib
    dev = self.trainer.device
    return torch.cuda.device(dev) if dev.type == 'cuda' else contextlib.nullcontext()

  def step(self, trainer, global_step):
    """Called between runs, after global step ``global_step`` is complete (0: before the first)."""
    assert trainer is self.trainer, 'Monitor.begin() was given another trainer'
    n = self.log_image_every_n_iter
    if n and self.twin and self.sample_fn is not None and global_step % n == 0:
      self.write_grids(global_step)
    if trainer.last_run is not None:
      if self.save_summaries_steps:
        due = global_step % self.save_summaries_steps == 0
      else:
        due = bool(self.save_summaries_secs) and time.time() - self._last_summary >= self.save_summaries_secs
      if due:
        self.write_summaries(global_step)

  # ---- the sample pass --------------------------------------------------------------------------------------------
  def _forward(self, count):
    """``count`` forward runs of the training graph's generators under no_grad on batches of sample_fn; everything such a
    forward writes besides its outputs -- BatchNorm moving and renorm statistics, spectral-norm u and the per-run normalised
    kernels, the device draw counter -- is put back, so the next run starts from the same bits as without the monitor."""
    from . import twingan
    tr = self.trainer
    cfg, P = tr.cfg, tr.P
    for name in ('sn_cache', 'sn_pending', 'sn_leaves'):
      assert not P.__dict__.get(name), 'the monitor reads between runs, not inside one'
    state = {k: v.clone() for k, v in tr.store.state.items()}
    draws = tr._rng_state.clone()
    outs = []
    dt = twingan.act_dtype(cfg)
    try:
      with torch.no_grad():
        for _ in range(count):
          s, t = self.sample_fn(cfg.hw, self.batch_size)[:2]
          s, t = s.to(device=tr.device, dtype=dt), t.to(device=tr.device, dtype=dt)
          if cfg.is_growing:
            s, t = twingan.get_growing_image(s, cfg.alpha_grow), twingan.get_growing_image(t, cfg.alpha_grow)
          noise = None
          if cfg.use_style_embedding:
            noise = torch.randn(s.shape[0], cfg.style_embed_size, generator=self._gen, dtype=torch.float32).to(tr.device)
          o = twingan.forward_generators(P, s, t, cfg, style_noise=noise)
          outs.append({'sources': s.contiguous(), 'targets': t.contiguous(),
                       's_prime_output': o['s_prime'].contiguous(), 't_prime_output': o['t_prime'].contiguous(),
                       's_cycle_output': o['s_cycle'].contiguous(), 't_cycle_output': o['t_cycle'].contiguous(),
                       'encoded_source_content_before_classification': o['es'].contiguous(),
                       'encoded_target_content_before_classification': o['et'].contiguous()})
    finally:
      with torch.no_grad():
        for k, v in state.items():
          tr.store.state[k].copy_(v)
        tr._rng_state.copy_(draws)
      for name in ('sn_cache', 'sn_pending', 'sn_leaves'):      # u' is dropped unassigned: the next run iterates from u again
        d = P.__dict__.get(name)
        if d:
          d.clear()
    return outs

  def write_grids(self, global_step):
    """<train_dir>/generated_samples/<step>_{source,target,s_prime,t_prime,s_cycle,t_cycle}.png: log_image_n_per_hw runs,
    each run's batch one column with the batch index running down the rows; and the two interleaved grids with columns
    source 0, prime 0, source 1, prime 1, ...  One launch per grid."""
    out_dir = os.path.join(self.train_dir, 'generated_samples')
    os.makedirs(out_dir, exist_ok=True)
    with self._device():
      host = [(name, g.cpu().numpy()) for name, g in self.render_grids(self._forward(self.log_image_n_per_hw))]
    paths = []
    for name, g in host:
      paths.append(os.path.join(out_dir, '%d_%s.png' % (global_step, name)))
      write_png(paths[-1], g)
    return paths

  @staticmethod
  def render_grids(runs):
    """[(name, uint8 device tensor)] of the eight grids over the outputs of _forward: one launch each, no synchronisation."""
    n, b = len(runs), runs[0]['sources'].shape[0]
    grids = [(name, ops.image_grid([(r[key], k) for k, r in enumerate(runs)], b, n)) for name, key in _IMAGES]
    grids += [(name, ops.image_grid([(r[key], 2 * k + j) for k, r in enumerate(runs) for j, key in enumerate((a, p))], b, 2 * n))
              for name, a, p in _INTERLEAVED]
    return grids

  # ---- summaries --------------------------------------------------------------------------------------------------
  def _grad_scale(self, group):
    """(scale by value, device scalar or None) that turns the group's stored gradients into unscaled ones: 1 / loss_scale as
    the apply divides, or the inv_scale field of the group's TgLossScaleState under dynamic loss scaling."""
    tr = self.trainer
    if tr._ls is not None:
      return 1.0, tr._ls[group].view(torch.float32)[2:3]
    return 1.0 / float(tr.cfg.loss_scale), None

  def collect(self):
    """Enqueues every launch of a read-out and -> (SummaryBuffer, row tags, scalar tags).  No synchronisation."""
    tr = self.trainer
    s = tr.store
    group = tr.last_run[0]
    with self._device():
      acts = self._forward(1)[0] if (self.twin and self.sample_fn is not None) else {}
      rows = [(k, g, 'var') for g in s.GROUPS for k in self.names[g]]
      rows += [(k, group, 'grad') for k in self.names[group]]
      rows += [(k, None, 'act') for k in acts]
      scalars = []
      for g, (loss, terms) in tr.last_losses.items():
        scalars.append((LOSS_TAG[g], loss))
        scalars += [('losses/' + k, v) for k, v in terms.items()]
      if 'gdrop_strength' in s.state:
        scalars.append(('gdrop_strength', s.state['gdrop_strength']))
      if tr._ls is not None:
        scalars += [('loss_scale/' + g, t.view(torch.float32)[0:1]) for g, t in tr._ls.items()]
      buf = ops.SummaryBuffer(len(rows), tr.device, extra=len(scalars))
      row = 0
      for g in s.GROUPS:
        if g in self._var_tables:
          ops.tensor_summaries(table=self._var_tables[g], out=buf, row=row)
          row += self._var_tables[g].njobs
      if group in self._grad_tables:
        scale, scale_dev = self._grad_scale(group)
        ops.tensor_summaries(table=self._grad_tables[group], scale=scale, scale_dev=scale_dev, out=buf, row=row)
        row += self._grad_tables[group].njobs
      if acts:
        ops.tensor_summaries(list(acts.values()), out=buf, row=row)
      if scalars:
        with torch.no_grad():
          buf.extra_view().copy_(torch.cat([v.detach().reshape(-1)[:1].float() for _, v in scalars]))
    return buf, rows, [k for k, _ in scalars]

  def values(self, buf, rows, scalar_tags):
    """The read-out (one copy) -> {tag: float | histogram dict(min, max, num, sum, sum_squares, bucket)} in writing order."""
    stats, buckets, extra = buf.read(extra=True)
    out = {}
    for tag, v in zip(scalar_tags, extra.tolist()):
      out[tag] = v
    out['learning_rate'] = float(self.trainer.cfg.learning_rate)
    for i, (name, _, kind) in enumerate(rows):
      st = stats[i]
      tag = {'var': name, 'grad': 'gradients/' + name, 'act': 'activations/' + name}[kind]
      out[tag] = dict(min=float(st['min']), max=float(st['max']), num=int(st['num']), sum=float(st['sum']),
                      sum_squares=float(st['sum_squares']), bucket=buckets[i])
      if kind == 'grad':      # tf.global_norm([grad]) = sqrt(sum of squares), a one-value histogram
        norm = math.sqrt(float(st['sum_squares']))
        one = np.zeros(len(self._limits), dtype=np.uint32)
        one[int(np.searchsorted(self._limits, norm, side='right'))] = 1
        out['gradient_norms/' + name] = dict(min=norm, max=norm, num=1, sum=norm, sum_squares=norm * norm, bucket=one)
      if kind == 'act':       # tf.nn.zero_fraction: zeros over all elements
        total = int(st['num']) + int(st['nonfinite'])
        out['sparsity/' + name] = float(st['zeros']) / total if total else 0.0
      if st['nonfinite']:
        out['nonfinite/' + tag] = float(st['nonfinite'])
    return out

  def write_summaries(self, global_step):
    vals = self.values(*self.collect())
    protos = []
    for tag, v in vals.items():
      if isinstance(v, dict):
        protos.append(summary.histogram_value(tag, summary.histogram_proto(v['min'], v['max'], v['num'], v['sum'], v['sum_squares'],
                                                                           self._limits, v['bucket'])))
      else:
        protos.append(summary.scalar_value(tag, v))
    self.writer.add(global_step, protos)
    self._last_summary = time.time()
    return vals
