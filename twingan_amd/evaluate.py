"""Evaluation of a trained stage on the GPU -- the step docs/infer_and_eval.md of the reference calls "Evaluation".

MS-SSIM (libs/ms_ssim.py, the PGGAN diversity metric): ops.msssim is the fused HIP kernel, MsSsim the accumulator with the
protocol of the reference's API class (ms_ssim.py:174-199).  The sliced Wasserstein distance (--calc_swd,
image_generation.py:868-941 _calc_swd) has no runnable reference -- one route raises (:926-927), the other asserts that TF
1.8 "is wrongly normalizing by patch" (:931) -- but the algorithm is fixed: section 5 of the PGGAN paper with the reference's
parameters (:938), resolutions (:912-916), 1e3 scale (:910) and result file (:918-925), normalised the way its comment asks
for.  SlicedWasserstein is its accumulator over the ops.swd_* kernels, write_swd_result the file.  Two definitions are this
project's own: the ``real`` column is the distance between the first and the second half of the reals in feed order (the
estimator's noise floor at half the sample), and a channel with sigma = 0 normalises to 0 (not NaN).
evaluate_translation scores a TwinGAN checkpoint: the diversity of what it generates, the similarity of the cycle
s -> t' -> s_cyc to its source (the quantity the L1 cycle loss trains) and, given target-domain images, the SWD between them
and the translations (real = targets, fake = t_prime_output: twingan.py:762-763).  Images stay on the device in the model's
dtype; nothing synchronises before the final read-out.  Which weights are scored is the caller's choice of state dict: the
raw iterate or, under Config.moving_average_decay, the moving averages (ParamStore.averaged_state_dict).  The Inception score needs a pretrained classifier and is out of scope.

KernelDistance is the feature-space metric that needs no classifier: the unbiased kernel two-sample distance (MMD^2) of
Binkowski et al., "Demystifying MMD GANs", over [N, D] feature rows -- with the cubic polynomial kernel the KID -- from the
block sums of ops.mmd_block_sums (include/twingan_hip_mmd.h).  Fed with the model's own content embeddings
(evaluate_translation(latent=True)) it measures how far apart the two domains lie in the shared latent space; fed with any
other rows (embed.read_embeddings of Inception features computed elsewhere) it is KID proper.  This project's own definition:
kid_mean / kid_std are taken over DISJOINT consecutive subsets of subset_size rows (1024), not the literature's 100 random
subsets of 1000."""
import dataclasses

import numpy as np
import torch

from . import ops, pggan
from .config import Config
from .params import ParamStore, declare_twingan
from .twingan import encode_style, translate


class MsSsim:
  """begin() / feed(minibatch) / end() of libs/ms_ssim.py:174-199 for NHWC device minibatches: feed scores
  minibatch[0::2] against minibatch[1::2] and adds the pair scores to a device accumulator; end() returns the average over
  all pairs fed and is the only call that synchronises.  ``scale``: what a pixel is multiplied by on load (255 for [0, 1])."""

  def __init__(self, max_val=255., scale=1., weights=None, k1=0.01, k2=0.03):
    self.kw = dict(max_val=max_val, scale=scale, weights=weights, k1=k1, k2=k2)
    self.sum = None
    self.num_pairs = 0

  def begin(self, mode=None):
    self.sum = None
    self.num_pairs = 0

  def feed_pairs(self, img1, img2):
    """Scores img1[i] against img2[i]; returns the per-pair scores (device tensor)."""
    score, _, _, mean = ops.msssim(img1.contiguous(), img2.contiguous(), return_mean=True, **self.kw)
    part = mean * float(score.shape[0])      # as the reference: score of the minibatch * its number of pairs
    self.sum = part if self.sum is None else self.sum + part
    self.num_pairs += score.shape[0]
    return score

  def feed(self, minibatch, mode=None):
    assert minibatch.shape[0] % 2 == 0, 'a minibatch holds pairs: even size'
    return self.feed_pairs(minibatch[0::2], minibatch[1::2])

  def end(self, mode=None):
    assert self.num_pairs > 0, 'nothing was fed'
    return float(self.sum.item()) / self.num_pairs


class SlicedWasserstein:
  """begin() / feed(reals, fakes) / end() like MsSsim, for NHWC device minibatches [n, hw, hw, 3] in [0, 1] (fp32 / bf16 /
  fp16; hw a power of two in 16..512).  feed builds both Laplacian pyramids and gathers ``per`` 7 x 7 x 3 descriptors per image
  and level into buffers preallocated for ``num_images`` (the reference's swd_num_images) -- no synchronisation; end()
  normalises, projects on ``repeats`` x ``dirs`` unit directions per level, sorts and returns
    {'resolutions': [hw, hw/2, ..., 16], 'real': [...], 'fake': [...], 'average': (real, fake)}      (all times 1e3)
  fake = distance(reals, fakes); real = distance(first half of the reals in feed order, second half) -- this project's
  definition of the reference's ``real`` column; it needs an even number of images.  Patch centres and directions are inputs of
  the kernels: drawn from a CPU torch.Generator seeded at begin() (so a seed fixes the result bit for bit) unless injected."""

  def __init__(self, hw, num_images, per=128, repeats=4, dirs=128, scale=255., quantize=True, seed=0):
    self.resolutions = ops.swd_resolutions(hw)
    if not self.resolutions or hw & (hw - 1) or hw > 512:      # image_generation.py:869-871: no SWD on small images
      raise ValueError('SlicedWasserstein: hw must be a power of two in 16..512 (got %d)' % hw)
    self.hw, self.num_images, self.per, self.repeats, self.dirs = hw, int(num_images), int(per), int(repeats), int(dirs)
    self.scale, self.quantize, self.seed = float(scale), bool(quantize), seed
    self.gen = torch.Generator().manual_seed(seed)
    self.desc = None
    self.count = 0

  def begin(self, mode=None):
    self.gen.manual_seed(self.seed)
    self.count = 0

  def draw_centres(self, n):
    """One feed's tables: per level (centres of the reals, of the fakes), int32 [n * per, 2] in [3, s - 3), independent draws."""
    return [tuple(torch.randint(3, s - 3, (n * self.per, 2), generator=self.gen, dtype=torch.int32) for _ in range(2))
            for s in self.resolutions]

  def draw_dirs(self):
    """Per level: [repeats, 147, dirs] fp32 Gaussian directions of unit L2 norm over the 147 axis."""
    out = []
    for _ in self.resolutions:
      d = torch.randn(self.repeats, ops.SWD_K, self.dirs, generator=self.gen, dtype=torch.float32)
      out.append(d / d.norm(dim=1, keepdim=True))
    return out

  def feed(self, reals, fakes, centres=None):
    n = reals.shape[0]
    if tuple(reals.shape) != tuple(fakes.shape) or tuple(reals.shape[1:]) != (self.hw, self.hw, 3):
      raise ops._lib.TgError('SlicedWasserstein.feed: reals and fakes must both be [n, %d, %d, 3] (got %s and %s)'
                             % (self.hw, self.hw, tuple(reals.shape), tuple(fakes.shape)))
    if self.count + n > self.num_images:
      raise ops._lib.TgError('SlicedWasserstein.feed: %d images fed, the buffers hold %d' % (self.count + n, self.num_images))
    if self.desc is None:
      self.desc = [tuple(torch.empty(self.num_images * self.per, ops.SWD_K, dtype=torch.float32, device=reals.device)
                         for _ in range(2)) for _ in self.resolutions]
    centres = self.draw_centres(n) if centres is None else centres
    assert len(centres) == len(self.resolutions), 'centres: one (reals, fakes) pair of tables per level'
    for which, x in enumerate((reals, fakes)):
      levels = ops.swd_pyramid(x.contiguous(), self.scale, self.quantize)
      for l, level in enumerate(levels):
        ops.swd_descriptors(level, centres[l][which], self.per, out=self.desc[l][which], row_offset=self.count * self.per)
    self.count += n

  def distances(self, dirs=None):
    """-> per level (real, fake) device tensors [1], not yet scaled; no synchronisation."""
    if self.count == 0 or self.count % 2:
      raise ops._lib.TgError('SlicedWasserstein.end: the real column compares two halves of the reals: feed an even, non-zero '
                             'number of images (got %d)' % self.count)
    dirs = self.draw_dirs() if dirs is None else dirs
    assert len(dirs) == len(self.resolutions), 'dirs: one [repeats, 147, dirs] tensor per level'
    n, out = self.count * self.per, []
    for l, (dr, df) in enumerate(self.desc):
      d = torch.as_tensor(dirs[l], dtype=torch.float32).to(dr.device).contiguous()
      fake = ops.swd_distance(dr[:n], df[:n], d)[0]
      real = ops.swd_distance(dr[:n // 2], dr[n // 2:n], d)[0]
      out.append((real, fake))
    return out

  def end(self, dirs=None, mode=None):
    table = torch.stack([torch.cat(p) for p in self.distances(dirs)]).double().cpu() * 1e3      # the only synchronisation
    real, fake = [float(v) for v in table[:, 0]], [float(v) for v in table[:, 1]]
    return {'resolutions': list(self.resolutions), 'real': real, 'fake': fake,
            'average': (sum(real) / len(real), sum(fake) / len(fake))}


def write_swd_result(path, result, num_images):
  """The reference's result file (image_generation.py:918-925) for what SlicedWasserstein.end() returned."""
  with open(path, 'w') as f:
    f.write('swd sliced wasserstein score evaluated on %d images.\n' % num_images)
    f.write('res\treal\tfake\n')
    for hw, real, fake in zip(result['resolutions'], result['real'], result['fake']):
      f.write('%d\t%f\t%f\n' % (hw, real, fake))
    f.write('Average\t%f\t%f\n' % tuple(result['average']))


def kernel_distance_from_sums(xx, yy, xy, m, n, block, subset_size):
  """The host arithmetic of KernelDistance.end(), float64: ``xx`` [ceil(m / block), ceil(m / block)] and ``yy`` (n likewise) are
  the block sums of the two sets against themselves WITHOUT the diagonal pairs, ``xy`` [ceil(m / block), ceil(n / block)] those
  of one against the other.  -> the dict KernelDistance.end() documents."""
  xx, yy, xy = (np.asarray(v, dtype=np.float64) for v in (xx, yy, xy))
  m, n, block, subset_size = int(m), int(n), int(block), int(subset_size)
  if m < 2 or n < 2:
    raise ValueError('KernelDistance: the unbiased estimate needs at least 2 rows on each side (got %d and %d)' % (m, n))
  if block < 32 or block % 32 or subset_size < block or subset_size % block:
    raise ValueError('KernelDistance: block = %d must be a multiple of 32, subset_size = %d a multiple of block' % (block, subset_size))
  bm, bn = -(-m // block), -(-n // block)
  if xx.shape != (bm, bm) or yy.shape != (bn, bn) or xy.shape != (bm, bn):
    raise ValueError('KernelDistance: block sums of shapes %s, %s, %s do not belong to %d and %d rows in blocks of %d'
                     % (xx.shape, yy.shape, xy.shape, m, n, block))

  def estimate(sxx, syy, sxy, rows_x, rows_y):
    return float(sxx.sum()) / (rows_x * (rows_x - 1)) + float(syy.sum()) / (rows_y * (rows_y - 1)) - 2.0 * float(sxy.sum()) / (rows_x * rows_y)

  out = {'mmd2': estimate(xx, yy, xy, m, n), 'm': m, 'n': n, 'subset_size': subset_size}
  per, subsets = subset_size // block, min(m, n) // subset_size
  vals = [estimate(xx[k * per:(k + 1) * per, k * per:(k + 1) * per], yy[k * per:(k + 1) * per, k * per:(k + 1) * per],
                   xy[k * per:(k + 1) * per, k * per:(k + 1) * per], subset_size, subset_size) for k in range(subsets)]
  out['num_subsets'] = subsets
  out['kid_mean'] = float(np.mean(vals)) if vals else None
  out['kid_std'] = float(np.std(vals)) if vals else None
  return out


class KernelDistance:
  """begin() / feed(x_rows, y_rows) / end() like MsSsim and SlicedWasserstein, for feature rows: feed copies [*, dim] device
  tensors (one dtype for everything fed: fp32 / bf16 / fp16; either argument may be None) behind what was fed before into
  buffers preallocated for ``capacity`` rows a side -- no synchronisation, and more rows than the buffers hold are refused;
  end() launches three ops.mmd_block_sums (X against X and Y against Y without the diagonal, X against Y), makes ONE
  device-to-host copy, the only synchronisation, and returns, all in float64 on the host,
    {'mmd2':        the unbiased estimate over everything fed, sumXX / (m (m - 1)) + sumYY / (n (n - 1)) - 2 sumXY / (m n),
     'kid_mean', 'kid_std', 'num_subsets', 'subset_size':
                    the same estimator on each of the min(m, n) // subset_size DISJOINT CONSECUTIVE subsets (rows
                    k subset_size .. of either side), read off the same block sums: their mean and their standard deviation
                    (the population one, numpy.std); None / None / 0 when fewer rows than one subset were fed,
     'm', 'n':      rows fed on each side}.
  The kernel is (gamma x.y + coef0) ** degree; ``gamma`` None = float32(1 / dim): at the defaults the KID's cubic kernel.
  This project's own definition: the literature's KID averages 100 RANDOM subsets of 1000; this one takes disjoint subsets of
  1024 in feed order -- or, with ``shuffle_seed``, in the order of one permutation per side drawn at end() from a CPU
  torch.Generator seeded with it (X's first), so a seed fixes the result bit for bit.  ``subset_size`` must be a multiple of
  ``block`` (itself a multiple of 32); fewer than 2 rows on a side are refused."""

  def __init__(self, dim, capacity, subset_size=1024, block=32, degree=3, gamma=None, coef0=1.0, shuffle_seed=None):
    self.dim, self.capacity, self.subset_size, self.block = int(dim), int(capacity), int(subset_size), int(block)
    if self.dim < 1 or self.capacity < 2:
      raise ValueError('KernelDistance: dim = %d, capacity = %d' % (self.dim, self.capacity))
    if self.block < 32 or self.block % 32 or self.subset_size < self.block or self.subset_size % self.block:
      raise ValueError('KernelDistance: block = %d must be a multiple of 32, subset_size = %d a multiple of block'
                       % (self.block, self.subset_size))
    if not 1 <= int(degree) <= ops.MMD_MAX_DEGREE:
      raise ValueError('KernelDistance: degree = %d outside 1 .. %d' % (degree, ops.MMD_MAX_DEGREE))
    self.kernel = dict(block=self.block, degree=int(degree), gamma=gamma, coef0=float(coef0))
    self.shuffle_seed = shuffle_seed
    self.buf = None
    self.count = [0, 0]

  def begin(self, mode=None):
    self.count = [0, 0]

  def feed(self, x_rows, y_rows, mode=None):
    for side, rows in enumerate((x_rows, y_rows)):
      if rows is None:
        continue
      if rows.dim() != 2 or rows.shape[1] != self.dim:
        raise ops._lib.TgError('KernelDistance.feed: rows [*, %d] are needed (got %s)' % (self.dim, tuple(rows.shape)))
      if self.buf is None:
        self.buf = [torch.empty(self.capacity, self.dim, dtype=rows.dtype, device=rows.device) for _ in range(2)]
      if rows.dtype != self.buf[0].dtype or rows.device != self.buf[0].device:
        raise ops._lib.TgError('KernelDistance.feed: rows of %s on %s, the buffers hold %s on %s'
                               % (rows.dtype, rows.device, self.buf[0].dtype, self.buf[0].device))
      k = int(rows.shape[0])
      if self.count[side] + k > self.capacity:
        raise ops._lib.TgError('KernelDistance.feed: %d rows fed, the buffers hold %d' % (self.count[side] + k, self.capacity))
      self.buf[side][self.count[side]:self.count[side] + k].copy_(rows)
      self.count[side] += k

  def block_sums(self):
    """-> (xx, yy, xy) device fp64 block sums of what was fed; no synchronisation."""
    m, n = self.count
    if m < 2 or n < 2:
      raise ops._lib.TgError('KernelDistance.end: the unbiased estimate needs at least 2 rows on each side (got %d and %d)' % (m, n))
    x, y = self.buf[0][:m], self.buf[1][:n]
    if self.shuffle_seed is not None:
      gen = torch.Generator().manual_seed(int(self.shuffle_seed))
      x, y = (t.index_select(0, torch.randperm(t.shape[0], generator=gen).to(t.device)) for t in (x, y))
    with torch.cuda.device(x.device):
      return (ops.mmd_block_sums(x, x, skip_same_index=True, **self.kernel), ops.mmd_block_sums(y, y, skip_same_index=True, **self.kernel),
              ops.mmd_block_sums(x, y, **self.kernel))

  def end(self, mode=None):
    m, n = self.count
    xx, yy, xy = self.block_sums()
    host = torch.cat([xx.reshape(-1), yy.reshape(-1), xy.reshape(-1)]).cpu().numpy()      # the only synchronisation
    a, b = xx.numel(), xx.numel() + yy.numel()
    return kernel_distance_from_sums(host[:a].reshape(xx.shape), host[a:b].reshape(yy.shape), host[b:].reshape(xy.shape), m, n,
                                     self.block, self.subset_size)


def evaluate_translation(cfg, state_dict, sources, to='t', batch=16, device='cuda', translate_fn=None, targets=None, latent=False,
                         encode_fn=None):
  """Scores a TwinGAN stage on ``sources`` (float [N, hw, hw, 3] in [0, 1], N even; tensor or array):
    ms_ssim_diversity: MS-SSIM between consecutive generated images translate(source, to) (pairs 0-1, 2-3, ...; lower =
                       more diverse, the reference's use of the metric);
    ms_ssim_cycle:     MS-SSIM(source, translate(translate(source, to), from)).
  Style-embedding configurations use the encoded style of each translation's own input, as ImageInferer.infer does for
  custom_generated_*_style_source.  ``translate_fn(x, to) -> image batch`` replaces the model (tests: an identity stand-in);
  with it ``state_dict`` is not read.  With ``targets`` (images of the domain translated to, same shape as ``sources``) the
  result also holds swd_real, swd_fake (per resolution, times 1e3) and swd_resolutions: SlicedWasserstein at its defaults
  fed (targets, translate(sources)) batch by batch.
  ``state_dict`` names the weights that are scored: ParamStore.state_dict(include_state=True) for the last optimiser
  iterate, ParamStore.averaged_state_dict() for the moving averages of a run under Config.moving_average_decay -- the
  weights the reference's eval branch restores (model/model_inheritor.py:1150-1155) and the PGGAN paper scores.
  ``latent`` (True, or a dict of KernelDistance keyword arguments such as subset_size; needs ``targets``) adds
  out['latent'] = {'domains': ..., 'translation': ..., 'floor': ...}, three KernelDistance.end() dicts over content
  embeddings E_d(x) = pggan.encoder_before_classification under is_training=False, flattened as
  embed.ContentEncoder.encode does, all fed batch by batch in the same loop:
    domains      E_from(sources) against E_to(targets): the alignment of the shared latent space;
    translation  E_to(translate(sources, to)) against E_to(targets): fakes against reals;
    floor        the first against the second half of E_to(targets) in feed order: the estimator's noise at half the sample,
                 as SWD's ``real`` column.
  ``encode_fn(x, domain) -> [B, D]`` replaces the encoder as translate_fn replaces the model."""
  assert to in ('s', 't'), to
  if latent and targets is None:
    raise ValueError('evaluate_translation: latent=True compares with the target domain: targets are needed')
  cfg = cfg if isinstance(cfg, Config) else Config(**cfg)
  device = torch.device(device)
  dtype = {'bf16': torch.bfloat16, 'fp16': torch.float16, 'fp32': torch.float32}[cfg.precision]
  frm = 's' if to == 't' else 't'
  store = None
  if translate_fn is None or (latent and encode_fn is None):
    store = declare_twingan(ParamStore(device), cfg).build(0)
    store.load_state_dict(state_dict)
  if latent and encode_fn is None:
    cfg_infer = dataclasses.replace(cfg, is_training=False)

    def encode_fn(x, domain):
      net, _ = pggan.encoder_before_classification(store.P, x.contiguous(), domain, cfg_infer)
      return net.contiguous().reshape(x.shape[0], -1)

  if translate_fn is None:
    def translate_fn(x, to_):
      style = encode_style(store.P, x, cfg, 's' if to_ == 't' else 't') if cfg.use_style_embedding else None
      return translate(store.P, x, cfg, to_, style)

  x_all = torch.as_tensor(sources)
  assert x_all.dim() == 4 and x_all.shape[0] % 2 == 0 and batch % 2 == 0, 'pairs: even number of sources and even batch'
  diversity, cycle = MsSsim(scale=255.), MsSsim(scale=255.)
  diversity.begin()
  cycle.begin()
  swd, t_all = None, None
  if targets is not None:
    t_all = torch.as_tensor(targets)
    assert tuple(t_all.shape) == tuple(x_all.shape), 'targets: as many images as sources, of the same size'
    swd = SlicedWasserstein(x_all.shape[1], x_all.shape[0])
    swd.begin()
  kd, total, half = None, x_all.shape[0], x_all.shape[0] // 2
  with torch.cuda.device(device), torch.no_grad():
    for i in range(0, x_all.shape[0], batch):
      x = x_all[i:i + batch].to(device).to(dtype).contiguous()
      y = translate_fn(x, to).detach()
      back = translate_fn(y, frm).detach()
      diversity.feed(y)
      cycle.feed_pairs(x, back)
      if swd is not None:
        t = t_all[i:i + batch].to(device).to(dtype).contiguous()
        swd.feed(t, y)
        if latent:
          e_src, e_fake, e_tgt = encode_fn(x, frm), encode_fn(y, to), encode_fn(t, to)
          if kd is None:
            kw = dict(latent) if isinstance(latent, dict) else {}
            kd = {'domains': KernelDistance(e_tgt.shape[1], total, **kw), 'translation': KernelDistance(e_tgt.shape[1], total, **kw),
                  'floor': KernelDistance(e_tgt.shape[1], max(half, 2), **kw)}
          kd['domains'].feed(e_src, e_tgt)
          kd['translation'].feed(e_fake, e_tgt)
          first = min(max(half - i, 0), e_tgt.shape[0])      # rows of this batch that belong to the first half
          kd['floor'].feed(e_tgt[:first] if first else None, e_tgt[first:] if first < e_tgt.shape[0] else None)
    out = {'ms_ssim_diversity': diversity.end(), 'ms_ssim_cycle': cycle.end()}
    if swd is not None:
      res = swd.end()
      out.update(swd_real=res['real'], swd_fake=res['fake'], swd_resolutions=res['resolutions'])
    if kd is not None:
      out['latent'] = {k: v.end() for k, v in kd.items()}
  if store is not None:
    store.close()
  return out
