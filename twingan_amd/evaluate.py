"""Evaluation of a trained stage on the GPU -- the step docs/infer_and_eval.md of the reference calls "Evaluation".

MS-SSIM (libs/ms_ssim.py, the PGGAN diversity metric) is the one metric of the reference that can be run, so it is the
one built here: ops.msssim is the fused HIP kernel, MsSsim the accumulator with the protocol of the reference's API class
(ms_ssim.py:174-199), evaluate_translation the scores of a TwinGAN checkpoint: the diversity of what it generates and
the similarity of the cycle s -> t' -> s_cyc to its source (the quantity the L1 cycle loss trains).  Images stay on the
device in the model's dtype; nothing synchronises before the final read-out.  The sliced Wasserstein distance and the
Inception score have no runnable reference (image_generation.py:926-931 raises) and are out of scope."""
import torch

from . import ops
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


def evaluate_translation(cfg, state_dict, sources, to='t', batch=16, device='cuda', translate_fn=None):
  """Scores a TwinGAN stage on ``sources`` (float [N, hw, hw, 3] in [0, 1], N even; tensor or array):
    ms_ssim_diversity: MS-SSIM between consecutive generated images translate(source, to) (pairs 0-1, 2-3, ...; lower =
                       more diverse, the reference's use of the metric);
    ms_ssim_cycle:     MS-SSIM(source, translate(translate(source, to), from)).
  Style-embedding configurations use the encoded style of each translation's own input, as ImageInferer.infer does for
  custom_generated_*_style_source.  ``translate_fn(x, to) -> image batch`` replaces the model (tests: an identity stand-in);
  with it ``state_dict`` is not read."""
  assert to in ('s', 't'), to
  cfg = cfg if isinstance(cfg, Config) else Config(**cfg)
  device = torch.device(device)
  dtype = {'bf16': torch.bfloat16, 'fp16': torch.float16, 'fp32': torch.float32}[cfg.precision]
  frm = 's' if to == 't' else 't'
  store = None
  if translate_fn is None:
    store = declare_twingan(ParamStore(device), cfg).build(0)
    store.load_state_dict(state_dict)

    def translate_fn(x, to_):
      style = encode_style(store.P, x, cfg, 's' if to_ == 't' else 't') if cfg.use_style_embedding else None
      return translate(store.P, x, cfg, to_, style)

  x_all = torch.as_tensor(sources)
  assert x_all.dim() == 4 and x_all.shape[0] % 2 == 0 and batch % 2 == 0, 'pairs: even number of sources and even batch'
  diversity, cycle = MsSsim(scale=255.), MsSsim(scale=255.)
  diversity.begin()
  cycle.begin()
  with torch.cuda.device(device), torch.no_grad():
    for i in range(0, x_all.shape[0], batch):
      x = x_all[i:i + batch].to(device).to(dtype).contiguous()
      y = translate_fn(x, to).detach()
      back = translate_fn(y, frm).detach()
      diversity.feed(y)
      cycle.feed_pairs(x, back)
    out = {'ms_ssim_diversity': diversity.end(), 'ms_ssim_cycle': cycle.end()}
  if store is not None:
    store.close()
  return out
