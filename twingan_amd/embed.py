"""The shared latent space, exported and searched -- the MI355X counterpart of the trainer's --do_output --output_single_file
branch (model/model_inheritor.py:1172-1180, twingan.py:685-729), which walks a dataset once and appends
`filename, flattened encoded_*_content_before_classification` rows to a CSV, and of the search the reference's blog runs over
those rows (docs/blog/blog_EN.md:98-100) and leaves to the reader.

ContentEncoder gives the embedding of a batch of images, export_embeddings / read_embeddings are the CSV, NearestNeighbours is
the exact search on the device (ops.knn_topk, include/twingan_hip_knn.h) as a begin() / feed() / end() accumulator like
evaluate.MsSsim, and cross_domain_neighbours is the blog's use: the closest faces of both domains to a portrait.

This project's own definitions (the reference has no search): results ascend by (distance, index) and equal distances resolve
to the lower index; a pair whose distance is NaN is never selected; cosine distance against a zero row is 1; slots for which
the gallery had no row are +inf / -1."""
import csv
import dataclasses

import numpy as np
import torch

from . import ops, pggan
from .config import Config
from .inference import ImageInferer

METRICS = ('l2', 'cosine')


class ContentEncoder(ImageInferer):
  """E_s / E_t of a trained TwinGAN under the inference configuration twingan.translate derives (is_training=False: batch norm
  on its moving statistics).  State dict, checkpoint and averaged weights as ImageInferer: ``from_checkpoint(cfg, model_path,
  device, moving_average=)``."""

  def __init__(self, cfg, state_dict, device='cuda', output_tensor_name='custom_generated_t_style_source'):
    super().__init__(cfg, state_dict, device, output_tensor_name)      # infer() keeps working on the same variables
    self.cfg_infer = dataclasses.replace(self.cfg, is_training=False)

  @classmethod
  def from_checkpoint(cls, cfg, model_path, device='cuda', moving_average=False):
    return super().from_checkpoint(cfg, model_path, device, moving_average=moving_average)

  @property
  def dim(self):
    """D = 4 * 4 * max_ch."""
    return 16 * int(self.cfg.max_ch)

  def encode(self, images, domain):
    """``images``: what preprocess() takes, or a device tensor [B, hw, hw, 3] of the model's dtype; ``domain`` 's' or 't'
    -> [B, 16 C] of the model's dtype on the device: pggan.encoder_before_classification, flattened in NHWC order (the
    reference's reshape([B, -1]) of a TF tensor)."""
    if domain not in ('s', 't'):
      raise ValueError("encode: domain must be 's' or 't' (got %r)" % (domain,))
    ready = isinstance(images, torch.Tensor) and images.is_cuda and images.dtype == self.dtype and images.dim() == 4 and \
        images.shape[1] == self.cfg.hw
    x = images.contiguous() if ready else self.preprocess(images)
    with torch.cuda.device(self.device), torch.no_grad():
      net, _ = pggan.encoder_before_classification(self.store.P, x, domain, self.cfg_infer)
      return net.contiguous().reshape(x.shape[0], -1)


def embedding_row(filename, values):
  """One CSV row of the reference's _write_outputs: the name, then every value as Python's repr of the float32's double --
  what its ``[name] + embedding.tolist()`` hands csv.writer."""
  return [filename] + [float(np.float32(v)) for v in values]


def export_embeddings(encoder, batches, domain, csv_path):
  """Appends `filename, e_0, ..., e_{D-1}` rows to ``csv_path`` for every (filenames, images) of ``batches``; one
  device-to-host copy per batch.  -> the number of rows written."""
  rows = 0
  with open(csv_path, 'a', newline='') as fh:
    w = csv.writer(fh)
    for names, images in batches:
      emb = encoder.encode(images, domain).float().cpu().numpy()      # the one copy
      if len(names) != emb.shape[0]:
        raise ValueError('export_embeddings: %d names for %d images' % (len(names), emb.shape[0]))
      for name, e in zip(names, emb):
        w.writerow(embedding_row(name.decode() if isinstance(name, bytes) else str(name), e))
      rows += emb.shape[0]
  return rows


def read_embeddings(csv_path):
  """-> (filenames, float32 [N, D]) of a file export_embeddings wrote (bit for bit: repr round-trips a double)."""
  names, rows = [], []
  with open(csv_path, newline='') as fh:
    for row in csv.reader(fh):
      if row:
        names.append(row[0])
        rows.append(np.array([float(v) for v in row[1:]], dtype=np.float64).astype(np.float32))
  if not rows:
    return names, np.zeros((0, 0), dtype=np.float32)
  if len({r.size for r in rows}) != 1:
    raise ValueError('read_embeddings: %s holds rows of different lengths' % csv_path)
  return names, np.stack(rows)


class NearestNeighbours:
  """begin() / feed(gallery_batch) / end() over ops.knn_topk: the k nearest gallery rows of every query, exact, the gallery
  streamed in batches of any size (the result does not depend on how it was cut).  ``queries``: device tensor [Q, D] (fp32 /
  bf16 / fp16); gallery batches must have its dtype and D.  feed numbers rows in feed order and does not synchronise; end()
  returns NumPy (dist float32 [Q, k], idx int64 [Q, k]) in one device-to-host copy and is the only synchronisation.
  ``query_ids``: int64 [Q] (tensor, array or list), the gallery index that IS query i and is left out of its result (a set
  searched against itself); a device tensor is used as it is."""

  def __init__(self, queries, k, metric='l2', query_ids=None):
    if metric not in METRICS:
      raise ValueError('NearestNeighbours: metric %r is not one of %s' % (metric, METRICS))
    self.queries = queries.contiguous()
    self.k, self.metric = int(k), metric
    if query_ids is not None and not isinstance(query_ids, torch.Tensor):
      query_ids = torch.as_tensor(np.asarray(query_ids), dtype=torch.int64)
    self.query_ids = None if query_ids is None else query_ids.to(device=queries.device, dtype=torch.int64).contiguous()      # no wait
    self.begin()

  def begin(self, mode=None):
    self.table = None
    self.count = 0

  def feed(self, gallery_batch, mode=None):
    with torch.cuda.device(self.queries.device):
      self.table = ops.knn_topk(self.queries, gallery_batch.contiguous(), self.k, self.metric, out=self.table,
                                index_offset=self.count, query_ids=self.query_ids)
    self.count += int(gallery_batch.shape[0])
    return self.table

  def end(self, mode=None):
    assert self.table is not None, 'nothing was fed'
    dist, idx = self.table
    ni = idx.numel() * 8      # the int64 part first: both views stay aligned
    host = torch.cat([idx.view(torch.uint8).reshape(-1), dist.view(torch.uint8).reshape(-1)]).cpu().numpy()      # the one copy
    return host[ni:].view(np.float32).reshape(dist.shape).copy(), host[:ni].view(np.int64).reshape(idx.shape).copy()


def cross_domain_neighbours(encoder, query_images, query_domain, galleries, k, metric='l2'):
  """The blog's demonstration: the content embedding of ``query_images`` (domain ``query_domain``) against the galleries of
  both domains.  ``galleries``: {'s': ..., 't': ...} (either may be missing), each an embedding tensor [N, D] or an iterable of
  such batches, in the encoder's dtype (ContentEncoder.encode of a dataset, or read_embeddings moved to the device).
  -> {domain: (dist [Q, k], idx [Q, k])} as NumPy; indices count that gallery's rows in feed order."""
  q = encoder.encode(query_images, query_domain)
  out = {}
  for dom, gal in galleries.items():
    nn = NearestNeighbours(q, k, metric)
    for batch in ([gal] if isinstance(gal, torch.Tensor) else gal):
      nn.feed(batch.to(device=q.device, dtype=q.dtype))
    out[dom] = nn.end()
  return out
