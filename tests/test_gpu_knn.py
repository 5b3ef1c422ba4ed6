"""Nearest-neighbour search over embeddings on the device (include/twingan_hip_knn.h, ops.knn_topk, twingan_amd/embed.py)
against the float64 / int64 restatement tests/knn_ref.py.  Also runs under TG_EMU=1 over the emulated kernels.

Exact cases: integer-valued inputs in [-4, 4] are exact in bf16, fp16 and fp32, and with d <= 4096 every norm, dot product
and squared distance is an integer below 2^24, so fp32 is exact in any summation order -- distances and indices must EQUAL the
int64 reference under the (distance, index) order, ties (plentiful) included.

Real-valued cases: Gaussian inputs rounded to the dtype first; the two conditions of knn_ref.check_real hold for every query
with the bounds knn_ref derives from the inputs alone (its docstring): squared L2 b = gamma_(d+3) (|q|^2 + |g|^2 + 2 sum|q_i||g_i|),
cosine b = gamma_(d+8) (sum|q_i g_i| / (|q||g|) + |cos| + 1), u = 2^-23."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guarded      # noqa: E402
import knn_ref as R      # noqa: E402

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
DTYPES = {'fp32': torch.float32, 'bf16': torch.bfloat16, 'fp16': torch.float16}
EXACT_SHAPES = [(1, 1, 1, 1), (3, 5, 16, 8), (33, 257, 24, 8), (70, 1000, 128, 32), (5, 4099, 4096, 8)]


def _ints(seed, q, n, d):
  rng = np.random.default_rng(seed)
  return rng.integers(-4, 5, size=(q, d)).astype(np.float32), rng.integers(-4, 5, size=(n, d)).astype(np.float32)


def _reals(seed, q, n, d, dt):
  """Gaussian rows rounded to the dtype: -> (float32 arrays that hold exactly the rounded values)."""
  g = torch.Generator().manual_seed(seed)
  return tuple(torch.randn(r, d, generator=g).to(dt).float().numpy() for r in (q, n))


def _dev(a, dt):
  return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(dt).contiguous()


def _search(q, g, k, metric='l2', chunk=None, index_offset=0, query_ids=None):
  """ops.knn_topk over the gallery in chunks of ``chunk`` rows (None: one) -> NumPy (dist, idx)."""
  from twingan_amd import ops
  n = g.shape[0]
  chunk = chunk or n
  table = None
  for lo in range(0, n, chunk):
    table = ops.knn_topk(q, g[lo:lo + chunk], k, metric, out=table, index_offset=index_offset + lo, query_ids=query_ids)
  torch.cuda.synchronize()
  return table[0].cpu().numpy(), table[1].cpu().numpy()


@pytest.fixture(scope='module')
def exact_refs():
  """The int64 reference of every exact shape, computed once."""
  out = {}
  for shape in EXACT_SHAPES:
    q, n, d, k = shape
    qa, ga = _ints(sum(shape), q, n, d)
    out[shape] = (qa, ga, R.topk(R.sq_l2_int(qa, ga), k))
  return out


@pytest.mark.parametrize('dtype', list(DTYPES))
@pytest.mark.parametrize('shape', EXACT_SHAPES, ids=lambda s: 'q%d_n%d_d%d_k%d' % s)
def test_exact_cases_equal_the_integer_reference(shape, dtype, exact_refs):
  qa, ga, (want_d, want_i) = exact_refs[shape]
  got_d, got_i = _search(_dev(qa, DTYPES[dtype]), _dev(ga, DTYPES[dtype]), shape[3])
  assert np.array_equal(got_i, want_i), (got_i[:2], want_i[:2])
  assert np.array_equal(got_d.astype(np.float64), want_d)
  if shape[1] < shape[3]:      # the filler
    assert np.all(got_i[:, shape[1]:] == -1) and np.all(np.isposinf(got_d[:, shape[1]:]))


@pytest.mark.parametrize('dtype', list(DTYPES))
def test_split_plan_runs_the_merge_and_duplicated_rows_resolve_by_index(dtype):
  from twingan_amd import ops
  q, n, d, k = 33, 700, 40, 16
  assert ops.knn_plan(q, n, d, k)[0] > 1 and ops.knn_plan(q, 128, d, k)[0] == 1 and ops.knn_plan(1, 1, 1, 1)[0] == 1
  qa, base = _ints(11, q, 9, d)
  ga = base[np.random.default_rng(12).integers(0, 9, size=n)]      # nine distinct rows, each many times over
  want_d, want_i = R.topk(R.sq_l2_int(qa, ga), k)
  got_d, got_i = _search(_dev(qa, DTYPES[dtype]), _dev(ga, DTYPES[dtype]), k)
  assert np.array_equal(got_i, want_i) and np.array_equal(got_d.astype(np.float64), want_d)
  # the plan is where the rule lives: the workspace it reports is what the launch accepts, and one byte less is refused
  from twingan_amd import _lib
  splits, ws_bytes = ops.knn_plan(q, n, d, k)
  assert ws_bytes == 4 * (2 * splits * q * k + q + n)
  dist, idx = ops.knn_table(q, k, DEV)
  ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=DEV)
  qd, gd = _dev(qa, DTYPES[dtype]), _dev(ga, DTYPES[dtype])
  args = [qd.data_ptr(), q, gd.data_ptr(), n, d, ops._dt(qd), 0, k, 0, None, dist.data_ptr(), idx.data_ptr(), ws.data_ptr()]
  with pytest.raises(_lib.TgError, match='workspace'):
    _lib.call('tg_knn_topk', *args, ws_bytes - 1, ops._stream())
  _lib.call('tg_knn_topk', *args, ws_bytes, ops._stream())
  torch.cuda.synchronize()
  assert np.array_equal(idx.cpu().numpy(), want_i)


@pytest.mark.parametrize('metric', ['l2', 'cosine'])
@pytest.mark.parametrize('dtype', list(DTYPES))
@pytest.mark.parametrize('shape', [(33, 257, 24, 8), (70, 1000, 130, 32), (5, 515, 1031, 8)], ids=lambda s: 'q%d_n%d_d%d_k%d' % s)
def test_real_valued_cases_within_the_derived_bounds(shape, dtype, metric):
  q, n, d, k = shape
  qa, ga = _reals(5 + q, q, n, d, DTYPES[dtype])
  if metric == 'cosine':
    ga[3] = 0      # a zero row: distance 1 to everything
  ref, bound = (R.sq_l2(qa, ga), R.sq_l2_bound(qa, ga)) if metric == 'l2' else (R.cosine(qa, ga), R.cosine_bound(qa, ga))
  got_d, got_i = _search(_dev(qa, DTYPES[dtype]), _dev(ga, DTYPES[dtype]), k, metric)
  w1, w2 = R.check_real(got_d, got_i, ref, bound, k)
  print('[knn %s %s %s] worst error / bound %.3f, worst order shortfall / allowed %.3f' % (metric, dtype, shape, w1, w2))
  if metric == 'cosine':
    assert np.all(ref[:, 3] == 1.0)
    hit = got_i == 3
    assert np.all(got_d[hit] == 1.0)


@pytest.mark.parametrize('metric', ['l2', 'cosine'])
@pytest.mark.parametrize('dtype', list(DTYPES))
@pytest.mark.parametrize('q', [70, 40, 5])      # the three query tiles of the 16-bit kernel: 128, 64, 32 (the last two take the gallery norms in the tile loop)
def test_results_are_bit_identical_however_the_gallery_is_chunked_or_split(q, dtype, metric):
  from twingan_amd import ops
  n, d, k = 1000, 128, 32
  assert ops.knn_plan(q, n, d, k)[0] > 1 and ops.knn_plan(q, 7, d, k)[0] == 1 and ops.knn_plan(q, 256, d, k)[0] == 2
  qa, ga = _reals(21, q, n, d, DTYPES[dtype])
  ga[500:520] = ga[100:120]      # ties across chunk and tile borders
  qd, gd = _dev(qa, DTYPES[dtype]), _dev(ga, DTYPES[dtype])
  one = _search(qd, gd, k, metric)
  for chunk in (1, 7, 256):
    got = _search(qd, gd, k, metric, chunk=chunk)
    assert np.array_equal(got[1], one[1]), chunk
    assert got[0].tobytes() == one[0].tobytes(), chunk
  again = _search(qd, gd, k, metric)
  assert again[0].tobytes() == one[0].tobytes() and np.array_equal(again[1], one[1])
  if q == 70:      # a pair's distance does not depend on the query tile either: the first 5 and 40 queries searched alone
    for sub in (5, 40):
      part = _search(qd[:sub].contiguous(), gd, k, metric)
      assert part[0].tobytes() == one[0][:sub].tobytes() and np.array_equal(part[1], one[1][:sub]), sub


def test_index_offset_beyond_32_bits_and_query_ids():
  off = 1 << 33
  q, n, d, k = 40, 300, 32, 5
  _, ga = _ints(31, q, n, d)
  ga += np.arange(n, dtype=np.float32)[:, None] % 3      # still integers, fewer exact duplicates
  qa = ga[:q].copy()      # the set against itself
  gd, qd = _dev(ga, torch.bfloat16), _dev(qa, torch.bfloat16)
  dist = R.sq_l2_int(qa, ga)
  got_d, got_i = _search(qd, gd, k, chunk=128, index_offset=off)
  want_d, want_i = R.topk(dist, k, index_offset=off)
  assert np.array_equal(got_i, want_i) and got_i.min() >= off and np.array_equal(got_d.astype(np.float64), want_d)
  assert np.all(got_d[:, 0] == 0)      # every query finds itself (or an exact duplicate with a lower index) at distance 0
  ids = torch.arange(q, dtype=torch.int64, device=DEV) + off
  got_d, got_i = _search(qd, gd, k, chunk=128, index_offset=off, query_ids=ids)
  want_d, want_i = R.topk(dist, k, index_offset=off, query_ids=ids.cpu().numpy())
  assert np.array_equal(got_i, want_i) and np.array_equal(got_d.astype(np.float64), want_d)
  for i in range(q):      # exactly the self match is gone: the rest of the unrestricted list moves up
    full = R.topk(dist[i:i + 1], k + 1, index_offset=off)[1][0].tolist()
    full.remove(off + i)
    assert got_i[i].tolist() == full[:k]


@pytest.mark.parametrize('dtype', list(DTYPES))
@pytest.mark.parametrize('metric', ['l2', 'cosine'])
def test_nan_and_inf_rows_are_never_returned_ahead_of_finite_rows(dtype, metric):
  q, n, d, k = 9, 200, 48, 8
  qa, ga = _reals(41, q, n, d, DTYPES[dtype])
  ga[5, 7] = np.nan
  ga[130, 0] = np.inf
  ga[131, 3] = -np.inf
  got_d, got_i = _search(_dev(qa, DTYPES[dtype]), _dev(ga, DTYPES[dtype]), k, metric, chunk=64)
  assert np.all(np.isfinite(got_d)) and not np.isin(got_i, [5, 130, 131]).any()
  keep = np.ones(n, dtype=bool)
  keep[[5, 130, 131]] = False
  ref, bound = (R.sq_l2(qa, ga[keep]), R.sq_l2_bound(qa, ga[keep])) if metric == 'l2' else (R.cosine(qa, ga[keep]), R.cosine_bound(qa, ga[keep]))
  R.check_real(got_d, np.searchsorted(np.flatnonzero(keep), got_i), ref, bound, k)
  # a gallery of nothing else: the table stays the filler, and a NaN in the incoming table is not kept
  from twingan_amd import ops
  bad = _dev(ga[[5, 130, 131]], DTYPES[dtype])
  dist, idx = ops.knn_table(q, k, DEV)
  dist[0, 0] = float('nan')
  idx[0, 0] = 77
  ops.knn_topk(_dev(qa, DTYPES[dtype]), bad, k, metric, out=(dist, idx))
  torch.cuda.synchronize()
  assert bool(torch.isinf(dist).all()) and bool((idx == -1).all())


def test_bad_arguments_are_refused():
  from twingan_amd import _lib, ops
  q = torch.zeros(4, 16, dtype=torch.bfloat16, device=DEV)
  g = torch.zeros(10, 16, dtype=torch.bfloat16, device=DEV)
  for k in (0, 33):
    with pytest.raises(_lib.TgError, match='k = %d' % k):
      ops.knn_topk(q, g, k)
  with pytest.raises(_lib.TgError, match='d = 0'):
    ops.knn_topk(q[:, :0].contiguous(), g[:, :0].contiguous(), 3)
  with pytest.raises(_lib.TgError, match='float16'):
    ops.knn_topk(q, g.to(torch.float16), 3)
  with pytest.raises(_lib.TgError, match='metric'):
    ops.knn_topk(q, g, 3, metric='l1')
  with pytest.raises(_lib.TgError):
    ops.knn_topk(q, g[:, :8].contiguous(), 3)
  with pytest.raises(_lib.TgError, match='dtype'):
    _lib.call('tg_knn_sqnorm', q.data_ptr(), 4, 16, 7, g.data_ptr(), ops._stream())


@pytest.mark.parametrize('dtype', list(DTYPES))
@pytest.mark.parametrize('shape', [(1, 1, 1, 1), (33, 257, 24, 8), (70, 333, 27, 32)], ids=lambda s: 'q%d_n%d_d%d_k%d' % s)
def test_guard_bands_and_poison_round_every_buffer(shape, dtype):
  """tests/guarded.py: the operands sit between NaN bytes and are unchanged afterwards, the workspace, the fresh table and the
  norms ops.py allocates sit between guard bytes that stay intact, and results agree with the ordinary run bit for bit.  d = 27
  and 24 take the scalar tail of the staging (27 on a base that is not 16-byte aligned row by row)."""
  from twingan_amd import ops
  q, n, d, k = shape
  qa, ga = _ints(51, q, n, d)
  qd, gd = _dev(qa, DTYPES[dtype]), _dev(ga, DTYPES[dtype])
  served = []
  A, B = guarded.check(lambda a, b: ops.knn_topk(a, b, k), [qd, gd], DEV, sync=torch.cuda.synchronize, served=served)
  assert len(served) >= 3, served      # dist, idx, workspace
  want_d, want_i = R.topk(R.sq_l2_int(qa, ga), k)
  assert np.array_equal(B[1].cpu().numpy(), want_i) and np.array_equal(B[0].cpu().numpy().astype(np.float64), want_d)
  # the in/out form on a running table, and row_sqnorm
  table = ops.knn_table(q, k, DEV)
  guarded.check(lambda a, b, dd, ii: ops.knn_topk(a, b, k, out=(dd, ii), index_offset=5), [qd, gd, table[0], table[1]], DEV,
                inout=(2, 3), sync=torch.cuda.synchronize)
  _, N = guarded.check(ops.row_sqnorm, [gd], DEV, sync=torch.cuda.synchronize)
  assert np.array_equal(N.cpu().numpy().astype(np.int64), (ga.astype(np.int64) ** 2).sum(1))


# ------------------------------------------------------------------------------------------------ the encoder and the CSV
def _encoder(norm, precision='fp32', seed=3):
  from oracle import torch_ref as OR      # checker only
  from twingan_amd import Config
  from twingan_amd.embed import ContentEncoder
  cfg = Config(hw=16, max_ch=8, precision=precision, generator_norm_type=norm)
  rcfg = OR.Config(hw=16, max_ch=8, norm=norm, is_training=False)
  Pref = OR.init_params(rcfg, seed=seed, dtype=torch.float64, std='he')
  sd = {k: v.float() for k, v in Pref.items()}
  enc = ContentEncoder(cfg, sd, DEV)
  return cfg, rcfg, enc, {k: v.float().double() for k, v in Pref.items()}, OR


@pytest.mark.parametrize('norm', ['instance_norm', 'batch_norm'])
def test_content_encoder_is_the_inference_forward_and_the_oracles_encoder(norm):
  import dataclasses
  from twingan_amd import twingan as T
  cfg, rcfg, enc, Pref, OR = _encoder(norm)
  g = torch.Generator().manual_seed(9)
  s, t = torch.rand(3, 16, 16, 3, generator=g), torch.rand(3, 16, 16, 3, generator=g)
  sd, td = s.to(DEV), t.to(DEV)
  es, et = enc.encode(sd, 's'), enc.encode(td, 't')
  assert es.shape == (3, 16 * 8) == (3, enc.dim) and es.dtype == torch.float32
  # the trainer's forward under the inference configuration, on the same variables
  with torch.no_grad(), torch.cuda.device(enc.device):
    o = T.forward_generators(enc.store.P, sd, td, dataclasses.replace(cfg, is_training=False))
  torch.cuda.synchronize()
  assert torch.equal(es, o['es'].contiguous().reshape(3, -1)) and torch.equal(et, o['et'].contiguous().reshape(3, -1))
  # the oracle's encoder: the end-point tolerance of tests/test_gpu_model.py::test_networks_fp32_forward
  for x, dom, got in ((s, 's', es), (t, 't', et)):
    with torch.no_grad():
      want, _ = OR.encoder(Pref, x.double(), dom, rcfg)
    want = want.reshape(3, -1).numpy()      # NHWC, flattened
    err = float(np.linalg.norm(got.double().cpu().numpy() - want) / (np.linalg.norm(want) + 1e-30))
    assert err < 2e-5, (norm, dom, err)
  # numpy images go through preprocess() and give the same rows
  assert torch.equal(enc.encode(s.numpy(), 's'), es)


def test_export_read_search_round_trip(tmp_path):
  from twingan_amd import embed
  cfg, _, enc, _, _ = _encoder('instance_norm')
  g = torch.Generator().manual_seed(17)
  images = torch.rand(64, 16, 16, 3, generator=g)
  names = ['img_%03d.png' % i for i in range(64)]
  path = str(tmp_path / 'emb.csv')
  batches = [(names[lo:lo + 24], images[lo:lo + 24].to(DEV)) for lo in range(0, 64, 24)]
  assert embed.export_embeddings(enc, batches[:1], 's', path) == 24
  assert embed.export_embeddings(enc, batches[1:], 's', path) == 40      # appends
  got_names, emb = embed.read_embeddings(path)
  assert got_names == names and emb.shape == (64, enc.dim) and emb.dtype == np.float32
  direct = torch.cat([enc.encode(b, 's') for _, b in batches]).cpu().numpy()
  assert emb.tobytes() == direct.tobytes()      # float32 bit for bit through the text
  assert np.unique(emb, axis=0).shape[0] == 64
  e = torch.from_numpy(emb).to(DEV)
  nn = embed.NearestNeighbours(e, 4)
  for lo in range(0, 64, 20):
    nn.feed(e[lo:lo + 20])
  dist, idx = nn.end()
  assert idx[:, 0].tolist() == list(range(64)) and np.all(dist[:, 0] == 0) and np.all(dist[:, 1] > 0)
  nn = embed.NearestNeighbours(e, 4, query_ids=np.arange(64))
  nn.feed(e)
  dist2, idx2 = nn.end()
  assert not (idx2 == np.arange(64)[:, None]).any()
  assert np.array_equal(idx2[:, :3], idx[:, 1:]) and dist2[:, :3].tobytes() == dist[:, 1:].tobytes()
  # the blog's use: a portrait against both domains' galleries
  res = embed.cross_domain_neighbours(enc, images[:5].to(DEV), 's', {'s': e, 't': [e[:40], e[40:]]}, 3)
  assert set(res) == {'s', 't'} and res['s'][1][:, 0].tolist() == [0, 1, 2, 3, 4] and np.array_equal(res['s'][1], res['t'][1])


def test_content_encoder_from_checkpoint_plain_and_averaged(tmp_path):
  """from_checkpoint reads what ImageInferer.from_checkpoint reads: the variables of a saved trainer give the rows its own
  state dict gives, bit for bit, and moving_average=True the rows of its averaged weights (which differ after training)."""
  from twingan_amd import Config
  from twingan_amd import checkpoint as ckpt
  from twingan_amd.embed import ContentEncoder
  from twingan_amd.twingan import Trainer
  cfg = Config(hw=16, max_ch=8, precision='fp32', loss_architecture='wgan', generator_norm_type='batch_norm', moving_average_decay=0.9)
  g = torch.Generator().manual_seed(23)
  s, t = torch.rand(2, 16, 16, 3, generator=g).to(DEV), torch.rand(2, 16, 16, 3, generator=g).to(DEV)
  tr = Trainer(cfg, device=DEV, seed=6)
  for _ in range(2):
    tr.run(s, t)
  ckpt.save(tr, str(tmp_path / 'run'))
  live = ContentEncoder(cfg, tr.store.state_dict(include_state=True), DEV).encode(s, 's')
  avg = ContentEncoder(cfg, tr.store.averaged_state_dict(), DEV).encode(s, 's')
  tr.close()
  from_file = ContentEncoder.from_checkpoint(cfg, str(tmp_path / 'run'), DEV)
  assert isinstance(from_file, ContentEncoder) and torch.equal(from_file.encode(s, 's'), live)
  from_avg = ContentEncoder.from_checkpoint(cfg, str(tmp_path / 'run'), device=DEV, moving_average=True)
  assert torch.equal(from_avg.encode(s, 's'), avg) and not torch.equal(avg, live)
  # a device tensor of query_ids is taken as it is, and end() returns what the table holds
  from twingan_amd import embed
  ids = torch.arange(2, dtype=torch.int64, device=DEV)
  nn = embed.NearestNeighbours(live, 1, query_ids=ids)
  assert nn.query_ids.data_ptr() == ids.data_ptr()
  table = nn.feed(live)
  dist, idx = nn.end()
  assert idx[:, 0].tolist() == [1, 0] and np.array_equal(dist, table[0].cpu().numpy()) and np.array_equal(idx, table[1].cpu().numpy())
