// The case table of bounds_main.cpp (included into its anonymous namespace).  Shapes are the smallest members of the
// suite's own tables (CONV_CASES, the cheap rows of EDGE_CASES, the chunk-edge, flash, loss-sum, spectral-norm, SWD and
// MS-SSIM cases of tests/test_gpu_ops.py and friends) plus, per family, extents off the tile, channel counts one above and
// below the group width, numel of a vector +- 1, n = 1 and an odd batch, groups of 2 and 3 and nb != n.
// Sizes come from include/twingan_hip.h alone.

// ------------------------------------------------------------------------------------------------------------- convs
struct ConvShape {
  int n, h, w, cin, cout, k, valid;
};

TgConvDesc conv_desc(const ConvShape& s, int dtype, int algo, int groups = 0, int epilogue = 0) {
  TgConvDesc d;
  memset(&d, 0, sizeof(d));
  d.n = s.n, d.hin = s.h, d.win = s.w, d.cin = s.cin, d.cout = s.cout, d.kh = d.kw = s.k;
  d.hout = s.valid ? s.h - s.k + 1 : s.h, d.wout = s.valid ? s.w - s.k + 1 : s.w;
  d.pad_t = d.pad_l = s.valid ? 0 : (s.k - 1) / 2;
  d.dtype = dtype, d.algo = algo, d.epilogue = epilogue, d.lrelu_alpha = 0.2f, d.groups = groups;
  return d;
}

struct ConvBufs {
  size_t nx, ny, nw, G;
};
ConvBufs conv_sizes(const TgConvDesc& d) {
  ConvBufs b;
  b.G = d.groups > 1 ? d.groups : 1;
  b.nx = (size_t)d.n * d.hin * d.win * d.cin;
  b.ny = (size_t)d.n * d.hout * d.wout * d.cout;
  b.nw = b.G * d.kh * d.kw * d.cin * d.cout;
  return b;
}

// the weight operand of a conv call: the fp32 master for the direct algorithm, a pack of `mode` otherwise (made by the
// library into a buffer of exactly tg_conv2d_pack_elems elements)
const void* conv_weight(Ctx& c, const TgConvDesc& d, int mode) {
  const ConvBufs b = conv_sizes(d);
  float* wm = (float*)c.in("w", b.nw, F32);
  for (size_t i = 0; i < b.nw; ++i) wm[i] *= 0.25f;
  if (d.algo == TG_ALGO_DIRECT) return wm;
  const size_t pe = tg_conv2d_pack_elems(&d, mode);
  if (!pe) throw Fail{"tg_conv2d_pack_elems returned 0"};
  void* pk = c.in("w_pack", pe, d.dtype);
  need(tg_conv2d_pack_weights(&d, wm, mode, pk, nullptr), "tg_conv2d_pack_weights (preparing)");
  return pk;
}

enum ConvOp { C_FWD, C_FWD_BIAS, C_FWD_MASKED, C_FWD_STATS, C_FWD_POOL, C_FWD_POOL_SIGNS, C_BWD_DATA, C_BWD_DATA_MASKED,
              C_UNPOOL, C_UNPOOL_KEEP, C_UNPOOL_ACT, C_WGRAD, C_WGRAD_NOWS, C_WGRAD_ACC, C_WGRAD_BIAS, C_WGRAD2, C_WGRAD2_BIAS,
              C_PACK0, C_PACK1, C_PACK_MULTI };
const char* const CONV_OP_NAMES[] = {"fwd", "fwd_bias_lrelu", "fwd_masked", "fwd_stats", "fwd_pool", "fwd_pool_signs", "bwd_data",
                                     "bwd_data_masked", "bwd_data_unpool", "bwd_data_unpool_keep", "bwd_data_unpool_act", "bwd_weight",
                                     "bwd_weight_nows", "bwd_weight_acc", "bwd_weight_bias", "bwd_weight2", "bwd_weight2_bias", "pack0",
                                     "pack1", "pack_multi"};

void conv_run(Ctx& c, ConvOp op, const ConvShape& s, int dtype, int algo, int groups, int nb) {
  TgConvDesc d = conv_desc(s, dtype, algo, groups, op == C_FWD_BIAS || op == C_FWD_POOL || op == C_FWD_POOL_SIGNS ? (TG_EPI_BIAS | TG_EPI_LRELU) : 0);
  const ConvBufs b = conv_sizes(d);
  const size_t npool = (size_t)d.n * (d.hout / 2) * (d.wout / 2) * d.cout;
  switch (op) {
    case C_FWD:
    case C_FWD_BIAS: {
      const void* x = c.in("x", b.nx, dtype);
      const void* w = conv_weight(c, d, 0);
      const float* bias = op == C_FWD_BIAS ? (const float*)c.in("bias", b.G * d.cout, F32) : nullptr;
      void* y = c.out("y", b.ny, dtype);
      c.go();
      need(tg_conv2d_fwd(&d, x, w, bias, y, nullptr), "tg_conv2d_fwd");
      break;
    }
    case C_FWD_MASKED: {
      const void* x = c.in("x", b.nx, dtype);
      const void* w = conv_weight(c, d, 0);
      const void* m = c.in("mask_src", b.ny, dtype);
      void* y = c.out("y", b.ny, dtype);
      c.go();
      need(tg_conv2d_fwd_masked(&d, x, w, m, y, nullptr), "tg_conv2d_fwd_masked");
      break;
    }
    case C_FWD_STATS: {
      const int chunks = tg_conv2d_fwd_stats_chunks(&d);
      if (chunks <= 0) throw Fail{"tg_conv2d_fwd_stats_chunks: no statistics epilogue at this shape"};
      const void* x = c.in("x", b.nx, dtype);
      const void* w = conv_weight(c, d, 0);
      void* y = c.out("y", b.ny, dtype);
      float* part = (float*)c.out("partials", (size_t)d.n * chunks * 2 * d.cout, F32);
      c.go();
      need(tg_conv2d_fwd_stats(&d, x, w, y, part, chunks, nullptr), "tg_conv2d_fwd_stats");
      break;
    }
    case C_FWD_POOL:
    case C_FWD_POOL_SIGNS: {
      if (!tg_conv2d_fwd_pool_supported(&d)) throw Fail{"tg_conv2d_fwd_pool_supported: 0"};
      const void* x = c.in("x", b.nx, dtype);
      const void* w = conv_weight(c, d, 0);
      const float* bias = (const float*)c.in("bias", b.G * d.cout, F32);
      void* y = op == C_FWD_POOL ? c.out("y", b.ny, dtype) : c.out("y_signs", b.ny / 8, U8);
      void* yp = c.out("y_pooled", npool, dtype);
      c.go();
      if (op == C_FWD_POOL) need(tg_conv2d_fwd_pool(&d, x, w, bias, y, yp, nullptr), "tg_conv2d_fwd_pool");
      else need(tg_conv2d_fwd_pool_signs(&d, x, w, bias, y, yp, nullptr), "tg_conv2d_fwd_pool_signs");
      break;
    }
    case C_BWD_DATA:
    case C_BWD_DATA_MASKED: {
      const void* gy = c.in("gy", b.ny, dtype);
      const void* w = conv_weight(c, d, 1);
      const void* xa = op == C_BWD_DATA_MASKED ? c.in("x_act", b.nx, dtype) : nullptr;
      void* gx = c.out("gx", b.nx, dtype);
      c.go();
      if (xa) need(tg_conv2d_bwd_data_masked(&d, gy, w, xa, gx, nullptr), "tg_conv2d_bwd_data_masked");
      else need(tg_conv2d_bwd_data(&d, gy, w, gx, nullptr), "tg_conv2d_bwd_data");
      break;
    }
    case C_UNPOOL:
    case C_UNPOOL_KEEP:
    case C_UNPOOL_ACT: {
      if (!tg_conv2d_bwd_data_unpool_supported(&d)) throw Fail{"tg_conv2d_bwd_data_unpool_supported: 0"};
      const void* gyp = c.in("gy_pooled", npool, dtype);
      const void* sg = op == C_UNPOOL_ACT ? c.in("y_act", b.ny, dtype) : c.in("y_signs", b.ny / 8, U8);
      const void* w = conv_weight(c, d, 1);
      const void* xa = c.in("x_act", b.nx, dtype);
      void* gx = c.out("gx", b.nx, dtype);
      void* gyo = op == C_UNPOOL ? nullptr : c.out("gy_out", b.ny, dtype);
      c.go();
      if (op == C_UNPOOL_ACT) need(tg_conv2d_bwd_data_unpool_act(&d, gyp, sg, w, xa, gx, gyo, nullptr), "tg_conv2d_bwd_data_unpool_act");
      else need(tg_conv2d_bwd_data_unpool(&d, gyp, sg, w, xa, gx, gyo, nullptr), "tg_conv2d_bwd_data_unpool");
      break;
    }
    case C_WGRAD:
    case C_WGRAD_NOWS:
    case C_WGRAD_ACC:
    case C_WGRAD_BIAS: {
      const void* x = c.in("x", b.nx, dtype);
      const void* gy = c.in("gy", b.ny, dtype);
      const int acc = op == C_WGRAD_ACC;
      float* gw = (float*)(acc ? c.inout("gw", b.nw, F32) : c.out("gw", b.nw, F32));
      float* gb = op == C_WGRAD_BIAS ? (float*)c.inout("gbias", b.G * d.cout, F32) : nullptr;      // always ADDS
      const size_t wsb = op == C_WGRAD_NOWS ? 0 : tg_conv2d_bwd_weight_workspace(&d);
      void* ws = c.scratch("workspace", wsb);
      c.go();
      if (gb) need(tg_conv2d_bwd_weight_bias(&d, x, gy, gw, gb, acc, ws, wsb, nullptr), "tg_conv2d_bwd_weight_bias");
      else need(tg_conv2d_bwd_weight(&d, x, gy, gw, acc, ws, wsb, nullptr), "tg_conv2d_bwd_weight");
      break;
    }
    case C_WGRAD2:
    case C_WGRAD2_BIAS: {
      const size_t wsb = tg_conv2d_bwd_weight2_workspace(&d, nb);
      if (!wsb) throw Fail{"tg_conv2d_bwd_weight2_workspace: layer not eligible"};
      const void* xa = c.in("xa", b.nx, dtype);
      const void* gya = c.in("gya", b.ny, dtype);
      const void* xb = c.in("xb", b.nx / d.n * nb, dtype);
      const void* gyb = c.in("gyb", b.ny / d.n * nb, dtype);
      float* gw = (float*)c.out("gw", b.nw, F32);
      float* gb = op == C_WGRAD2_BIAS ? (float*)c.inout("gbias", b.G * d.cout, F32) : nullptr;
      void* ws = c.scratch("workspace", wsb);
      c.go();
      if (gb) need(tg_conv2d_bwd_weight2_bias(&d, nb, xa, gya, xb, gyb, gw, gb, 1, 0, ws, wsb, nullptr), "tg_conv2d_bwd_weight2_bias");
      else need(tg_conv2d_bwd_weight2(&d, nb, xa, gya, xb, gyb, gw, 0, ws, wsb, nullptr), "tg_conv2d_bwd_weight2");
      break;
    }
    case C_PACK0:
    case C_PACK1: {
      const int mode = op == C_PACK1;
      const float* wm = (const float*)c.in("w", b.nw, F32);
      (void)tg_conv2d_pack_layout(&d, mode);
      void* pk = c.out("w_pack", tg_conv2d_pack_elems(&d, mode), dtype);
      c.go();
      need(tg_conv2d_pack_weights(&d, wm, mode, pk, nullptr), "tg_conv2d_pack_weights");
      break;
    }
    case C_PACK_MULTI: {      // one job per weight set and mode, as twingan_amd/ops.py PackCache.refresh builds the table
      const float* wm = (const float*)c.in("w", b.nw, F32);
      const size_t pe0 = tg_conv2d_pack_elems(&d, 0), pe1 = tg_conv2d_pack_elems(&d, 1);
      char* p0 = (char*)c.out("w_pack0", pe0, dtype);
      char* p1 = (char*)c.out("w_pack1", pe1, dtype);
      const int njobs = 2 * (int)b.G;
      std::vector<unsigned char> host(tg_pack_table_bytes(njobs));
      int32_t blocks = 0;
      const size_t wset = b.nw / b.G;
      for (int j = 0; j < njobs; ++j) {
        const int g = j / 2, mode = j & 1;
        char* dst = (mode ? p1 + g * (pe1 / b.G) * 2 : p0 + g * (pe0 / b.G) * 2);
        need(tg_pack_table_fill(&d, wm + g * wset, mode, dst, j, host.data(), &blocks), "tg_pack_table_fill");
      }
      const void* table = c.in_bytes("table", host.data(), host.size());
      c.go();
      need(tg_conv2d_pack_weights_multi(table, njobs, blocks, nullptr), "tg_conv2d_pack_weights_multi");
      break;
    }
  }
  if (op < C_PACK0) c.kernel();
}

// tg_wgrad_defer / tg_wgrad_defer_flush: an accumulating filter gradient whose split-K slab reduction is queued, then issued
// by the flush from the workspace and the gradient buffer the call left behind
void wgrad_deferred(Ctx& c, const ConvShape& s, int dtype) {
  TgConvDesc d = conv_desc(s, dtype, TG_ALGO_MFMA);
  const ConvBufs b = conv_sizes(d);
  const void* x = c.in("x", b.nx, dtype);
  const void* gy = c.in("gy", b.ny, dtype);
  float* gw = (float*)c.inout("gw", b.nw, F32);
  const size_t wsb = tg_conv2d_bwd_weight_workspace(&d);
  void* ws = c.scratch("workspace", wsb);
  c.go();
  tg_wgrad_defer(1);
  const int rc = tg_conv2d_bwd_weight(&d, x, gy, gw, 1, ws, wsb, nullptr);
  const int issued = tg_wgrad_defer_flush(nullptr);
  tg_wgrad_defer(0);
  need(rc, "tg_conv2d_bwd_weight (deferred)");
  if (issued < 0) throw Fail{"tg_wgrad_defer_flush failed"};
  printf("deferred reductions issued by the flush: %d\n", issued);
  c.kernel();
}

void add_conv(ConvOp op, const char* tag, const ConvShape& s, int dtype, int algo, int groups = 0, int nb = 0) {
  char name[200];
  snprintf(name, sizeof name, "conv_%s.%s.%s.%s.n%d_%dx%d_c%d_%d_k%d%s%s", CONV_OP_NAMES[op], tag, algo == TG_ALGO_DIRECT ? "direct" : "mfma",
           dname(dtype), s.n, s.h, s.w, s.cin, s.cout, s.k, s.valid ? "v" : "s",
           groups > 1 ? (std::string("_g") + std::to_string(groups)).c_str() : nb ? (std::string("_nb") + std::to_string(nb)).c_str() : "");
  add(name, [=](Ctx& c) { conv_run(c, op, s, dtype, algo, groups, nb); });
}

void register_conv_cases() {
  // direct kernels: CONV_CASES at their smallest members, odd extents, the last image of an odd batch, every storage type
  const ConvShape direct[] = {{2, 6, 6, 5, 7, 3, 0}, {1, 9, 5, 3, 4, 3, 0}, {2, 5, 5, 4, 6, 1, 0}, {3, 4, 4, 5, 6, 4, 1}, {2, 7, 7, 3, 5, 4, 1}};
  const ConvOp direct_ops[] = {C_FWD, C_FWD_BIAS, C_FWD_MASKED, C_BWD_DATA, C_BWD_DATA_MASKED, C_WGRAD, C_WGRAD_NOWS, C_WGRAD_ACC, C_WGRAD_BIAS};
  for (const ConvShape& s : direct)
    for (int dt : {TG_F32, TG_BF16, TG_F16})
      for (ConvOp op : direct_ops) {
        if (dt != TG_F32 && &s != &direct[1] && &s != &direct[3]) continue;      // 16-bit direct: the 9x5 and the VALID odd batch
        add_conv(op, "cases", s, dt, TG_ALGO_DIRECT);
      }
  // (a group's slice of every operand must itself be 16-byte aligned: channel counts of 4 floats / 8 halves)
  add_conv(C_FWD, "groups", {4, 5, 3, 4, 4, 3, 0}, TG_F32, TG_ALGO_DIRECT, 2);
  add_conv(C_FWD_BIAS, "groups", {3, 5, 3, 4, 4, 3, 0}, TG_F32, TG_ALGO_DIRECT, 3);
  add_conv(C_BWD_DATA, "groups", {3, 5, 3, 8, 8, 3, 0}, TG_BF16, TG_ALGO_DIRECT, 3);
  add_conv(C_WGRAD_BIAS, "groups", {4, 5, 3, 4, 4, 3, 0}, TG_F32, TG_ALGO_DIRECT, 2);
  add_conv(C_WGRAD, "groups", {3, 5, 3, 8, 8, 3, 0}, TG_F16, TG_ALGO_DIRECT, 3);

  // MFMA paths: cin / cout one group (8) above and below a 16 / 32 / 64 channel block, maps off the tile, n = 1 and odd n
  const ConvShape mfma[] = {
      {2, 8, 8, 16, 16, 3, 0},       // CONV_CASES' MFMA member: whole-image kernel
      {1, 9, 5, 8, 24, 3, 0},        // off every tile, cout below 32
      {3, 6, 10, 24, 40, 3, 0},      // odd batch, cin 24 (conv_img refuses it), cout one group above 32
      {1, 5, 7, 40, 8, 1, 0},        // 1x1, cin above 32, cout of one group
      {3, 4, 4, 8, 8, 4, 1},         // the dense 4x4 VALID layer
      {1, 16, 16, 56, 72, 3, 0},     // one group below / above 64
  };
  // (the header allows NULL / 0 only where the workspace query returns 0: the direct algorithm, above.  The MFMA filter
  // gradients refuse it -- "workspace too small (0 < 6912)", TG_EINVAL -- as do the other workspace-taking entry points)
  const ConvOp mfma_ops[] = {C_FWD, C_FWD_BIAS, C_FWD_MASKED, C_BWD_DATA, C_BWD_DATA_MASKED, C_WGRAD, C_WGRAD_ACC, C_WGRAD_BIAS,
                             C_PACK0, C_PACK1};
  for (const ConvShape& s : mfma)
    for (int dt : {TG_BF16, TG_F16})
      for (ConvOp op : mfma_ops) {
        if (dt == TG_F16 && &s != &mfma[1] && &s != &mfma[2]) continue;
        add_conv(op, "edges", s, dt, TG_ALGO_MFMA);
      }
  add_conv(C_FWD, "v1", {1, 9, 5, 8, 24, 3, 0}, TG_BF16, TG_ALGO_MFMA_V1);
  add_conv(C_BWD_DATA, "v1", {1, 9, 5, 8, 24, 3, 0}, TG_BF16, TG_ALGO_MFMA_V1);
  // the rows of EDGE_CASES (tests/test_gpu_ops.py), both sides of their thresholds, at the batch the table names
  for (int dt : {TG_BF16, TG_F16}) {
    for (int n : {64, 65})
      for (ConvOp op : {C_FWD, C_FWD_MASKED, C_BWD_DATA, C_BWD_DATA_MASKED}) {
        add_conv(op, "small_k1_hw8", {n, 8, 8, 32, 32, 1, 0}, dt, TG_ALGO_MFMA);
        add_conv(op, "small_k3_hw8_c24", {n, 8, 8, 24, 40, 3, 0}, dt, TG_ALGO_MFMA);
      }
    for (int n : {256, 257})
      for (ConvOp op : {C_FWD, C_FWD_MASKED, C_FWD_STATS, C_BWD_DATA, C_BWD_DATA_MASKED}) {
        if (op == C_FWD_STATS && n == 257) continue;      // above the threshold the dispatched kernel has no statistics epilogue
        add_conv(op, "small_k3_hw4", {n, 4, 4, 32, 32, 3, 0}, dt, TG_ALGO_MFMA);
      }
    for (int n : {4096, 4097})
      for (ConvOp op : {C_FWD, C_FWD_MASKED, C_BWD_DATA, C_BWD_DATA_MASKED, C_WGRAD, C_WGRAD_BIAS}) add_conv(op, "dense", {n, 4, 4, 8, 8, 4, 1}, dt, TG_ALGO_MFMA);
  }
  // GROUPED_EDGE_CASES: the grouped call and its groups on either side of the same thresholds
  struct GE {
    const char* id;
    int G, k, valid, hw, cin, cout, n;
  };
  const GE grouped[] = {{"g2_k1_hw8_under", 2, 1, 0, 8, 32, 32, 64},  {"g3_k1_hw8_under", 3, 1, 0, 8, 32, 32, 48},  {"g2_k3_hw4_under", 2, 3, 0, 4, 32, 32, 256},
                        {"g3_k3_hw4_under", 3, 3, 0, 4, 32, 32, 240}, {"g2_dense_under", 2, 4, 1, 4, 8, 8, 384},    {"g2_k1_hw8_n96", 2, 1, 0, 8, 32, 32, 96},
                        {"g3_k1_hw8_n96", 3, 1, 0, 8, 32, 32, 96},    {"g2_k3_hw4_n264", 2, 3, 0, 4, 32, 32, 264},  {"g2_k3_hw4_n384", 2, 3, 0, 4, 32, 32, 384},
                        {"g3_k3_hw4_n600", 3, 3, 0, 4, 32, 32, 600},  {"g2_dense_n8192", 2, 4, 1, 4, 8, 8, 8192},   {"g3_dense_n6144", 3, 4, 1, 4, 8, 8, 6144},
                        {"g2_k1_hw8_over", 2, 1, 0, 8, 32, 32, 130},  {"g3_k1_hw8_over", 3, 1, 0, 8, 32, 32, 195},  {"g2_k3_hw4_over", 2, 3, 0, 4, 32, 32, 514},
                        {"g2_dense_over", 2, 4, 1, 4, 8, 8, 8194}};
  for (const GE& g : grouped)
    for (int dt : {TG_BF16, TG_F16})
      for (ConvOp op : {C_FWD, C_FWD_MASKED, C_BWD_DATA, C_BWD_DATA_MASKED}) add_conv(op, g.id, {g.n, g.hw, g.hw, g.cin, g.cout, g.k, g.valid}, dt, TG_ALGO_MFMA, g.G);
  for (int dt : {TG_BF16, TG_F16}) {
    for (int n : {64, 65})
      for (ConvOp op : {C_WGRAD, C_WGRAD_BIAS}) {
        add_conv(op, "small_k1_hw8", {n, 8, 8, 32, 32, 1, 0}, dt, TG_ALGO_MFMA);
        add_conv(op, "small_k3_hw8_c24", {n, 8, 8, 24, 40, 3, 0}, dt, TG_ALGO_MFMA);
      }
    for (int n : {256, 257})
      for (ConvOp op : {C_WGRAD, C_WGRAD_BIAS}) add_conv(op, "small_k3_hw4", {n, 4, 4, 32, 32, 3, 0}, dt, TG_ALGO_MFMA);
  }
  // The 128x128 rows of EDGE_CASES take 30-160 s per case over the sanitized emulation.  Every row on both sides of its
  // threshold: forward and backward-data in both storage types, the masked, statistics, pool, sign-byte and unpooling forms
  // in bf16.  Their f16 variants of those forms, their filter gradients and the grouped / upsample-concat rows at the
  // recorded batches are asserted on the device (tests/test_gpu_bounds.py test_edge_rows_*); BOUNDS_EXTRA=1 adds one case of
  // each kind left out, for timing by hand (tests/test_bounds_cpu.py DEVICE_ROWS quotes the figures).
  struct TR {
    const char* id;
    int k, cin, cout, n_lo, n_hi, stats, pool, unpool;
  };
  const TR tile_rows[] = {{"tile_bn", 3, 48, 64, 7, 8, 1, 1, 1},      {"tile_mt", 3, 64, 32, 7, 8, 1, 1, 1},      {"tile_wres16", 3, 16, 32, 15, 16, 1, 1, 1},
                          {"tile_wres32", 3, 32, 32, 15, 16, 1, 1, 1}, {"tile_thin16", 3, 16, 16, 15, 16, 1, 1, 0}, {"tile_k1_wres", 1, 32, 32, 15, 16, 0, 0, 0}};
  for (const TR& r : tile_rows)
    for (int n : {r.n_lo, r.n_hi}) {
      const ConvShape s = {n, 128, 128, r.cin, r.cout, r.k, 0};
      for (int dt : {TG_BF16, TG_F16})
        for (ConvOp op : {C_FWD, C_BWD_DATA}) add_conv(op, r.id, s, dt, TG_ALGO_MFMA);
      add_conv(C_FWD_MASKED, r.id, s, TG_BF16, TG_ALGO_MFMA);
      add_conv(C_BWD_DATA_MASKED, r.id, s, TG_BF16, TG_ALGO_MFMA);
      if (r.stats) add_conv(C_FWD_STATS, r.id, s, TG_BF16, TG_ALGO_MFMA);
      if (r.pool) add_conv(C_FWD_POOL, r.id, s, TG_BF16, TG_ALGO_MFMA);
      if (r.pool) add_conv(C_FWD_POOL_SIGNS, r.id, s, TG_BF16, TG_ALGO_MFMA);
      if (r.unpool) add_conv(C_UNPOOL_KEEP, r.id, s, TG_BF16, TG_ALGO_MFMA);
    }
  if (getenv("BOUNDS_EXTRA")) {
    add_conv(C_WGRAD_BIAS, "tile_wres16", {15, 128, 128, 16, 32, 3, 0}, TG_BF16, TG_ALGO_MFMA);
    add_conv(C_FWD, "g2_tile_n16", {16, 128, 128, 16, 32, 3, 0}, TG_BF16, TG_ALGO_MFMA, 2);
    add_conv(C_FWD, "g2_mbstd_c264_n264", {264, 4, 4, 264, 256, 3, 0}, TG_BF16, TG_ALGO_MFMA, 2);
  }
  // statistics, pool, sign bytes, unpool on the smallest maps the tile kernels take
  for (int dt : {TG_BF16, TG_F16}) {
    add_conv(C_FWD_STATS, "tile", {1, 8, 16, 32, 32, 3, 0}, dt, TG_ALGO_MFMA);
    add_conv(C_FWD_STATS, "tile", {3, 16, 16, 24, 40, 3, 0}, dt, TG_ALGO_MFMA);
    add_conv(C_FWD_POOL, "tile", {1, 8, 16, 8, 24, 3, 0}, dt, TG_ALGO_MFMA);
    add_conv(C_FWD_POOL, "tile", {3, 16, 16, 32, 40, 3, 0}, dt, TG_ALGO_MFMA);
    add_conv(C_FWD_POOL_SIGNS, "tile", {1, 8, 16, 8, 24, 3, 0}, dt, TG_ALGO_MFMA);
    add_conv(C_FWD_POOL_SIGNS, "tile", {3, 16, 16, 32, 40, 3, 0}, dt, TG_ALGO_MFMA);
    for (ConvOp op : {C_UNPOOL, C_UNPOOL_KEEP, C_UNPOOL_ACT}) {
      add_conv(op, "tile", {1, 8, 16, 24, 32, 3, 0}, dt, TG_ALGO_MFMA);
      add_conv(op, "tile", {3, 16, 16, 40, 64, 3, 0}, dt, TG_ALGO_MFMA);
    }
  }
  // groups of 2 and 3, the paired filter gradient with nb != n, the multi-pack table
  for (int G : {2, 3}) {
    const ConvShape s = {2 * G, 8, 16, 24, 40, 3, 0};
    for (ConvOp op : {C_FWD_BIAS, C_FWD_MASKED, C_BWD_DATA, C_BWD_DATA_MASKED, C_WGRAD, C_WGRAD_BIAS, C_FWD_POOL_SIGNS, C_PACK0, C_PACK1, C_PACK_MULTI})
      add_conv(op, "groups", s, G == 2 ? TG_BF16 : TG_F16, TG_ALGO_MFMA, G);
    add_conv(C_FWD, "groups_small", {3 * G, 4, 4, 32, 32, 3, 0}, TG_BF16, TG_ALGO_MFMA, G);
  }
  add_conv(C_UNPOOL_KEEP, "groups", {4, 8, 16, 24, 32, 3, 0}, TG_BF16, TG_ALGO_MFMA, 2);
  add_conv(C_PACK_MULTI, "single", {1, 9, 5, 8, 24, 3, 0}, TG_BF16, TG_ALGO_MFMA);
  for (int dt : {TG_BF16, TG_F16}) {
    add(std::string("conv_bwd_weight_deferred.") + dname(dt) + ".n3_6x10_c24_40", [=](Ctx& c) { wgrad_deferred(c, {3, 6, 10, 24, 40, 3, 0}, dt); });
    add(std::string("conv_bwd_weight_deferred.") + dname(dt) + ".n1_16x16_c56_72", [=](Ctx& c) { wgrad_deferred(c, {1, 16, 16, 56, 72, 3, 0}, dt); });
  }
  for (int dt : {TG_BF16, TG_F16}) {
    add_conv(C_WGRAD2, "pair", {2, 16, 16, 24, 40, 3, 0}, dt, TG_ALGO_MFMA, 0, 3);
    add_conv(C_WGRAD2_BIAS, "pair", {3, 8, 16, 32, 32, 3, 0}, dt, TG_ALGO_MFMA, 0, 1);
  }
}


// ---------------------------------------------------------------------------------- upsample-concat convs (16-bit only)
unsigned pack_perm(std::initializer_list<int> perm) {
  unsigned v = 0;
  int k = 0;
  for (int g : perm) v |= (unsigned)(g & 0xff) << (8 * k++);
  return v;
}

struct UpcatShape {
  int n, h, w, c0, c1, cout, gsz, n1;
  unsigned perm;
};

void register_upcat_cases() {
  // h % 8 == 0, w % 16 == 0, c0 / c1 % 32 == 0, cout % 8 == 0: the smallest map, cout one group above and below 32, n = 1,
  // an odd batch, and the grouped read of the skips (4 groups of 1 reading 2 skip images)
  const UpcatShape shapes[] = {{1, 8, 16, 32, 32, 24, 0, 1, 0}, {3, 16, 16, 32, 64, 40, 0, 3, 0}, {4, 8, 16, 64, 32, 8, 1, 2, pack_perm({1, 0, 0, 1})}};
  for (const UpcatShape& u : shapes)
    for (int dt : {TG_BF16, TG_F16}) {
      if (!tg_conv2d_upcat_supported(u.h, u.w, u.c0, u.c1, u.cout)) continue;
      char tag[120];
      snprintf(tag, sizeof tag, "%s.n%d_%dx%d_c%d+%d_%d_gsz%d", dname(dt), u.n, u.h, u.w, u.c0, u.c1, u.cout, u.gsz);
      const size_t n0 = (size_t)u.n * (u.h / 2) * (u.w / 2) * u.c0, n1 = (size_t)u.n1 * u.h * u.w * u.c1, ny = (size_t)u.n * u.h * u.w * u.cout;
      const size_t nw = (size_t)9 * (u.c0 + u.c1) * u.cout;
      const ConvShape cs = {u.n, u.h, u.w, u.c0 + u.c1, u.cout, 3, 0};
      auto pack = [=](Ctx& c, int mode) {
        TgConvDesc d = conv_desc(cs, dt, TG_ALGO_MFMA);
        return conv_weight(c, d, mode);
      };
      for (int stats = 0; stats < 2; ++stats)
        add(std::string(stats ? "upcat_fwd_stats." : "upcat_fwd.") + tag, [=](Ctx& c) {
          const void* x0 = c.in("x0", n0, dt);
          const void* x1 = c.in("x1", n1, dt);
          const void* w = pack(c, 0);
          void* y = c.out("y", ny, dt);
          if (stats) {
            const int chunks = tg_conv2d_upcat_fwd_stats_chunks(u.n, u.h, u.w, u.c0, u.c1, u.cout);
            if (chunks <= 0) throw Fail{"tg_conv2d_upcat_fwd_stats_chunks: 0"};
            float* part = (float*)c.out("partials", (size_t)u.n * chunks * 2 * u.cout, F32);
            c.go();
            need(tg_conv2d_upcat_fwd_stats(x0, x1, w, y, part, chunks, u.n, u.h, u.w, u.c0, u.c1, u.cout, u.gsz, u.perm, dt, nullptr),
                 "tg_conv2d_upcat_fwd_stats");
          } else {
            c.go();
            need(tg_conv2d_upcat_fwd(x0, x1, w, y, u.n, u.h, u.w, u.c0, u.c1, u.cout, u.gsz, u.perm, dt, nullptr), "tg_conv2d_upcat_fwd");
          }
          c.kernel();
        });
      for (int which = 0; which < 3; ++which)      // both gradients, g0 alone, g1 alone
        add(std::string("upcat_bwd_data.") + (which == 0 ? "both." : which == 1 ? "g0." : "g1.") + tag, [=](Ctx& c) {
          const void* gy = c.in("gy", ny, dt);
          const void* w = pack(c, 1);
          void* g0 = which != 2 ? c.out("g0", n0, dt) : nullptr;
          void* g1 = which != 1 ? c.out("g1", n1, dt) : nullptr;
          c.go();
          need(tg_conv2d_upcat_bwd_data(gy, w, g0, g1, u.n, u.h, u.w, u.c0, u.c1, u.cout, u.gsz, u.perm, dt, nullptr), "tg_conv2d_upcat_bwd_data");
          c.kernel();
        });
      for (int acc = 0; acc < 2; ++acc)
        add(std::string(acc ? "upcat_bwd_weight_acc." : "upcat_bwd_weight.") + tag, [=](Ctx& c) {
          const void* x0 = c.in("x0", n0, dt);
          const void* x1 = c.in("x1", n1, dt);
          const void* gy = c.in("gy", ny, dt);
          float* gw = (float*)(acc ? c.inout("gw", nw, F32) : c.out("gw", nw, F32));
          const size_t wsb = tg_conv2d_upcat_bwd_weight_workspace(u.n, u.h, u.w, u.c0, u.c1, u.cout);
          void* ws = c.scratch("workspace", wsb);
          c.go();
          need(tg_conv2d_upcat_bwd_weight(x0, x1, gy, gw, acc, ws, wsb, u.n, u.h, u.w, u.c0, u.c1, u.cout, u.gsz, u.perm, dt, nullptr),
               "tg_conv2d_upcat_bwd_weight");
          c.kernel();
        });
    }
}

// ---------------------------------------------------------------------------------------- pointwise (RGB-side) convs
void register_pointwise_cases() {
  struct S {
    int64_t npix;
    int cin, cout;
  };
  // npix 4099 and 35 (a vector tail; not a multiple of 4: off the RGB kernel's shape), 4096 (on it), channel counts of a
  // vector + 1 and - 1 on the wide side
  const S shapes[] = {{4099, 3, 16}, {4096, 3, 16}, {35, 3, 9}, {35, 7, 3}, {4099, 16, 3}, {4096, 32, 3}, {1, 3, 8}};
  for (const S& sh : shapes)
    for (int dt : {TG_F32, TG_BF16, TG_F16}) {
      char tag[80];
      snprintf(tag, sizeof tag, "%s.npix%d_c%d_%d", dname(dt), (int)sh.npix, sh.cin, sh.cout);
      const size_t nx = sh.npix * sh.cin, ny = sh.npix * sh.cout, nw = (size_t)sh.cin * sh.cout;
      for (int wt = 0; wt < 2; ++wt)
        add(std::string(wt ? "pointwise_fwd_wt." : "pointwise_fwd.") + tag, [=](Ctx& c) {
          const void* x = c.in("x", nx, dt);
          const float* w = (const float*)c.in("w", nw, F32);
          const float* b = (const float*)c.in("bias", sh.cout, F32);
          void* y = c.out("y", ny, dt);
          c.go();
          need(tg_pointwise_conv_fwd(x, w, wt ? nullptr : b, y, sh.npix, sh.cin, sh.cout, wt, wt ? 0 : (TG_EPI_BIAS | TG_EPI_LRELU), 0.2f, dt, nullptr),
               "tg_pointwise_conv_fwd");
        });
      if (sh.cin <= 4) {
        add(std::string("pointwise_fwd_masked.") + tag, [=](Ctx& c) {
          const void* x = c.in("x", nx, dt);
          const float* w = (const float*)c.in("w", nw, F32);
          const void* m = c.in("mask", ny, dt);
          void* y = c.out("y", ny, dt);
          c.go();
          need(tg_pointwise_conv_fwd_masked(x, w, m, y, sh.npix, sh.cin, sh.cout, 1, 0.2f, dt, nullptr), "tg_pointwise_conv_fwd_masked");
        });
        for (int acc = 0; acc < 2; ++acc)
          add(std::string(acc ? "pointwise_bwd_weight_bias_acc." : "pointwise_bwd_weight_bias.") + tag, [=](Ctx& c) {
            const void* x = c.in("x", nx, dt);
            const void* gy = c.in("gy", ny, dt);
            float* gw = (float*)(acc ? c.inout("gw", nw, F32) : c.out("gw", nw, F32));
            float* gb = (float*)(acc ? c.inout("gbias", sh.cout, F32) : c.out("gbias", sh.cout, F32));
            c.go();
            need(tg_pointwise_conv_bwd_weight_bias(x, gy, gw, gb, sh.npix, sh.cin, sh.cout, acc, dt, nullptr), "tg_pointwise_conv_bwd_weight_bias");
          });
      }
      for (int ordered = 0; ordered < 2; ++ordered)
        add(std::string(ordered ? "pointwise_bwd_weight_ordered." : "pointwise_bwd_weight.") + tag, [=](Ctx& c) {
          const void* x = c.in("x", nx, dt);
          const void* gy = c.in("gy", ny, dt);
          float* gw = (float*)c.out("gw", nw, F32);
          const size_t wsf = 256 * nw;
          float* ws = ordered ? (float*)c.scratch("workspace", wsf * 4) : nullptr;
          c.go();
          if (ordered) need(tg_pointwise_conv_bwd_weight_ordered(x, gy, gw, sh.npix, sh.cin, sh.cout, 0, ws, wsf, dt, nullptr), "tg_pointwise_conv_bwd_weight_ordered");
          else need(tg_pointwise_conv_bwd_weight(x, gy, gw, sh.npix, sh.cin, sh.cout, 0, dt, nullptr), "tg_pointwise_conv_bwd_weight");
        });
    }
}

// --------------------------------------------------------------------------------------------------------- normaliser
struct NormShape {
  int n, h, w, c, pool, split;      // split < 0: one domain
};

void register_norm_cases() {
  // the cheap rows of NORM_EDGE_CASES (tests/test_gpu_ops.py): tail chunks in both passes, the scalar path (c 3, 5, 24), the
  // wide vector path (c 256), pool, split at 0 / 1 / n - 1, n = 1
  const NormShape shapes[] = {{3, 40, 24, 16, 1, 1}, {5, 17, 13, 8, 0, 0}, {3, 5, 13, 24, 0, 1}, {3, 16, 16, 5, 1, -1}, {3, 1, 257, 5, 0, 2},
                              {3, 3, 86, 3, 0, 1}, {2, 34, 30, 256, 1, 1}, {1, 9, 5, 8, 0, -1}};
  for (const NormShape& s : shapes)
    for (int dt : {TG_F32, TG_BF16, TG_F16}) {
      if (dt == TG_F16 && s.c != 16 && s.c != 5) continue;
      char tag[80];
      snprintf(tag, sizeof tag, "%s.n%d_%dx%d_c%d_split%d", dname(dt), s.n, s.h, s.w, s.c, s.split);
      const size_t ne = (size_t)s.n * s.h * s.w * s.c, nc = (size_t)s.n * s.c, npix = (size_t)s.n * s.h * s.w;
      const size_t npool = (size_t)s.n * (s.h / 2) * (s.w / 2) * s.c;
      const bool pn_ok = s.c >= 8 && (s.c & (s.c - 1)) == 0;      // pixel norm takes c = 8 * 2^k only
      const int flags = pn_ok ? 3 : 1, split = s.split < 0 ? 0 : s.split;
      const bool two = s.split >= 0;
      add(std::string("instance_norm_stats.") + tag, [=](Ctx& c) {
        const void* y = c.in("y", ne, dt);
        float* mean = (float*)c.out("mean", nc, F32);
        float* rstd = (float*)c.out("rstd", nc, F32);
        c.go();
        need(tg_instance_norm_stats(y, mean, rstd, s.n, s.h, s.w, s.c, 1e-5f, dt, nullptr), "tg_instance_norm_stats");
      });
      for (int per_image = 0; per_image < 2; ++per_image)
        add(std::string(per_image ? "norm_act_fwd_per_image." : "norm_act_fwd.") + tag, [=](Ctx& c) {
          const void* y = c.in("y", ne, dt);
          const float* mean = (const float*)c.in("mean", nc, F32);
          const float* rstd = (const float*)c.in_pos("rstd", nc, F32);
          const float* ga = (const float*)c.in_pos("gamma", per_image ? nc : s.c, F32);
          const float* be = (const float*)c.in("beta", per_image ? nc : s.c, F32);
          const float* ga2 = two && !per_image ? (const float*)c.in_pos("gamma2", s.c, F32) : nullptr;
          const float* be2 = two && !per_image ? (const float*)c.in("beta2", s.c, F32) : nullptr;
          void* z = c.out("z", ne, dt);
          float* pn = pn_ok ? (float*)c.out("pn_scale", npix, F32) : nullptr;
          c.go();
          need(tg_norm_act_fwd(y, mean, rstd, ga, be, ga2, be2, split, per_image, z, pn, s.n, s.h, s.w, s.c, flags, 0.2f, 1e-8f, dt, nullptr),
               "tg_norm_act_fwd");
        });
      const int chunks = tg_norm_chunks(s.n, s.h, s.w);
      const size_t npart = (size_t)s.n * chunks * 2 * s.c;
      add(std::string("instance_norm_partials.") + tag, [=](Ctx& c) {
        const void* y = c.in("y", ne, dt);
        float* part = (float*)c.out("partials", npart, F32);
        c.go();
        need(tg_instance_norm_partials(y, part, s.n, s.h, s.w, s.c, dt, nullptr), "tg_instance_norm_partials");
      });
      for (int from_conv = 0; from_conv < 2; ++from_conv)
        add(std::string(from_conv ? "norm_act_fwd_conv_stats." : "norm_act_fwd_partials.") + tag, [=](Ctx& c) {
          const void* y = c.in("y", ne, dt);
          const int pc = from_conv ? 3 : chunks;
          float* part = (float*)c.in_const("partials", (size_t)s.n * pc * 2 * s.c, F32, 0.f);
          if (from_conv) {      // [n][3][2][c] unshifted: sums 0, sums of squares positive
            for (int i = 0; i < s.n * pc; ++i)
              for (int k = 0; k < s.c; ++k) part[((size_t)i * 2 + 1) * s.c + k] = 0.25f * s.h * s.w;
          } else {
            need(tg_instance_norm_partials(y, part, s.n, s.h, s.w, s.c, dt, nullptr), "tg_instance_norm_partials (preparing)");
          }
          float* mean = (float*)c.out("mean", nc, F32);
          float* rstd = (float*)c.out("rstd", nc, F32);
          const float* ga = (const float*)c.in_pos("gamma", s.c, F32);
          const float* be = (const float*)c.in("beta", s.c, F32);
          const float* ga2 = two ? (const float*)c.in_pos("gamma2", s.c, F32) : nullptr;
          const float* be2 = two ? (const float*)c.in("beta2", s.c, F32) : nullptr;
          void* z = c.out("z", ne, dt);
          void* zp = s.pool ? c.out("z_pooled", npool, dt) : nullptr;
          float* pn = pn_ok ? (float*)c.out("pn_scale", npix, F32) : nullptr;
          c.go();
          if (from_conv)
            need(tg_norm_act_fwd_conv_stats(y, part, pc, mean, rstd, ga, be, ga2, be2, split, z, zp, pn, s.n, s.h, s.w, s.c, flags, 0.2f, 1e-5f, 1e-8f,
                                            dt, nullptr), "tg_norm_act_fwd_conv_stats");
          else
            need(tg_norm_act_fwd_partials(y, part, mean, rstd, ga, be, ga2, be2, split, z, zp, pn, s.n, s.h, s.w, s.c, flags, 0.2f, 1e-5f, 1e-8f, dt,
                                          nullptr), "tg_norm_act_fwd_partials");
        });
      for (int mode = 0; mode < 3; ++mode)      // written gradients, accumulated gradients, per-image parameters
        add(std::string(mode == 0 ? "norm_act_bwd." : mode == 1 ? "norm_act_bwd_acc." : "norm_act_bwd_per_image.") + tag, [=](Ctx& c) {
          const bool per_image = mode == 2, acc = mode == 1;
          const void* gz = c.in("gz", ne, dt);
          const void* gzp = s.pool ? c.in("gz_pooled", npool, dt) : nullptr;
          const void* y = c.in("y", ne, dt);
          const float* pn = pn_ok ? (const float*)c.in_pos("pn_scale", npix, F32) : nullptr;
          const float* mean = (const float*)c.in("mean", nc, F32);
          const float* rstd = (const float*)c.in_pos("rstd", nc, F32);
          const size_t np = per_image ? nc : s.c;
          const float* ga = (const float*)c.in_pos("gamma", np, F32);
          const float* be = (const float*)c.in("beta", np, F32);
          const bool two2 = two && !per_image;
          const float* ga2 = two2 ? (const float*)c.in_pos("gamma2", s.c, F32) : nullptr;
          const float* be2 = two2 ? (const float*)c.in("beta2", s.c, F32) : nullptr;
          void* gy = c.out("gy", ne, dt);
          float* gg = (float*)(acc ? c.inout("ggamma", np, F32) : c.out("ggamma", np, F32));
          float* gb = (float*)(acc ? c.inout("gbeta", np, F32) : c.out("gbeta", np, F32));
          // (with split at 0 or n one of the two parameter sets sees no image: in/out, so that an untouched one is no finding)
          float* gg2 = two2 ? (float*)c.inout("ggamma2", s.c, F32) : nullptr;
          float* gb2 = two2 ? (float*)c.inout("gbeta2", s.c, F32) : nullptr;
          float* sums = (float*)c.scratch("sums", npart * 4);
          c.go();
          need(tg_norm_act_bwd(gz, gzp, y, pn, mean, rstd, ga, be, ga2, be2, split, gy, per_image, gg, gb, gg2, gb2, sums, s.n, s.h, s.w, s.c, flags,
                               0.2f, acc, dt, nullptr), "tg_norm_act_bwd");
        });
    }
}

// ------------------------------------------------------------------------ discriminator pointwise, resampling, fade-in
const int64_t NUMELS[] = {1, 7, 9, 4099};      // one 16-byte vector of halves - 1 and + 1 (fp32: two vectors), a long tail

void register_elementwise_cases() {
  for (int dt : {TG_F32, TG_BF16, TG_F16}) {
    const std::string dn = std::string(dname(dt)) + ".";
    for (int64_t numel : NUMELS) {
      const std::string tag = dn + "numel" + std::to_string(numel);
      add("lrelu_bwd." + tag, [=](Ctx& c) {
        const void* gz = c.in("gz", numel, dt);
        const void* z = c.in("z", numel, dt);
        void* gy = c.out("gy", numel, dt);
        c.go();
        need(tg_lrelu_bwd(gz, z, gy, numel, 0.2f, dt, nullptr), "tg_lrelu_bwd");
      });
      for (int two = 0; two < 2; ++two)
        add(std::string(two ? "axpby." : "axpby_one.") + tag, [=](Ctx& c) {
          const void* x = c.in("x", numel, dt);
          const void* y = two ? c.in("y", numel, dt) : nullptr;
          void* o = c.out("out", numel, dt);
          c.go();
          need(tg_axpby(x, y, o, numel, 0.25f, 0.75f, dt, nullptr), "tg_axpby");
        });
      add("fill_scaled." + tag, [=](Ctx& c) {
        const float* sc = (const float*)c.in_pos("scalar", 1, F32);
        void* o = c.out("out", numel, dt);
        c.go();
        need(tg_fill_scaled(o, sc, 0.5f, numel, dt, nullptr), "tg_fill_scaled");
      });
      for (int dst : {TG_F32, TG_BF16, TG_F16})
        if (dt == TG_F32 || dst == TG_F32)      // one side of a cast is fp32
        add("cast." + tag + "_to_" + dname(dst), [=](Ctx& c) {
          const void* x = c.in("src", numel, dt);
          void* o = c.out("dst", numel, dst);
          c.go();
          need(tg_cast(x, o, numel, dt, dst, nullptr), "tg_cast");
        });
      add("tanh_fwd." + tag, [=](Ctx& c) {
        const void* x = c.in("x", numel, dt);
        void* y = c.out("y", numel, dt);
        c.go();
        need(tg_tanh_fwd(x, y, numel, dt, nullptr), "tg_tanh_fwd");
      });
      add("tanh_bwd." + tag, [=](Ctx& c) {
        const void* g = c.in("g", numel, dt);
        const void* y = c.in("y", numel, dt);
        void* gx = c.out("gx", numel, dt);
        c.go();
        need(tg_tanh_bwd(g, y, gx, numel, dt, nullptr), "tg_tanh_bwd");
      });
      for (int three = 0; three < 2; ++three)
        add(std::string(three ? "mul3." : "mul2.") + tag, [=](Ctx& c) {
          const void* a = c.in("a", numel, dt);
          const void* b = c.in("b", numel, dt);
          const void* cc = three ? c.in("c", numel, dt) : nullptr;
          void* o = c.out("out", numel, dt);
          c.go();
          need(tg_mul3(a, b, cc, o, 0.5f, numel, dt, nullptr), "tg_mul3");
        });
      add("scale_dev." + tag, [=](Ctx& c) {
        const void* x = c.in("x", numel, dt);
        const float* sc = (const float*)c.in_pos("scalar", 1, F32);
        void* o = c.out("out", numel, dt);
        c.go();
        need(tg_scale_dev(x, sc, o, numel, dt, nullptr), "tg_scale_dev");
      });
      add("dot." + tag, [=](Ctx& c) {
        const void* a = c.in("a", numel, dt);
        const void* b = c.in("b", numel, dt);
        float* o = (float*)c.out("out", 1, F32);
        float* ws = (float*)c.scratch("ws", 1024 * 4);
        c.go();
        need(tg_dot(a, b, o, ws, numel, dt, nullptr), "tg_dot");
      });
      // loss sums
      for (int acc = 0; acc < 2; ++acc) {
        add(std::string(acc ? "sum_acc." : "sum.") + tag, [=](Ctx& c) {
          const void* x = c.in("x", numel, dt);
          float* o = (float*)(acc ? c.inout("out", 1, F32) : c.out("out", 1, F32));
          c.go();
          need(tg_sum(x, o, numel, 0.5f, acc, dt, nullptr), "tg_sum");
        });
        add(std::string(acc ? "abs_diff_sum_acc." : "abs_diff_sum.") + tag, [=](Ctx& c) {
          const void* a = c.in("a", numel, dt);
          const void* b = c.in("b", numel, dt);
          float* o = (float*)(acc ? c.inout("out", 1, F32) : c.out("out", 1, F32));
          c.go();
          need(tg_abs_diff_sum(a, b, o, numel, 0.5f, acc, dt, nullptr), "tg_abs_diff_sum");
        });
      }
      for (int two = 0; two < 2; ++two)
        add(std::string(two ? "sum_ordered_abs_diff." : "sum_ordered.") + tag, [=](Ctx& c) {
          const void* x = c.in("x", numel, dt);
          const void* y = two ? c.in("y", numel, dt) : nullptr;
          float* o = (float*)c.out("out", 1, F32);
          const size_t rows = two ? 512 : 3;      // fewer rows mean fewer workgroups
          float* ws = (float*)c.scratch("workspace", rows * 4);
          c.go();
          need(tg_sum_ordered(x, y, o, numel, 0.5f, 0, ws, rows, dt, nullptr), "tg_sum_ordered");
        });
      for (int which = 0; which < 3; ++which)
        add(std::string(which == 0 ? "abs_diff_bwd." : which == 1 ? "abs_diff_bwd_ga." : "abs_diff_bwd_gb.") + tag, [=](Ctx& c) {
          const void* a = c.in("a", numel, dt);
          const void* b = c.in("b", numel, dt);
          const float* gs = (const float*)c.in_pos("gscale", 1, F32);
          void* ga = which != 2 ? c.out("ga", numel, dt) : nullptr;
          void* gb = which != 1 ? c.out("gb", numel, dt) : nullptr;
          c.go();
          need(tg_abs_diff_bwd(a, b, gs, ga, gb, numel, 0.5f, dt, nullptr), "tg_abs_diff_bwd");
        });
    }
    // per-pixel / per-channel kernels: npix off the block, c of a vector +- 1 and the scalar path
    struct PC {
      int64_t npix;
      int c;
    };
    for (const PC& s : {PC{35, 7}, PC{35, 9}, PC{4099, 8}, PC{1, 16}, PC{129, 3}}) {
      const std::string tag = dn + "npix" + std::to_string(s.npix) + "_c" + std::to_string(s.c);
      const size_t ne = s.npix * s.c;
      for (int bias = 0; bias < 2; ++bias)
        add(std::string(bias ? "bias_lrelu_fwd." : "bias_lrelu_fwd_nobias.") + tag, [=](Ctx& c) {
          const void* y = c.in("y", ne, dt);
          const float* b = bias ? (const float*)c.in("bias", s.c, F32) : nullptr;
          void* z = c.out("z", ne, dt);
          c.go();
          need(tg_bias_lrelu_fwd(y, b, z, s.npix, s.c, 0.2f, dt, nullptr), "tg_bias_lrelu_fwd");
        });
      for (int acc = 0; acc < 2; ++acc) {
        add(std::string(acc ? "lrelu_bwd_bias_acc." : "lrelu_bwd_bias.") + tag, [=](Ctx& c) {
          const void* gz = c.in("gz", ne, dt);
          const void* z = c.in("z", ne, dt);
          void* gy = c.out("gy", ne, dt);
          float* gb = (float*)(acc ? c.inout("gbias", s.c, F32) : c.out("gbias", s.c, F32));
          c.go();
          need(tg_lrelu_bwd_bias(gz, z, gy, gb, s.npix, s.c, 0.2f, acc, dt, nullptr), "tg_lrelu_bwd_bias");
        });
        add(std::string(acc ? "channel_sum_acc." : "channel_sum.") + tag, [=](Ctx& c) {
          const void* g = c.in("g", ne, dt);
          float* o = (float*)(acc ? c.inout("out", s.c, F32) : c.out("out", s.c, F32));
          c.go();
          need(tg_channel_sum(g, o, s.npix, s.c, acc, dt, nullptr), "tg_channel_sum");
        });
        add(std::string(acc ? "channel_sum_ordered_acc." : "channel_sum_ordered.") + tag, [=](Ctx& c) {
          const void* g = c.in("g", ne, dt);
          float* o = (float*)(acc ? c.inout("out", s.c, F32) : c.out("out", s.c, F32));
          const size_t wsf = (size_t)(acc ? 512 : 5) * s.c;
          float* ws = (float*)c.scratch("workspace", wsf * 4);
          c.go();
          need(tg_channel_sum_ordered(g, o, s.npix, s.c, acc, ws, wsf, dt, nullptr), "tg_channel_sum_ordered");
        });
      }
    }
    // 2x2 resampling: maps off every tile, n = 1 and an odd batch, c of a vector +- 1
    struct R {
      int n, h, w, c;
    };
    for (const R& s : {R{1, 10, 6, 7}, R{3, 6, 10, 9}, R{3, 2, 2, 16}, R{1, 18, 6, 24}}) {
      const std::string tag = dn + "n" + std::to_string(s.n) + "_" + std::to_string(s.h) + "x" + std::to_string(s.w) + "_c" + std::to_string(s.c);
      const size_t nfull = (size_t)s.n * s.h * s.w * s.c, nhalf = nfull / 4;
      add("pool2x2_fwd." + tag, [=](Ctx& c) {
        const void* x = c.in("x", nfull, dt);
        void* y = c.out("y", nhalf, dt);
        c.go();
        need(tg_pool2x2_fwd(x, y, s.n, s.h, s.w, s.c, 0.25f, dt, nullptr), "tg_pool2x2_fwd");
      });
      add("pool2x2_bwd." + tag, [=](Ctx& c) {
        const void* gy = c.in("gy", nhalf, dt);
        void* gx = c.out("gx", nfull, dt);
        c.go();
        need(tg_pool2x2_bwd(gy, gx, s.n, s.h, s.w, s.c, 0.25f, dt, nullptr), "tg_pool2x2_bwd");
      });
      for (int which = 0; which < 3; ++which)      // both incoming gradients with a bias gradient, pooled alone, full alone
        add(std::string(which == 0 ? "lrelu_pool_bwd." : which == 1 ? "lrelu_pool_bwd_pooled." : "lrelu_pool_bwd_full.") + tag, [=](Ctx& c) {
          const void* gz = which != 1 ? c.in("gz", nfull, dt) : nullptr;
          const void* gzp = which != 2 ? c.in("gz_pooled", nhalf, dt) : nullptr;
          const void* z = c.in("z", nfull, dt);
          void* gy = c.out("gy", nfull, dt);
          float* gb = which == 0 ? (float*)c.out("gbias", s.c, F32) : nullptr;
          c.go();
          need(tg_lrelu_pool_bwd(gz, gzp, z, gy, gb, s.n, s.h, s.w, s.c, 0.2f, 0, dt, nullptr), "tg_lrelu_pool_bwd");
        });
      if (dt != TG_F32 && s.c % 8 == 0)
        for (int bias = 0; bias < 2; ++bias)
          add(std::string(bias ? "lrelu_pool_bwd_signs_bias." : "lrelu_pool_bwd_signs.") + tag, [=](Ctx& c) {
            const void* gzp = c.in("gz_pooled", nhalf, dt);
            const void* sg = c.in("z_signs", nfull / 8, U8);
            void* gy = c.out("gy", nfull, dt);
            float* gb = bias ? (float*)c.out("gbias", s.c, F32) : nullptr;
            c.go();
            need(tg_lrelu_pool_bwd_signs(gzp, sg, gy, gb, s.n, s.h, s.w, s.c, 0.2f, 0, dt, nullptr), "tg_lrelu_pool_bwd_signs");
          });
      // upsample + concat: here (h, w) is the LOW resolution
      const int c1 = s.c == 16 ? 0 : s.c + 1;
      const size_t n0 = nfull, nout = nfull * 4 / s.c * (s.c + c1), nskip = nfull * 4 / s.c * c1;
      add("upsample2x_concat_fwd." + tag, [=](Ctx& c) {
        const void* x0 = c.in("x0", n0, dt);
        const void* x1 = c1 ? c.in("x1", nskip, dt) : nullptr;
        void* o = c.out("out", nout, dt);
        c.go();
        need(tg_upsample2x_concat_fwd(x0, x1, o, s.n, s.h, s.w, s.c, c1, 0, 0, dt, nullptr), "tg_upsample2x_concat_fwd");
      });
      add("upsample2x_concat_bwd." + tag, [=](Ctx& c) {
        const void* go = c.in("gout", nout, dt);
        void* g0 = c.out("g0", n0, dt);
        void* g1 = c1 ? c.out("g1", nskip, dt) : nullptr;
        c.go();
        need(tg_upsample2x_concat_bwd(go, g0, g1, s.n, s.h, s.w, s.c, c1, 0, 0, dt, nullptr), "tg_upsample2x_concat_bwd");
      });
    }
    // the grouped read of the skips: 4 output groups of 1 image read 2 skip images
    add("upsample2x_concat_fwd." + dn + "grouped", [=](Ctx& c) {
      const void* x0 = c.in("x0", 4 * 3 * 5 * 8, dt);
      const void* x1 = c.in("x1", 2 * 6 * 10 * 16, dt);
      void* o = c.out("out", 4 * 6 * 10 * 24, dt);
      c.go();
      need(tg_upsample2x_concat_fwd(x0, x1, o, 4, 3, 5, 8, 16, 1, pack_perm({1, 0, 0, 1}), dt, nullptr), "tg_upsample2x_concat_fwd");
    });
    add("upsample2x_concat_bwd." + dn + "grouped", [=](Ctx& c) {
      const void* go = c.in("gout", 4 * 6 * 10 * 24, dt);
      void* g0 = c.out("g0", 4 * 3 * 5 * 8, dt);
      void* g1 = c.out("g1", 2 * 6 * 10 * 16, dt);
      c.go();
      need(tg_upsample2x_concat_bwd(go, g0, g1, 4, 3, 5, 8, 16, 1, pack_perm({1, 0, 0, 1}), dt, nullptr), "tg_upsample2x_concat_bwd");
    });
    // per-sample kernels: batch 1 and 3, per-sample length of a vector +- 1 and a long tail
    for (int batch : {1, 3})
      for (int64_t per : {7, 9, 4099}) {
        const std::string tag = dn + "b" + std::to_string(batch) + "_per" + std::to_string(per);
        const size_t ne = (size_t)batch * per;
        add("sample_lerp." + tag, [=](Ctx& c) {
          const void* x = c.in("x", ne, dt);
          const void* y = c.in("y", ne, dt);
          const float* a = (const float*)c.in_pos("alpha", batch, F32);
          void* o = c.out("out", ne, dt);
          c.go();
          need(tg_sample_lerp(x, y, a, o, batch, per, dt, nullptr), "tg_sample_lerp");
        });
        for (int sc = 0; sc < 2; ++sc)
          add(std::string(sc ? "sample_scale_scalar." : "sample_scale.") + tag, [=](Ctx& c) {
            const void* x = c.in("x", ne, dt);
            const float* coef = (const float*)c.in("coef", batch, F32);
            const float* s1 = sc ? (const float*)c.in_pos("scalar", 1, F32) : nullptr;
            void* o = c.out("out", ne, dt);
            c.go();
            need(tg_sample_scale(x, coef, s1, o, batch, per, dt, nullptr), "tg_sample_scale");
          });
        add("sample_sumsq." + tag, [=](Ctx& c) {
          const void* x = c.in("x", ne, dt);
          float* o = (float*)c.out("out", batch, F32);
          c.go();
          need(tg_sample_sumsq(x, o, batch, per, dt, nullptr), "tg_sample_sumsq");
        });
      }
    // gdrop: [n, hw, c], c padded past the logical count
    for (int dev = 0; dev < 2; ++dev)
      add(std::string(dev ? "gdrop_dev." : "gdrop.") + dn + "n3_hw15_c16", [=](Ctx& c) {
        const void* x = c.in("x", 3 * 15 * 16, dt);
        const float* nz = (const float*)c.in("noise", 3 * 16, F32);
        const float* st = dev ? (const float*)c.in_pos("strength", 1, F32) : nullptr;
        void* o = c.out("out", 3 * 15 * 16, dt);
        c.go();
        need(tg_gdrop(x, nz, st, 0.3f, 9, o, 3, 15, 16, dt, nullptr), "tg_gdrop");
      });
    // minibatch stddev: hw 16, c off the vector, groups of 1 and 3
    for (int groups : {1, 3}) {
      const int n = 6, hw = 16, cc = 9, cpad = 16;
      const std::string tag = dn + "n6_g" + std::to_string(groups) + "_c9_16";
      const size_t nx = (size_t)n * hw * cc, no = (size_t)n * hw * cpad;
      add("mbstd_fwd." + tag, [=](Ctx& c) {
        const void* x = c.in("x", nx, dt);
        void* o = c.out("out", no, dt);
        float* st = groups == 3 ? (float*)c.out("stat", groups, F32) : nullptr;
        c.go();
        need(tg_mbstd_fwd(x, o, st, n, groups, hw, cc, cpad, 1e-8f, dt, nullptr), "tg_mbstd_fwd");
      });
      add("mbstd_bwd." + tag, [=](Ctx& c) {
        const void* go = c.in("gout", no, dt);
        const void* x = c.in("x", nx, dt);
        void* gx = c.out("gx", nx, dt);
        c.go();
        need(tg_mbstd_bwd(go, x, gx, n, groups, hw, cc, cpad, 1e-8f, dt, nullptr), "tg_mbstd_bwd");
      });
      add("mbstd_bwd_bwd." + tag, [=](Ctx& c) {
        const void* v = c.in("v", nx, dt);
        const void* go = c.in("gout", no, dt);
        const void* x = c.in("x", nx, dt);
        void* ggo = c.out("ggout", no, dt);
        void* gx2 = c.out("gx2", nx, dt);
        c.go();
        need(tg_mbstd_bwd_bwd(v, go, x, ggo, gx2, n, groups, hw, cc, cpad, 1e-8f, dt, nullptr), "tg_mbstd_bwd_bwd");
      });
    }
    // fully connected tail: m = 1 and an odd batch, k off the vector
    struct FC {
      int m, n, k;
    };
    for (const FC& s : {FC{1, 1, 7}, FC{3, 1, 4099}, FC{5, 3, 33}}) {
      const std::string tag = dn + "m" + std::to_string(s.m) + "_n" + std::to_string(s.n) + "_k" + std::to_string(s.k);
      add("fc_fwd." + tag, [=](Ctx& c) {
        const void* x = c.in("x", (size_t)s.m * s.k, dt);
        const float* w = (const float*)c.in("w", (size_t)s.k * s.n, F32);
        const float* b = (const float*)c.in("bias", s.n, F32);
        float* y = (float*)c.out("y", (size_t)s.m * s.n, F32);
        c.go();
        need(tg_fc_fwd(x, w, b, y, s.m, s.n, s.k, dt, nullptr), "tg_fc_fwd");
      });
      for (int acc = 0; acc < 2; ++acc)
        add(std::string(acc ? "fc_bwd_acc." : "fc_bwd.") + tag, [=](Ctx& c) {
          const void* x = c.in("x", (size_t)s.m * s.k, dt);
          const float* w = (const float*)c.in("w", (size_t)s.k * s.n, F32);
          const float* g = (const float*)c.in("g", (size_t)s.m * s.n, F32);
          void* gx = c.out("gx", (size_t)s.m * s.k, dt);
          float* gw = (float*)(acc ? c.inout("gw", (size_t)s.k * s.n, F32) : c.out("gw", (size_t)s.k * s.n, F32));
          float* gb = (float*)(acc ? c.inout("gb", s.n, F32) : c.out("gb", s.n, F32));
          c.go();
          need(tg_fc_bwd(x, w, g, gx, gw, gb, s.m, s.n, s.k, acc, acc, dt, nullptr), "tg_fc_bwd");
        });
    }
  }
}


// ---------------------------------------------------------------------------------------- attention: GEMM, softmax, flash
void register_attention_cases() {
  struct G {
    int batch, m, n, k, ta, tb;
  };
  // m / n / k off the 32-wide MFMA tile and on it, batch 1 and 3, every transpose form
  for (const G& g : {G{1, 33, 31, 17, 0, 0}, G{3, 32, 64, 16, 0, 1}, G{2, 5, 40, 33, 1, 0}, G{1, 64, 8, 72, 1, 1}})
    for (int dt : {TG_F32, TG_BF16})
      for (int cf32 = 0; cf32 < (dt == TG_BF16 ? 2 : 1); ++cf32)
        for (int acc = 0; acc < 2; ++acc) {
          char tag[120];
          snprintf(tag, sizeof tag, "%s.b%d_m%d_n%d_k%d_t%d%d%s%s", dname(dt), g.batch, g.m, g.n, g.k, g.ta, g.tb, cf32 ? "_cf32" : "", acc ? "_acc" : "");
          add(std::string("batched_gemm.") + tag, [=](Ctx& c) {
            const int lda = g.ta ? g.m : g.k, ldb = g.tb ? g.k : g.n, ldc = g.n;
            const int64_t sa = (int64_t)g.m * g.k, sb = (int64_t)g.k * g.n, sc = (int64_t)g.m * g.n;
            const void* a = c.in("a", g.batch * sa, dt);
            const void* b = c.in("b", g.batch * sb, dt);
            const int ck = dt == TG_F32 || cf32 ? F32 : dt;
            void* o = acc ? c.inout("c", g.batch * sc, ck) : c.out("c", g.batch * sc, ck);
            c.go();
            need(tg_batched_gemm(a, b, o, g.batch, g.m, g.n, g.k, g.ta, g.tb, lda, ldb, ldc, sa, sb, sc, 0.5f, acc, dt, cf32, nullptr), "tg_batched_gemm");
          });
        }
  for (const G& g : {G{1, 3, 5, 7, 0, 0}, G{1, 17, 1, 33, 1, 0}, G{1, 4, 9, 130, 0, 1}, G{1, 33, 3, 2, 1, 1}})
    for (int acc = 0; acc < 2; ++acc) {
      char tag[120];
      snprintf(tag, sizeof tag, "m%d_n%d_k%d_t%d%d%s", g.m, g.n, g.k, g.ta, g.tb, acc ? "_acc" : "");
      add(std::string("small_gemm.") + tag, [=](Ctx& c) {
        const float* a = (const float*)c.in("a", (size_t)g.m * g.k, F32);
        const float* b = (const float*)c.in("b", (size_t)g.k * g.n, F32);
        const float* bias = acc ? nullptr : (const float*)c.in("bias", g.n, F32);
        float* o = (float*)(acc ? c.inout("c", (size_t)g.m * g.n, F32) : c.out("c", (size_t)g.m * g.n, F32));
        c.go();
        need(tg_small_gemm(a, b, bias, o, g.m, g.n, g.k, g.ta, g.tb, acc, nullptr), "tg_small_gemm");
      });
    }
  struct RC {
    int64_t rows;
    int cols;
  };
  for (const RC& s : {RC{1, 1}, RC{3, 63}, RC{5, 65}, RC{2, 256}, RC{3, 1025}})
    for (int dt : {TG_F32, TG_BF16, TG_F16}) {
      const std::string tag = std::string(dname(dt)) + ".rows" + std::to_string(s.rows) + "_cols" + std::to_string(s.cols);
      const size_t ne = s.rows * s.cols;
      add("softmax_rows_fwd." + tag, [=](Ctx& c) {
        const void* x = c.in("s", ne, dt);
        void* p = c.out("p", ne, dt);
        c.go();
        need(tg_softmax_rows_fwd(x, p, s.rows, s.cols, dt, nullptr), "tg_softmax_rows_fwd");
      });
      add("softmax_rows_bwd." + tag, [=](Ctx& c) {
        const void* p = c.in_pos("p", ne, dt);
        const void* dp = c.in("dp", ne, dt);
        void* ds = c.out("ds", ne, dt);
        c.go();
        need(tg_softmax_rows_bwd(p, dp, ds, s.rows, s.cols, dt, nullptr), "tg_softmax_rows_bwd");
      });
      add("softmax_rows_bwd_bwd." + tag, [=](Ctx& c) {
        const void* p = c.in_pos("p", ne, dt);
        const void* dp = c.in("dp", ne, dt);
        const void* v = c.in("v", ne, dt);
        void* gp = c.out("gp", ne, dt);
        c.go();
        need(tg_softmax_rows_bwd_bwd(p, dp, v, gp, s.rows, s.cols, dt, nullptr), "tg_softmax_rows_bwd_bwd");
      });
    }
  for (const G& g : {G{1, 7, 9}, G{3, 33, 16}, G{2, 128, 8}, G{1, 1, 5}})
    add("transpose16.b" + std::to_string(g.batch) + "_" + std::to_string(g.m) + "x" + std::to_string(g.n), [=](Ctx& c) {
      const void* x = c.in("src", (size_t)g.batch * g.m * g.n, BF16);
      void* o = c.out("dst", (size_t)g.batch * g.m * g.n, BF16);
      c.go();
      need(tg_transpose16(x, o, g.batch, g.m, g.n, nullptr), "tg_transpose16");
    });
  // flash attention: the smallest members of the element-wise tests' (n, len, dk, dv) sets: one and two key tiles, n = 1 and 3
  struct F {
    int n, len, dk, dv;
  };
  for (const F& f : {F{1, 128, 8, 64}, F{3, 256, 16, 64}, F{1, 256, 16, 128}, F{2, 128, 16, 256}, F{1, 128, 8, 128}})
    for (int dt : {TG_BF16, TG_F16}) {
      if (dt == TG_F16 && f.len != 128) continue;
      char tg[80];
      snprintf(tg, sizeof tg, "%s.n%d_len%d_dk%d_dv%d", dname(dt), f.n, f.len, f.dk, f.dv);
      const std::string tag = tg;
      const size_t nq = (size_t)f.n * f.len * f.dk, nv = (size_t)f.n * f.len * f.dv, nl = (size_t)f.n * f.len;
      add("flash_fwd." + tag, [=](Ctx& c) {
        const void* q = c.in("q", nq, dt);
        const void* k = c.in("k", nq, dt);
        const void* v = c.in("v", nv, dt);
        void* o = c.out("o", nv, dt);
        float* lse = (float*)c.out("lse", nl, F32);
        void* ws = c.scratch("workspace", (size_t)tg_flash_attention_workspace_bytes(f.n, f.len, f.dk, f.dv, 0));
        c.go();
        need(tg_flash_attention_fwd(q, k, v, o, lse, ws, f.n, f.len, f.dk, f.dv, dt, nullptr), "tg_flash_attention_fwd");
      });
      if (f.dv > 128) continue;
      for (int second = 0; second < 2; ++second)
        add(std::string(second ? "flash_bwd_bwd." : "flash_bwd.") + tag, [=](Ctx& c) {
          const void* q = c.in("q", nq, dt);
          const void* k = c.in("k", nq, dt);
          const void* v = c.in("v", nv, dt);
          const void* d_o = c.in("d_o", nv, dt);
          void* o = c.in("o", nv, dt);
          float* lse = (float*)c.in("lse", nl, F32);
          void* ws0 = malloc((size_t)tg_flash_attention_workspace_bytes(f.n, f.len, f.dk, f.dv, 0));
          const int rc0 = tg_flash_attention_fwd(q, k, v, o, lse, ws0, f.n, f.len, f.dk, f.dv, dt, nullptr);      // a consistent (o, lse)
          free(ws0);
          need(rc0, "tg_flash_attention_fwd (preparing)");
          void* ws = c.scratch("workspace", (size_t)tg_flash_attention_workspace_bytes(f.n, f.len, f.dk, f.dv, second ? 2 : 1));
          if (!second) {
            void* dq = c.out("dq", nq, dt);
            void* dk = c.out("dk_out", nq, dt);
            void* dv = c.out("dv_out", nv, dt);
            c.go();
            need(tg_flash_attention_bwd(q, k, v, d_o, o, lse, ws, dq, dk, dv, f.n, f.len, f.dk, f.dv, dt, nullptr), "tg_flash_attention_bwd");
          } else {
            const void* aq = c.in("a_q", nq, dt);
            const void* ak = c.in("a_k", nq, dt);
            const void* av = c.in("a_v", nv, dt);
            void* jq = c.out("adj_q", nq, dt);
            void* jk = c.out("adj_k", nq, dt);
            void* jv = c.out("adj_v", nv, dt);
            void* jd = c.out("adj_do", nv, dt);
            c.go();
            need(tg_flash_attention_bwd_bwd(q, k, v, d_o, o, lse, aq, ak, av, ws, jq, jk, jv, jd, f.n, f.len, f.dk, f.dv, dt, nullptr),
                 "tg_flash_attention_bwd_bwd");
          }
        });
    }
}

// ------------------------------------------------------------------------------------------ loss tail, rows, random, Adam
void register_loss_cases() {
  for (int n : {1, 7, 257})
    for (int mode = 0; mode < 4; ++mode) {
      const std::string tag = "n" + std::to_string(n) + "_mode" + std::to_string(mode);
      for (int acc = 0; acc < 2; ++acc)
        add(std::string(acc ? "pred_loss_fwd_acc." : "pred_loss_fwd.") + tag, [=](Ctx& c) {
          const float* x = (const float*)c.in("x", n, F32);
          float* o = (float*)(acc ? c.inout("out", 1, F32) : c.out("out", 1, F32));
          c.go();
          need(tg_pred_loss_fwd(x, o, n, mode, 1.f, -1.f, 0.5f, acc, nullptr), "tg_pred_loss_fwd");
        });
      for (int gs = 0; gs < 2; ++gs)
        add(std::string(gs ? "pred_loss_bwd_gscale." : "pred_loss_bwd.") + tag, [=](Ctx& c) {
          const float* x = (const float*)c.in("x", n, F32);
          const float* g = gs ? (const float*)c.in_pos("gscale", 1, F32) : nullptr;
          float* gx = (float*)c.out("gx", n, F32);
          c.go();
          need(tg_pred_loss_bwd(x, g, gx, n, mode, 1.f, -1.f, 0.5f, nullptr), "tg_pred_loss_bwd");
        });
    }
  // the batched tail: 3 groups of 5, 12 jobs over 8 terms (the limits), and one group of one
  for (int big = 0; big < 2; ++big) {
    const int gsz = big ? 5 : 1, groups = big ? 3 : 1, njobs = big ? 12 : 1, nterms = big ? 8 : 1;
    auto jobs = [=]() {
      std::vector<TgPredJob> j(njobs);
      for (int i = 0; i < njobs; ++i) j[i] = TgPredJob{i % groups, i % nterms, i % 4, 1.f, -1.f, 0.5f};
      return j;
    };
    add(std::string("pred_losses_fwd.") + (big ? "limits" : "one"), [=](Ctx& c) {
      const float* pred = (const float*)c.in("pred", gsz * groups, F32);
      float* terms = (float*)c.out("terms", nterms, F32);
      const std::vector<TgPredJob> j = jobs();
      c.go();
      need(tg_pred_losses_fwd(pred, gsz, groups, j.data(), njobs, terms, nterms, nullptr), "tg_pred_losses_fwd");
    });
    add(std::string("pred_losses_bwd.") + (big ? "limits" : "one"), [=](Ctx& c) {
      const float* pred = (const float*)c.in("pred", gsz * groups, F32);
      std::vector<const float*> gt(nterms);
      for (int t = 0; t < nterms; ++t) gt[t] = big && t == 3 ? nullptr : (const float*)c.in_pos("gterm", 1, F32);
      float* gp = (float*)c.out("gpred", gsz * groups, F32);
      const std::vector<TgPredJob> j = jobs();
      c.go();
      need(tg_pred_losses_bwd(pred, gsz, groups, j.data(), njobs, gt.data(), nterms, gp, nullptr), "tg_pred_losses_bwd");
    });
  }
  for (int n : {1, 24})
    add("sum_scalars.n" + std::to_string(n), [=](Ctx& c) {
      std::vector<const float*> sc(n);
      for (int i = 0; i < n; ++i) sc[i] = (const float*)c.in("scalar", 1, F32);
      float* o = (float*)c.out("out", 1, F32);
      c.go();
      need(tg_sum_scalars(sc.data(), n, o, nullptr), "tg_sum_scalars");
    });
  for (int batch : {1, 3, 65}) {
    const std::string tag = "b" + std::to_string(batch);
    add("var_from_sums." + tag, [=](Ctx& c) {
      const float* sum = (const float*)c.in("sum", 1, F32);
      const float* ss = (const float*)c.in_const("sample_sumsq", batch, F32, 64.f);
      float* o = (float*)c.out("out", 1, F32);
      c.go();
      need(tg_var_from_sums(sum, ss, o, batch, (int64_t)batch * 48, nullptr), "tg_var_from_sums");
    });
    add("gp_penalty." + tag, [=](Ctx& c) {
      const float* ss = (const float*)c.in_pos("sumsq", batch, F32);
      float* loss = (float*)c.out("loss", 1, F32);
      float* coef = (float*)c.out("coef", batch, F32);
      c.go();
      need(tg_gp_penalty(ss, loss, coef, batch, 10.f, nullptr), "tg_gp_penalty");
    });
    for (int dim : {1, 7, 257}) {
      const std::string t2 = tag + "_dim" + std::to_string(dim);
      add("cosine_distance_fwd." + t2, [=](Ctx& c) {
        const float* e = (const float*)c.in_pos("expected", (size_t)batch * dim, F32);
        const float* m = (const float*)c.in_pos("embedding", (size_t)batch * dim, F32);
        float* o = (float*)c.out("out", 1, F32);
        c.go();
        need(tg_cosine_distance_fwd(e, m, o, batch, dim, 0.5f, nullptr), "tg_cosine_distance_fwd");
      });
      add("cosine_distance_bwd." + t2, [=](Ctx& c) {
        const float* e = (const float*)c.in_pos("expected", (size_t)batch * dim, F32);
        const float* m = (const float*)c.in_pos("embedding", (size_t)batch * dim, F32);
        const float* g = (const float*)c.in_pos("gscale", 1, F32);
        float* o = (float*)c.out("g_embedding", (size_t)batch * dim, F32);
        c.go();
        need(tg_cosine_distance_bwd(e, m, g, o, batch, dim, 0.5f, nullptr), "tg_cosine_distance_bwd");
      });
    }
  }
  // rows: 8 jobs (the limit) of 0..4 sources, numel off the vector, jobs laid end to end so that dst is fully written
  for (int dt : {TG_F32, TG_BF16, TG_F16})
    for (int njobs : {1, 8})
      add(std::string("rows_assemble.") + dname(dt) + ".jobs" + std::to_string(njobs), [=](Ctx& c) {
        const int64_t numels[8] = {4099, 7, 9, 1, 33, 8, 127, 4};
        std::vector<TgRowsJob> jobs(njobs);
        int64_t off = 0;
        for (int j = 0; j < njobs; ++j) {
          memset(&jobs[j], 0, sizeof(TgRowsJob));
          for (int q = 0; q < (njobs == 1 ? 1 : j % 5); ++q) jobs[j].src[q] = c.in("src", numels[j], dt);
          jobs[j].dst_off = off, jobs[j].numel = numels[j];
          off += numels[j];
        }
        void* dst = c.out("dst", off, dt);
        c.go();
        need(tg_rows_assemble(jobs.data(), njobs, dst, dt, nullptr), "tg_rows_assemble");
      });
  for (int64_t n : {(int64_t)1, (int64_t)7, (int64_t)4099})
    add("uniform.n" + std::to_string(n), [=](Ctx& c) {
      float* o = (float*)c.out("out", n, F32);
      uint32_t* st = (uint32_t*)c.in_const("state", 2, I32, 0.f, INOUT);
      c.go();
      need(tg_uniform(o, n, 1234567ull, st, -1.f, 1.f, nullptr), "tg_uniform");
    });
}

TgLossScaleState* loss_state(Ctx& c, Role role, int found, int skip) {
  if (tg_loss_scale_state_bytes() != sizeof(TgLossScaleState)) throw Fail{"tg_loss_scale_state_bytes != sizeof(TgLossScaleState)"};
  TgLossScaleState s;
  memset(&s, 0, sizeof s);
  s.scale = 128.f, s.seed = 128.f, s.inv_scale = 1.f / 128.f, s.found = found, s.skip = skip;
  return (TgLossScaleState*)c.in_bytes("state", &s, sizeof s, role);
}

void register_optimiser_cases() {
  // numel of a 16-byte vector - 1 / + 1, one element, a tail after many vectors; theta / m / v / avg are in/out state
  for (int64_t numel : {(int64_t)1, (int64_t)3, (int64_t)5, (int64_t)4099}) {
    const std::string tag = "numel" + std::to_string(numel);
    for (int variant = 0; variant < 3; ++variant)      // host rate, device rate, device rate + bf16 shadow
      add(std::string(variant == 0 ? "adam_step." : variant == 1 ? "adam_step_dev_rate." : "adam_step_shadow.") + tag, [=](Ctx& c) {
        float* th = (float*)c.inout("theta", numel, F32);
        const float* g = (const float*)c.in("grad", numel, F32);
        float* m = (float*)c.inout("m", numel, F32);
        float* v = (float*)c.in_pos("v", numel, F32, INOUT);
        const float* lr = variant ? (const float*)c.in_const("lr_t", 1, F32, 1e-3f) : nullptr;
        void* sh = variant == 2 ? c.out("theta_bf16", numel, BF16) : nullptr;
        c.go();
        need(tg_adam_step(th, g, m, v, sh, numel, 1e-3f, lr, 0.5f, 0.99f, 1e-8f, 0.5f, nullptr), "tg_adam_step");
      });
    add("adam_ema_step." + tag, [=](Ctx& c) {
      float* th = (float*)c.inout("theta", numel, F32);
      const float* g = (const float*)c.in("grad", numel, F32);
      float* m = (float*)c.inout("m", numel, F32);
      float* v = (float*)c.in_pos("v", numel, F32, INOUT);
      float* avg = (float*)c.inout("avg", numel, F32);
      const float* lr = (const float*)c.in_const("lr_t", 1, F32, 1e-3f);
      const float* w = (const float*)c.in_const("w", 1, F32, 0.125f);
      c.go();
      need(tg_adam_ema_step(th, g, m, v, avg, numel, lr, 0.5f, 0.99f, 1e-8f, 0.5f, w, nullptr), "tg_adam_ema_step");
    });
    add("ema_update." + tag, [=](Ctx& c) {
      float* avg = (float*)c.inout("avg", numel, F32);
      const float* var = (const float*)c.in("var", numel, F32);
      const float* w = (const float*)c.in_const("w", 1, F32, 0.125f);
      c.go();
      need(tg_ema_update(avg, var, numel, w, nullptr), "tg_ema_update");
    });
    for (int skip = 0; skip < 2; ++skip) {
      add(std::string(skip ? "adam_step_guarded_skip." : "adam_step_guarded.") + tag, [=](Ctx& c) {
        float* th = (float*)c.inout("theta", numel, F32);
        const float* g = (const float*)c.in("grad", numel, F32);
        float* m = (float*)c.inout("m", numel, F32);
        float* v = (float*)c.in_pos("v", numel, F32, INOUT);
        const float* lr = (const float*)c.in_const("lr_t", 1, F32, 1e-3f);
        const TgLossScaleState* st = loss_state(c, IN, 0, skip);
        c.go();
        need(tg_adam_step_guarded(th, g, m, v, numel, lr, 0.5f, 0.99f, 1e-8f, st, nullptr), "tg_adam_step_guarded");
      });
      add(std::string(skip ? "adam_ema_step_guarded_skip." : "adam_ema_step_guarded.") + tag, [=](Ctx& c) {
        float* th = (float*)c.inout("theta", numel, F32);
        const float* g = (const float*)c.in("grad", numel, F32);
        float* m = (float*)c.inout("m", numel, F32);
        float* v = (float*)c.in_pos("v", numel, F32, INOUT);
        float* avg = (float*)c.inout("avg", numel, F32);
        const float* lr = (const float*)c.in_const("lr_t", 1, F32, 1e-3f);
        const float* w = (const float*)c.in_const("w", 1, F32, 0.125f);
        const TgLossScaleState* st = loss_state(c, IN, 0, skip);
        c.go();
        need(tg_adam_ema_step_guarded(th, g, m, v, avg, numel, lr, 0.5f, 0.99f, 1e-8f, st, w, nullptr), "tg_adam_ema_step_guarded");
      });
    }
    add("nonfinite_check." + tag, [=](Ctx& c) {
      const float* x = (const float*)c.in("x", numel, F32);
      TgLossScaleState* st = loss_state(c, INOUT, 0, 0);
      c.go();
      need(tg_nonfinite_check(x, numel, st, nullptr), "tg_nonfinite_check");
    });
  }
  add("nonfinite_check.sweep_plus_tail", [=](Ctx& c) {      // one full sweep of the capped grid and a tail
    const int64_t numel = 4194304 + 5;
    const float* x = (const float*)c.in_const("x", numel, F32, 1.f);
    TgLossScaleState* st = loss_state(c, INOUT, 0, 0);
    c.go();
    need(tg_nonfinite_check(x, numel, st, nullptr), "tg_nonfinite_check");
  });
  add("adam_tick", [=](Ctx& c) {
    int64_t* step = (int64_t*)c.in_const("step", 1, I64, 3.f, INOUT);
    float* lr = (float*)c.out("lr_t", 1, F32);
    c.go();
    need(tg_adam_tick(step, lr, 1e-3f, 0.5f, 0.99f, nullptr), "tg_adam_tick");
  });
  for (int found = 0; found < 2; ++found)
    add(std::string(found ? "loss_scale_tick.found" : "loss_scale_tick.clean"), [=](Ctx& c) {
      TgLossScaleState* st = loss_state(c, INOUT, found, 0);
      int64_t* step = (int64_t*)c.in_const("step", 1, I64, 3.f, INOUT);
      float* lr = (float*)c.in_const("lr_t", 1, F32, 1e-3f, INOUT);
      c.go();
      need(tg_loss_scale_tick(st, step, lr, 1e-3f, 0.5f, 0.99f, 1, 65536.f, 1, nullptr), "tg_loss_scale_tick");
    });
  // the multi-tensor moving average: 1-element, off-vector and multi-block jobs next to each other
  add("ema_update_multi", [=](Ctx& c) {
    const int64_t numels[] = {1, 4099, 3, 5, 70001, 7};
    const int njobs = 6;
    std::vector<unsigned char> host(tg_ema_table_bytes(njobs));
    int32_t blocks = 0;
    for (int j = 0; j < njobs; ++j) {
      float* avg = (float*)c.inout("avg", numels[j], F32);
      const float* var = (const float*)c.in("var", numels[j], F32);
      need(tg_ema_table_fill(avg, var, numels[j], j, host.data(), &blocks), "tg_ema_table_fill");
    }
    const void* table = c.in_bytes("table", host.data(), host.size());
    const float* w = (const float*)c.in_const("w", 1, F32, 0.125f);
    c.go();
    need(tg_ema_update_multi(table, njobs, blocks, w, nullptr), "tg_ema_update_multi");
  });
}

// ---------------------------------------------------------------------------------------------------- spectral norm
struct SnShape {
  int kh, kw, cin, cout;
};
const SnShape SN_SHAPES[] = {{1, 1, 1, 1}, {1, 1, 1, 5}, {1, 1, 5, 1}, {1, 1, 2, 64}, {1, 1, 15, 65}, {1, 1, 17, 63}, {4, 4, 16, 1}, {1, 1, 4096, 1},
                             {3, 3, 7, 129}, {3, 3, 8, 257}, {1, 1, 64, 300}, {3, 3, 16, 512}, {1, 1, 16, 1023}, {1, 1, 33, 1024}, {1, 1, 1025, 3},
                             {3, 3, 16, 32}, {1, 1, 3, 16}, {4, 4, 64, 64}, {3, 3, 264, 256}, {3, 3, 5, 7}};
// the 33 jobs of tests/test_gpu_ops.py SN_MULTI_SHAPES: 1-block and many-block jobs adjacent
const int SN_MULTI[33] = {11, 0, 13, 2, 19, 7, 12, 1, 9, 16, 3, 14, 8, 17, 4, 10, 5, 15, 6, 18, 0, 12, 2, 13, 1, 11, 7, 9, 3, 14, 16, 4, 19};

void register_sn_cases() {
  for (const SnShape& s : SN_SHAPES) {
    const int k_rows = s.kh * s.kw * s.cin, cout = s.cout;
    if ((size_t)k_rows * cout > 200000) continue;      // (3,3,264,256): the multi table below carries it
    const std::string tag = std::to_string(k_rows) + "x" + std::to_string(cout);
    const size_t nw = (size_t)k_rows * cout;
    add("spectral_norm_fwd." + tag, [=](Ctx& c) {
      const float* w = (const float*)c.in("w", nw, F32);
      const float* u = (const float*)c.in_pos("u", cout, F32);
      float* wb = (float*)c.out("w_bar", nw, F32);
      float* un = (float*)c.out("u_new", cout, F32);
      float* v = (float*)c.out("v", k_rows, F32);
      float* st = (float*)c.out("stats", 2, F32);
      const size_t wsb = tg_spectral_norm_workspace(k_rows, cout);
      void* ws = c.scratch("ws", wsb);
      ((float*)w)[0] = 1.f;      // never the zero matrix
      c.go();
      need(tg_spectral_norm_fwd(w, u, wb, un, v, st, k_rows, cout, ws, wsb, nullptr), "tg_spectral_norm_fwd");
    });
    for (int acc = 0; acc < 2; ++acc)
      add(std::string(acc ? "spectral_norm_bwd_acc." : "spectral_norm_bwd.") + tag, [=](Ctx& c) {
        const float* g = (const float*)c.in("g_wbar", nw, F32);
        const float* w = (const float*)c.in("w", nw, F32);
        const float* u = (const float*)c.in_pos("u", cout, F32);
        float* un = (float*)c.in("u_new", cout, F32);
        float* v = (float*)c.in("v", k_rows, F32);
        float* st = (float*)c.in("stats", 2, F32);
        float* wb = (float*)malloc(nw * 4);
        const size_t wsb = tg_spectral_norm_workspace(k_rows, cout);
        void* ws = c.scratch("ws", wsb);
        ((float*)w)[0] = 1.f;
        const int rc0 = tg_spectral_norm_fwd(w, u, wb, un, v, st, k_rows, cout, ws, wsb, nullptr);      // consistent u_new, v, stats
        free(wb);
        need(rc0, "tg_spectral_norm_fwd (preparing)");
        float* gw = (float*)(acc ? c.inout("gw", nw, F32) : c.out("gw", nw, F32));
        c.go();
        need(tg_spectral_norm_bwd(g, w, u, un, v, st, gw, acc, k_rows, cout, ws, wsb, nullptr), "tg_spectral_norm_bwd");
      });
  }
  for (int assign = 0; assign < 2; ++assign)
    add(assign ? "sn_assign_u.33_jobs" : "spectral_norm_fwd_multi.33_jobs", [=](Ctx& c) {
      const int njobs = 33;
      std::vector<unsigned char> host(tg_sn_table_bytes(njobs));
      int32_t totals[3] = {0, 0, 0};
      for (int j = 0; j < njobs; ++j) {
        const SnShape& s = SN_SHAPES[SN_MULTI[j]];
        const int k_rows = s.kh * s.kw * s.cin, cout = s.cout;
        const size_t nw = (size_t)k_rows * cout;
        float* w = (float*)c.in("w", nw, F32);
        w[0] = 1.f;
        // sn_assign_u writes u from u_new: there u is in/out and u_new an input
        float* u = (float*)c.in_pos("u", cout, F32, assign ? INOUT : IN);
        float* wb = (float*)(assign ? c.inout("w_bar", nw, F32) : c.out("w_bar", nw, F32));
        float* un = (float*)(assign ? c.in("u_new", cout, F32) : c.out("u_new", cout, F32));
        float* v = (float*)(assign ? c.inout("v", k_rows, F32) : c.out("v", k_rows, F32));
        float* st = (float*)(assign ? c.inout("stats", 2, F32) : c.out("stats", 2, F32));
        const size_t wsb = tg_spectral_norm_workspace(k_rows, cout);
        void* ws = c.scratch("ws", wsb);
        need(tg_sn_table_fill(j, w, u, wb, un, v, st, ws, wsb, k_rows, cout, host.data(), totals), "tg_sn_table_fill");
      }
      const void* table = c.in_bytes("table", host.data(), host.size());
      c.go();
      if (assign) need(tg_sn_assign_u(table, njobs, nullptr), "tg_sn_assign_u");
      else need(tg_spectral_norm_fwd_multi(table, njobs, totals[0], totals[1], totals[2], nullptr), "tg_spectral_norm_fwd_multi");
    });
}


// ------------------------------------------------------------------------------------- preprocessing, MS-SSIM, SWD
void register_data_cases() {
  // three decoded images of different odd sizes (one smaller than the output), pad / crop / reshape rectangles, flips
  for (int dt : {TG_F32, TG_BF16, TG_F16})
    for (int crop = 0; crop < 2; ++crop)
      for (int n : {1, 3})
        add(std::string(crop ? "preprocess_images_crop." : "preprocess_images.") + dname(dt) + ".n" + std::to_string(n), [=](Ctx& c) {
          const int hw = 16, mid = 19;
          const int hs[3] = {9, 33, 21}, ws[3] = {23, 17, 5};
          std::vector<int64_t> off(n);
          std::vector<int32_t> rect(n * 6), cr(n * 4);
          std::vector<float> aug(n * 4);
          int64_t total = 0;
          for (int i = 0; i < n; ++i) {
            const int h = hs[i], w = ws[i], mx = h > w ? h : w, mn = h < w ? h : w;
            off[i] = total;
            total += (int64_t)h * w * 3;
            int32_t* r = &rect[i * 6];
            r[0] = h, r[1] = w;
            if (i == 0) r[2] = -((mx - h) / 2), r[3] = -((mx - w) / 2), r[4] = mx, r[5] = mx;       // PAD
            else if (i == 1) r[2] = (h - mn) / 2, r[3] = (w - mn) / 2, r[4] = mn, r[5] = mn;         // CROP
            else r[2] = 0, r[3] = 0, r[4] = h, r[5] = w;                                           // RESHAPE
            aug[i * 4] = (float)(i & 1), aug[i * 4 + 1] = (float)((i >> 1) & 1), aug[i * 4 + 2] = 0.125f, aug[i * 4 + 3] = 1.25f;
            cr[i * 4] = i, cr[i * 4 + 1] = 3 - i, cr[i * 4 + 2] = mid - 3, cr[i * 4 + 3] = mid - 3 - i;
          }
          const void* packed = c.in("packed", total, U8);
          const int64_t* offs = (const int64_t*)c.in_bytes("offsets", off.data(), n * 8);
          const int* rc = (const int*)c.in_bytes("rect", rect.data(), n * 24);
          const float* au = (const float*)c.in_bytes("aug", aug.data(), n * 16);
          const int* crp = crop ? (const int*)c.in_bytes("crop", cr.data(), n * 16) : nullptr;
          void* o = c.out("out", (size_t)n * hw * hw * 3, dt);
          c.go();
          if (crop) need(tg_preprocess_images_crop(packed, offs, rc, crp, au, o, n, hw, mid, 1, dt, nullptr), "tg_preprocess_images_crop");
          else need(tg_preprocess_images(packed, offs, rc, au, o, n, hw, dt, nullptr), "tg_preprocess_images");
        });
  struct M {
    int n, h, w, ch, levels;
  };
  // the smallest shapes of tests/msssim_np.py CASES, the non-square one, one channel, three levels, n = 1; 64x64 is multi-tile
  for (const M& m : {M{3, 16, 16, 3, 5}, M{1, 32, 48, 3, 5}, M{3, 64, 64, 1, 5}, M{3, 24, 40, 3, 3}, M{2, 32, 32, 4, 5}})
    for (int dt : {TG_F32, TG_BF16, TG_F16}) {
      char tag[80];
      snprintf(tag, sizeof tag, "%s.n%d_%dx%d_c%d_l%d", dname(dt), m.n, m.h, m.w, m.ch, m.levels);
      add(std::string("msssim.") + tag, [=](Ctx& c) {
        const size_t ne = (size_t)m.n * m.h * m.w * m.ch;
        const void* a = c.in_pos("img1", ne, dt);
        const void* b = c.in_pos("img2", ne, dt);
        float* score = (float*)c.out("score", m.n, F32);
        float* ssim = (float*)c.out("ssim", (size_t)m.levels * m.n, F32);
        float* cs = (float*)c.out("cs", (size_t)m.levels * m.n, F32);
        float* mean = (float*)c.out("mean", 1, F32);
        const size_t wsb = tg_msssim_workspace_bytes(m.n, m.h, m.w, m.ch, m.levels);
        if (!wsb) throw Fail{"tg_msssim_workspace_bytes: 0"};
        void* ws = c.scratch("ws", wsb);
        const float wts[3] = {0.2f, 0.3f, 0.5f};
        c.go();
        need(tg_msssim(a, b, m.n, m.h, m.w, m.ch, dt, 128.f, 255.f, 0.01f, 0.03f, m.levels == 3 ? wts : nullptr, m.levels, score, ssim, cs, mean, ws,
                       wsb, nullptr), "tg_msssim");
      });
    }
  for (int hw : {16, 32, 64})
    for (int dt : {TG_F32, TG_BF16, TG_F16})
      for (int n : {1, 3}) {
        if (hw == 64 && n == 3) continue;
        add(std::string("swd_pyramid.") + dname(dt) + ".n" + std::to_string(n) + "_hw" + std::to_string(hw), [=](Ctx& c) {
          const void* x = c.in_pos("x", (size_t)n * hw * hw * 3, dt);
          const size_t wsb = tg_swd_pyramid_workspace_bytes(n, hw);
          if (!wsb) throw Fail{"tg_swd_pyramid_workspace_bytes: 0"};
          void* ws = c.scratch("ws", wsb);      // the levels and the Gaussian scratch behind them: not every byte is a result
          c.go();
          need(tg_swd_pyramid(x, n, hw, 3, dt, 128.f, dt == TG_F32, ws, wsb, nullptr), "tg_swd_pyramid");
        });
      }
  for (int per : {1, 16})
    for (int s : {16, 32})
      add("swd_descriptors.s" + std::to_string(s) + "_per" + std::to_string(per), [=](Ctx& c) {
        const int n = 3;
        const float* level = (const float*)c.in("level", (size_t)n * s * s * 3, F32);
        std::vector<int32_t> tab(n * per * 2);
        for (int i = 0; i < n * per; ++i) tab[2 * i] = 3 + (int)(c.next() % (s - 6)), tab[2 * i + 1] = 3 + (int)(c.next() % (s - 6));
        tab[0] = 3, tab[1] = 3, tab[n * per * 2 - 2] = s - 4, tab[n * per * 2 - 1] = s - 4;      // both ends of the range
        const int* centres = (const int*)c.in_bytes("centres", tab.data(), tab.size() * 4);
        float* o = (float*)c.out("out", (size_t)n * per * 147, F32);
        c.go();
        need(tg_swd_descriptors(level, centres, n, s, per, o, 0, (int64_t)n * per, nullptr), "tg_swd_descriptors");
      });
  // N = 1, 2, 147 and 768 descriptors (tests/test_gpu_swd.py): one row, below and above a chunk of the statistics
  for (int64_t N : {(int64_t)1, (int64_t)2, (int64_t)147, (int64_t)768}) {
    const int repeats = 2, dirs_per = 8;
    int64_t npad = 1;
    while (npad < N) npad *= 2;
    const std::string tag = "N" + std::to_string(N);
    add("swd_project." + tag, [=](Ctx& c) {
      const float* desc = (const float*)c.in("desc", N * 147, F32);
      const float* dirs = (const float*)c.in("dirs", (size_t)repeats * 147 * dirs_per, F32);
      float* proj = (float*)c.out("proj", (size_t)repeats * dirs_per * npad, F32, false);      // rows N..Npad-1 are +inf
      float* stats = (float*)c.out("stats", 6, F32);
      const size_t wsb = tg_swd_project_workspace_bytes(N, repeats, dirs_per);
      void* ws = c.scratch("ws", wsb);
      c.go();
      need(tg_swd_project(desc, dirs, N, repeats, dirs_per, proj, stats, ws, wsb, nullptr), "tg_swd_project");
    });
    add("swd_mean_abs_diff." + tag, [=](Ctx& c) {
      const float* a = (const float*)c.in("a", (size_t)repeats * dirs_per * npad, F32);
      const float* b = (const float*)c.in("b", (size_t)repeats * dirs_per * npad, F32);
      float* o = (float*)c.out("out", repeats + 1, F32);
      const size_t wsb = tg_swd_mean_abs_diff_workspace_bytes(N, repeats, dirs_per);
      void* ws = c.scratch("ws", wsb);
      c.go();
      need(tg_swd_mean_abs_diff(a, b, N, npad, repeats, dirs_per, o, ws, wsb, nullptr), "tg_swd_mean_abs_diff");
    });
    for (int st = 0; st < 2; ++st)
      add(std::string(st ? "swd_distance_stats." : "swd_distance.") + tag, [=](Ctx& c) {
        const float* da = (const float*)c.in("desc_a", N * 147, F32);
        const float* db = (const float*)c.in("desc_b", N * 147, F32);
        const float* dirs = (const float*)c.in("dirs", (size_t)repeats * 147 * dirs_per, F32);
        float* o = (float*)c.out("out", repeats + 1, F32);
        float* stats = st ? (float*)c.out("stats", 12, F32) : nullptr;
        const size_t wsb = tg_swd_distance_workspace_bytes(N, repeats, dirs_per);
        void* ws = c.scratch("ws", wsb);
        c.go();
        need(tg_swd_distance(da, N, db, N, dirs, repeats, dirs_per, o, stats, ws, wsb, nullptr), "tg_swd_distance");
      });
  }
  // the sort: below a block, one block, and two / four blocks (the global passes)
  for (int64_t mult : {(int64_t)0, (int64_t)1, (int64_t)2, (int64_t)4})
    add("swd_sort_columns.blocks" + std::to_string(mult), [=](Ctx& c) {
      const int64_t npad = mult ? mult * tg_swd_sort_block() : 8;
      const int cols = 3;
      float* keys = (float*)c.inout("keys", (size_t)cols * npad, F32);
      c.go();
      need(tg_swd_sort_columns(keys, cols, npad, nullptr), "tg_swd_sort_columns");
    });
}

void register_cases() {
  register_conv_cases();
  register_upcat_cases();
  register_pointwise_cases();
  register_norm_cases();
  register_elementwise_cases();
  register_attention_cases();
  register_loss_cases();
  register_optimiser_cases();
  register_sn_cases();
  register_data_cases();
}
