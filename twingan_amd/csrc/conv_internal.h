// Internal interface between the conv translation units and capi.hip: every function one of them calls in another is
// declared here, once, with its default arguments; the definitions include this header, so the compiler checks them
// against it.  (The error / kernel-name plumbing every file uses is in tg_common.h, the C ABI in twingan_hip.h.)
#pragma once
#include "tg_common.h"

// the operation of a conv call: forward-shaped (forward, masked, pool), backward-data-shaped, filter gradient.
// TG_GRP_FWD / TG_GRP_DGRAD are also the `mode` of the weight pack the operation reads (tg_conv2d_pack_weights).
enum { TG_GRP_FWD = 0, TG_GRP_DGRAD = 1, TG_GRP_WGRAD = 2 };

// A stride-1 conv as a kernel sees it.  Backward-data is the forward conv over gy with the rotated pack: in = (hout, wout,
// cout), out = (hin, win, cin), pad' = k - 1 - pad of the descriptor.
struct TgConvShape {
  int n, hin, win, cin, hout, wout, cout, kh, kw, pad_t, pad_l;
};

// Optional operands of tg_conv_tile_run / tg_conv_img_run / tg_conv_small_run, all off by default.  conv_img and conv_small
// read mask, stats, groups and wset_elems only.
struct TgConvExtras {
  const void* mask = nullptr;           // out *= LeakyReLU'(mask), same shape as the output
  float* stats = nullptr;               // per-workgroup statistics partials of the output (plain epilogue only)
  int stat_chunks = 0;                  // conv_tile: chunks per image the caller sized `stats` for
  void* ypool = nullptr;                // conv_tile POOL: also write avg_pool2x2 of the output
  void* ymask = nullptr;                // conv_tile POOL: sign bits instead of the output itself
  const void* up_src = nullptr;         // conv_tile UNPOOL: gradient of the pooled output (the conv input is never in memory)
  const void* up_signs = nullptr;       //   sign bytes of the layer's activation output, or
  const void* up_z = nullptr;           //   that output itself
  float up_alpha = 0.f;
  void* up_store = nullptr;             //   optionally also store the unpooled gradient
  int groups = 1;                       // weight sets: image i reads set i / (n / groups)
  size_t wset_elems = 0;                // elements of one set's pack
};

// ---- conv_direct.hip
int tg_conv2d_fwd_direct(const TgConvDesc* d, const void* x, const void* w, const float* bias, void* y, hipStream_t s);
int tg_conv2d_bwd_data_direct(const TgConvDesc* d, const void* gy, const void* w, void* gx, hipStream_t s);
size_t tg_conv2d_bwd_weight_workspace_direct(const TgConvDesc* d);
int tg_conv2d_bwd_weight_direct(const TgConvDesc* d, const void* x, const void* gy, float* gw, int accumulate, hipStream_t s,
                                void* ws = nullptr, size_t ws_bytes = 0);

// ---- conv_mfma.hip: the MFMA side of the C ABI entry points (16-bit activations, algo != TG_ALGO_DIRECT)
bool tg_conv2d_grouped_native_mfma(const TgConvDesc* d, int op);
int tg_conv2d_fwd_mfma(const TgConvDesc* d, const void* x, const void* wp, const float* bias, void* y, hipStream_t s);
bool tg_conv2d_fwd_mask_fusable_mfma(const TgConvDesc* d);
int tg_conv2d_fwd_masked_mfma(const TgConvDesc* d, const void* x, const void* wp, const void* mask_src, void* y, hipStream_t s);
bool tg_conv2d_fwd_pool_supported_mfma(const TgConvDesc* d);
int tg_conv2d_fwd_pool_mfma(const TgConvDesc* d, const void* x, const void* wp, const float* bias, void* y, void* ypool,
                            hipStream_t s, void* ymask = nullptr);
int tg_conv2d_fwd_stats_chunks_mfma(const TgConvDesc* d);
int tg_conv2d_fwd_stats_mfma(const TgConvDesc* d, const void* x, const void* wp, void* y, float* partials, int chunks,
                             hipStream_t s);
bool tg_conv2d_bwd_data_mask_fusable_mfma(const TgConvDesc* d);
int tg_conv2d_bwd_data_mfma(const TgConvDesc* d, const void* gy, const void* wp, void* gx, hipStream_t s,
                            const void* mask = nullptr);
bool tg_conv2d_bwd_data_unpool_supported_mfma(const TgConvDesc* d);
int tg_conv2d_bwd_data_unpool_mfma(const TgConvDesc* d, const void* gy_pooled, const void* y_signs, const void* wp, void* gx,
                                   hipStream_t s, const void* mask, void* gy_out, const void* y_act);
size_t tg_conv2d_bwd_weight_workspace_mfma(const TgConvDesc* d);
bool tg_conv2d_bwd_weight_bias_fused_mfma(const TgConvDesc* d);
int tg_conv2d_bwd_weight_mfma(const TgConvDesc* d, const void* x, const void* gy, float* gw, int accumulate, void* ws,
                              size_t ws_bytes, hipStream_t s, float* gbias = nullptr);
bool tg_conv2d_bwd_weight2_supported_mfma(const TgConvDesc* d);
size_t tg_conv2d_bwd_weight2_workspace_mfma(const TgConvDesc* d, int nb);
int tg_conv2d_bwd_weight2_mfma(const TgConvDesc* d, int nb, const void* xa, const void* gya, const void* xb, const void* gyb,
                               float* gw, int accumulate, void* ws, size_t ws_bytes, hipStream_t s, float* gbias = nullptr,
                               int bias_segs = 3);

// ---- conv_tile.hip
bool tg_conv_tile_supported(int h, int w, int hout, int wout, int kh, int kw, int pad_t, int pad_l);
bool tg_conv_tile_grouped_native(const TgConvShape& c);
int tg_conv_tile_stats_chunks(const TgConvShape& c);
int tg_conv_tile_run(const TgConvShape& c, int epilogue, float alpha, const void* x, const void* wp, const float* bias, void* y,
                     hipStream_t s, const TgConvExtras& ex = {});
bool tg_conv_tile_upcat_supported(int h, int w, int c0, int c1, int cout);
int tg_conv_tile_upcat_run(int n, int h, int w, int c0, int c1, int cout, int gsz, unsigned perm, const void* x0,
                           const void* x1, const void* wp, void* y, hipStream_t s, float* stats = nullptr,
                           int stat_chunks = 0, int* chunks_query = nullptr);
int tg_conv_tile_upcat_bwd_run(int n, int h, int w, int c0, int c1, int cout, int gsz, unsigned perm, int n1, const void* gy,
                               const void* wp, void* g0, void* g1, hipStream_t s);

// ---- conv_img.hip / conv_small.hip
bool tg_conv_img_supported(int n, int hin, int win, int cin, int hout, int wout, int cout, int k, int pad_t, int pad_l);
bool tg_conv_img_stats_supported(int n, int hin, int win, int cin, int hout, int wout, int cout, int k, int pad_t, int pad_l);
int tg_conv_img_run(const TgConvShape& c, int epilogue, float alpha, const void* x, const void* wp, const float* bias, void* y,
                    hipStream_t s, const TgConvExtras& ex = {});
bool tg_conv_small_supported(int n, int hout, int wout, int kh, int kw);
bool tg_conv_small_stats_supported(int n, int hin, int win, int hout, int wout, int cout, int k, int pad_t, int pad_l);
int tg_conv_small_run(const TgConvShape& c, int epilogue, float alpha, const void* x, const void* wp, const float* bias, void* y,
                      hipStream_t s, const TgConvExtras& ex = {});

// ---- conv_wgrad_tile.hip
bool tg_wgrad_tile_supported(int h, int w, int hout, int wout, int kh, int kw, int pad_t, int pad_l);
size_t tg_wgrad_tile_workspace(int n, int h, int w, int cin, int cout);
int tg_wgrad_tile_run(int n, int h, int w, int cin, int cout, const void* x, const void* gy, float* gw, int accumulate,
                      void* ws, size_t ws_bytes, hipStream_t s, float* gbias = nullptr);
size_t tg_wgrad_tile_workspace2(int na, int nb, int h, int w, int cin, int cout);
int tg_wgrad_tile_run2(int na, int nb, int h, int w, int cin, int cout, const void* xa, const void* gya, const void* xb,
                       const void* gyb, float* gw, int accumulate, void* ws, size_t ws_bytes, hipStream_t s,
                       float* gbias = nullptr, int bias_segs = 3);
int tg_wgrad_tile_upcat_run(int n, int h, int w, int c0, int c1, int cout, int gsz, unsigned perm, const void* x0,
                            const void* x1, const void* gy, float* gw, int accumulate, void* ws, size_t ws_bytes,
                            hipStream_t s);
int tg_wgrad_slab_reduce(const float* slab, float* gw, int64_t nw, int nslices, int accumulate, hipStream_t s);
