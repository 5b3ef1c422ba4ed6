// syncnorm_bounds: bounds_main.cpp's sibling for include/twingan_hip_syncnorm.h (TEST INFRASTRUCTURE, built and run by
// tests/test_syncnorm_cpu.py as child processes; nothing loads it into python).  Linked with the AddressSanitizer objects of
// the emulated kernels that build.py build_bounds() leaves under _build_asan/ (all but bounds_main.o).
//
//   syncnorm_bounds --list          the case names, one per line
//   syncnorm_bounds --case NAME     runs one case: exit 0 and "ok NAME", or non-zero with a one-line reason on stderr
//
// Every buffer an entry point reads or writes is a heap allocation of its own whose LAST byte is the last byte of its
// documented size (y / gz / gy [n, h, w, c], gz_pooled [n, h/2, w/2, c], pn_scale [n*h*w], mean / rstd [n*c], moments
// [n][3][c], local [n][2][c], gathered [replicas][n][3 or 2][c], ws [n * tg_norm_chunks * 2 * c], the parameters [c] or
// [n][c]), so the sanitizer's redzone begins where the code must stop.  After rc == 0 the inputs are unchanged, and the results equal a plain host loop
// in double to a tolerance far above fp32 rounding (integer-valued inputs: the data is exact in the three formats).
#if !defined(__has_feature)
#error "syncnorm_bounds_main.cpp needs clang's __has_feature"
#elif !__has_feature(address_sanitizer)
#error "syncnorm_bounds_main.cpp is only meaningful under -fsanitize=address"
#endif
#include <sanitizer/asan_interface.h>

#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/twingan_hip_syncnorm.h"

namespace {

struct Fail {
  std::string why;
};

const unsigned char FILL = 0xA5;

struct Buf {
  unsigned char* p = nullptr;
  size_t bytes = 0;
  std::vector<unsigned char> before;
  Buf(const char* name, size_t n) : bytes(n) {
    void* q = nullptr;
    if (posix_memalign(&q, 16, n)) throw Fail{"out of memory"};
    p = (unsigned char*)q;
    unsigned char* end = p + n;
    if (__asan_address_is_poisoned(end - 1) || !__asan_address_is_poisoned(end))
      throw Fail{std::string(name) + ": the sanitizer's redzone does not begin at the end of the buffer"};
    memset(p, FILL, n);
  }
  ~Buf() { free(p); }
  Buf(const Buf&) = delete;
  float* f() { return (float*)p; }
  void keep() { before.assign(p, p + bytes); }
  void check_same(const char* name) const {
    if (memcmp(p, before.data(), bytes) != 0) throw Fail{std::string(name) + " was written (an input)"};
  }
};

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t next_u32() {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(rng_state >> 33);
}
int draw() { return (int)(next_u32() % 9) - 4; }      // integers in [-4, 4]: exact in the three formats

const char* DT_NAMES[] = {"f32", "bf16", "f16"};
size_t esize(int dtype) { return dtype == TG_F32 ? 4 : 2; }
void put(unsigned char* p, int dtype, size_t i, float v) {
  if (dtype == TG_F32) memcpy(p + 4 * i, &v, 4);
  else if (dtype == TG_BF16) {
    uint32_t b;
    memcpy(&b, &v, 4);
    uint16_t h = (uint16_t)(b >> 16);      // exact for the values drawn
    memcpy(p + 2 * i, &h, 2);
  } else {
    _Float16 h = (_Float16)v;
    memcpy(p + 2 * i, &h, 2);
  }
}
float get(const unsigned char* p, int dtype, size_t i) {
  if (dtype == TG_F32) {
    float v;
    memcpy(&v, p + 4 * i, 4);
    return v;
  }
  if (dtype == TG_BF16) {
    uint16_t h;
    memcpy(&h, p + 2 * i, 2);
    uint32_t b = (uint32_t)h << 16;
    float v;
    memcpy(&v, &b, 4);
    return v;
  }
  _Float16 h;
  memcpy(&h, p + 2 * i, 2);
  return (float)h;
}

struct Shape {
  const char* tag;
  int n, h, w, c;
};
// one chunk / a tail chunk / several chunks; vector path (c = 8, 32) and scalar path (c = 3, 24); even h, w for the pooled input
const Shape SHAPES[] = {{"n1_4x4_c8", 1, 4, 4, 8}, {"n3_10x26_c3", 3, 10, 26, 3}, {"n2_10x26_c32", 2, 10, 26, 32},
                        {"n2_64x16_c24", 2, 64, 16, 24}};

struct Case {
  std::string name;
  int kind;      // 0 moments, 1 merge, 2 backward sums, 3 backward apply
  int dtype, shape, variant;
};
std::vector<Case> cases;

void register_cases() {
  for (int dt = 0; dt < 3; ++dt)
    for (int s = 0; s < 4; ++s) {
      const std::string tail = std::string("_") + DT_NAMES[dt] + "_" + SHAPES[s].tag;
      cases.push_back(Case{"tg_norm_moments" + tail, 0, dt, s, 0});
      // variants: 0 returned [c] gradients, 1 accumulated, two domains, 2 rows [n][c], pooled gradient only
      for (int v = 0; v < 3; ++v) cases.push_back(Case{"tg_norm_act_bwd_sums" + tail + "_v" + std::to_string(v), 2, dt, s, v});
      for (int v = 0; v < 3; ++v) cases.push_back(Case{"tg_norm_act_bwd_apply" + tail + "_v" + std::to_string(v), 3, dt, s, v});
    }
  for (int r : {1, 2, 8})
    for (int s = 0; s < 4; ++s) cases.push_back(Case{"tg_norm_moments_merge_r" + std::to_string(r) + "_" + SHAPES[s].tag, 1, 0, s, r});
}

void ok(int rc, const char* what) {
  if (rc != 0) throw Fail{std::string(what) + ": rc " + std::to_string(rc) + " (" + tg_last_error() + ")"};
}
void near(double got, double want, double tol, const std::string& what) {
  if (!(fabs(got - want) <= tol * (1.0 + fabs(want))))
    throw Fail{what + ": got " + std::to_string(got) + ", the host loop gives " + std::to_string(want)};
}

void run_moments(const Case& cs) {
  const Shape& s = SHAPES[cs.shape];
  const size_t hw = (size_t)s.h * s.w, numel = s.n * hw * s.c;
  Buf y("y", numel * esize(cs.dtype));
  for (size_t i = 0; i < numel; ++i) put(y.p, cs.dtype, i, (float)draw());
  y.keep();
  const int chunks = tg_norm_chunks(s.n, s.h, s.w);
  if (chunks < 1) throw Fail{"tg_norm_chunks"};
  Buf ws("ws", (size_t)s.n * chunks * 2 * s.c * 4), mom("moments", (size_t)s.n * 3 * s.c * 4);
  ok(tg_norm_moments(y.p, mom.f(), ws.f(), s.n, s.h, s.w, s.c, cs.dtype, nullptr), "tg_norm_moments");
  y.check_same("y");
  for (int g = 0; g < s.n; ++g)
    for (int ch = 0; ch < s.c; ++ch) {
      double m = 0, m2 = 0;
      for (size_t p = 0; p < hw; ++p) m += get(y.p, cs.dtype, (g * hw + p) * s.c + ch);
      m /= (double)hw;
      for (size_t p = 0; p < hw; ++p) {
        const double d = get(y.p, cs.dtype, (g * hw + p) * s.c + ch) - m;
        m2 += d * d;
      }
      near((double)mom.f()[(g * 3) * s.c + ch] + (double)mom.f()[(g * 3 + 1) * s.c + ch], m, 1e-6, "mean");
      if (fabs(mom.f()[(g * 3 + 1) * s.c + ch]) > 1e-6 * (1.0 + fabs(m))) throw Fail{"the mean's second word is not a rounding remainder"};
      near(mom.f()[(g * 3 + 2) * s.c + ch], m2, 1e-4, "M2");
    }
  if (tg_norm_moments(nullptr, mom.f(), ws.f(), s.n, s.h, s.w, s.c, cs.dtype, nullptr) == 0 ||
      tg_norm_moments(y.p, mom.f(), ws.f(), s.n, s.h, s.w, s.c, 7, nullptr) == 0)
    throw Fail{"a bad argument was accepted"};
}

void run_merge(const Case& cs) {
  const Shape& s = SHAPES[cs.shape];
  const int R = cs.variant;
  const int64_t count = (int64_t)s.h * s.w;
  const size_t row = (size_t)s.n * 3 * s.c;
  Buf g("gathered", R * row * 4), mean("mean", (size_t)s.n * s.c * 4), rstd("rstd", (size_t)s.n * s.c * 4);
  for (int r = 0; r < R; ++r)
    for (int q = 0; q < s.n; ++q)
      for (int ch = 0; ch < s.c; ++ch) {
        g.f()[r * row + (q * 3) * s.c + ch] = (float)draw();
        g.f()[r * row + (q * 3 + 1) * s.c + ch] = 0.0625f * draw();
        g.f()[r * row + (q * 3 + 2) * s.c + ch] = (float)(count * (1 + next_u32() % 5));
      }
  g.keep();
  const float eps = 1e-3f;
  ok(tg_norm_moments_merge(g.f(), R, count, mean.f(), rstd.f(), s.n, s.c, eps, nullptr), "tg_norm_moments_merge");
  g.check_same("gathered");
  for (int q = 0; q < s.n; ++q)
    for (int ch = 0; ch < s.c; ++ch) {
      double m = 0, m2 = 0;
      for (int r = 0; r < R; ++r) m += (double)g.f()[r * row + (q * 3) * s.c + ch] + g.f()[r * row + (q * 3 + 1) * s.c + ch];
      m /= R;
      for (int r = 0; r < R; ++r) {
        const double d = (double)g.f()[r * row + (q * 3) * s.c + ch] + g.f()[r * row + (q * 3 + 1) * s.c + ch] - m;
        m2 += g.f()[r * row + (q * 3 + 2) * s.c + ch] + (double)count * d * d;
      }
      near(mean.f()[q * s.c + ch], m, 1e-5, "mean");
      near(rstd.f()[q * s.c + ch], 1.0 / sqrt(m2 / ((double)R * count) + eps), 1e-4, "rstd");
    }
  if (tg_norm_moments_merge(g.f(), 0, count, mean.f(), rstd.f(), s.n, s.c, eps, nullptr) == 0 ||
      tg_norm_moments_merge(g.f(), R, 0, mean.f(), rstd.f(), s.n, s.c, eps, nullptr) == 0 ||
      tg_norm_moments_merge(g.f(), 4, 1ll << 30, mean.f(), rstd.f(), s.n, s.c, eps, nullptr) == 0 ||
      tg_norm_moments_merge(nullptr, R, count, mean.f(), rstd.f(), s.n, s.c, eps, nullptr) == 0)
    throw Fail{"a bad argument was accepted"};
}

// The two backward entry points.  No activation and no pixel norm in the host loop's cases (variant 0, 1: flags 0; the
// flagged paths run for their addresses, variant 2: LeakyReLU, + pixel norm on the vector path): gu = g, yhat = (y - mean) rstd.
void run_backward(const Case& cs) {
  const Shape& s = SHAPES[cs.shape];
  const int v = cs.variant, dt = cs.dtype;
  const size_t hw = (size_t)s.h * s.w, numel = s.n * hw * s.c;
  const bool rows = v == 2, two = v == 1, pooled_only = v == 2;
  const int vn = dt == TG_F32 ? 4 : 8;
  const bool vec = s.c % vn == 0 && ((s.c / vn) & (s.c / vn - 1)) == 0 && s.c / vn <= 64;
  const int flags = v == 2 ? (1 | (vec ? 2 : 0)) : 0;
  const int R = 2;
  Buf y("y", numel * esize(dt)), gz("gz", numel * esize(dt)), gzp("gz_pooled", numel / 4 * esize(dt)), gy("gy", numel * esize(dt));
  Buf pn("pn_scale", s.n * hw * 4), mean("mean", (size_t)s.n * s.c * 4), rstd("rstd", (size_t)s.n * s.c * 4);
  const size_t prow = rows ? (size_t)s.n * s.c : (size_t)s.c;
  Buf ga("gamma", prow * 4), be("beta", prow * 4), ga2("gamma2", prow * 4), be2("beta2", prow * 4);
  Buf gga("ggamma", prow * 4), gbe("gbeta", prow * 4), gga2("ggamma2", prow * 4), gbe2("gbeta2", prow * 4);
  const int chunks = tg_norm_chunks(s.n, s.h, s.w);
  Buf ws("ws", (size_t)s.n * chunks * 2 * s.c * 4), local("local", (size_t)s.n * 2 * s.c * 4);
  Buf gathered("gathered", (size_t)R * s.n * 2 * s.c * 4);
  for (size_t i = 0; i < numel; ++i) {
    put(y.p, dt, i, (float)draw());
    put(gz.p, dt, i, (float)draw());
  }
  for (size_t i = 0; i < numel / 4; ++i) put(gzp.p, dt, i, (float)(4 * draw()));
  for (size_t i = 0; i < s.n * hw; ++i) pn.f()[i] = 0.5f;
  for (int i = 0; i < s.n * s.c; ++i) {
    mean.f()[i] = 0.25f * draw();
    rstd.f()[i] = 0.5f + 0.125f * (next_u32() % 4);
  }
  for (size_t i = 0; i < prow; ++i) {
    ga.f()[i] = 1.f + 0.25f * draw();
    be.f()[i] = 0.25f * draw();
    ga2.f()[i] = 1.f + 0.25f * draw();
    be2.f()[i] = 0.25f * draw();
    gga.f()[i] = gbe.f()[i] = gga2.f()[i] = gbe2.f()[i] = 1.f;      // what `accumulate` adds to
  }
  for (size_t i = 0; i < (size_t)R * s.n * 2 * s.c; ++i) gathered.f()[i] = (float)draw();
  for (Buf* b : {&y, &gz, &gzp, &pn, &mean, &rstd, &ga, &be, &ga2, &be2, &gathered}) b->keep();
  const int split = two ? s.n / 2 : s.n;
  const void* gz_in = pooled_only ? nullptr : gz.p;
  const void* gzp_in = pooled_only ? gzp.p : nullptr;
  // the incoming gradient of pixel p, channel ch of group g
  auto gin = [&](int g, size_t p, int ch) -> double {
    if (!pooled_only) return get(gz.p, dt, (g * hw + p) * s.c + ch);
    const size_t yy = p / s.w, xx = p % s.w;
    return 0.25 * get(gzp.p, dt, ((g * (size_t)(s.h / 2) + yy / 2) * (s.w / 2) + xx / 2) * s.c + ch);
  };
  auto par = [&](Buf& a, Buf& b, int g, int ch) -> double { return rows ? a.f()[g * s.c + ch] : (g < split ? a : b).f()[ch]; };
  if (cs.kind == 2) {
    ok(tg_norm_act_bwd_sums(gz_in, gzp_in, y.p, flags & 2 ? pn.f() : nullptr, mean.f(), rstd.f(), ga.f(), be.f(), two ? ga2.f() : nullptr,
                            two ? be2.f() : nullptr, split, rows ? 1 : 0, gga.f(), gbe.f(), two ? gga2.f() : nullptr,
                            two ? gbe2.f() : nullptr, ws.f(), local.f(), s.n, s.h, s.w, s.c, flags, 0.2f, v == 1 ? 1 : 0, dt, nullptr),
       "tg_norm_act_bwd_sums");
    if (flags == 0) {
      std::vector<double> pg(4 * s.c, 0.0);      // gbeta, ggamma, gbeta2, ggamma2
      for (int g = 0; g < s.n; ++g)
        for (int ch = 0; ch < s.c; ++ch) {
          double s1 = 0, s2 = 0;
          for (size_t p = 0; p < hw; ++p) {
            const double gu = gin(g, p, ch);
            s1 += gu;
            s2 += gu * (get(y.p, dt, (g * hw + p) * s.c + ch) - mean.f()[g * s.c + ch]) * rstd.f()[g * s.c + ch];
          }
          near(local.f()[(g * 2) * s.c + ch], s1, 1e-5 * hw, "S1");
          near(local.f()[(g * 2 + 1) * s.c + ch], s2, 1e-5 * hw, "S2");
          pg[(g < split ? 0 : 2) * s.c + ch] += s1;
          pg[(g < split ? 1 : 3) * s.c + ch] += s2;
        }
      const double base = v == 1 ? 1.0 : 0.0;
      for (int ch = 0; ch < s.c; ++ch) {
        near(gbe.f()[ch], base + pg[ch], 1e-5 * hw * s.n, "gbeta");
        near(gga.f()[ch], base + pg[s.c + ch], 1e-5 * hw * s.n, "ggamma");
        if (two) {
          near(gbe2.f()[ch], base + pg[2 * s.c + ch], 1e-5 * hw * s.n, "gbeta2");
          near(gga2.f()[ch], base + pg[3 * s.c + ch], 1e-5 * hw * s.n, "ggamma2");
        }
      }
    } else {      // rows: the group's sums are its gradient rows, bit for bit
      for (int i = 0; i < s.n * s.c; ++i) {
        const int g = i / s.c, ch = i % s.c;
        if (gbe.f()[i] != local.f()[(g * 2) * s.c + ch] || gga.f()[i] != local.f()[(g * 2 + 1) * s.c + ch])
          throw Fail{"the gradient rows are not the group's sums"};
      }
    }
    if (tg_norm_act_bwd_sums(gz_in, gzp_in, y.p, nullptr, mean.f(), rstd.f(), ga.f(), be.f(), nullptr, nullptr, split, rows ? 1 : 0,
                             nullptr, nullptr, nullptr, nullptr, ws.f(), local.f(), s.n, s.h, s.w, s.c, 4, 0.2f, 0, dt, nullptr) == 0 ||
        tg_norm_act_bwd_sums(gz_in, gzp_in, y.p, nullptr, mean.f(), rstd.f(), ga.f(), be.f(), nullptr, nullptr, split, 1, nullptr,
                             nullptr, nullptr, nullptr, ws.f(), local.f(), s.n, s.h, s.w, s.c, 0, 0.2f, 1, dt, nullptr) == 0 ||
        tg_norm_act_bwd_sums(nullptr, nullptr, y.p, nullptr, mean.f(), rstd.f(), ga.f(), be.f(), nullptr, nullptr, split, 0, nullptr,
                             nullptr, nullptr, nullptr, ws.f(), local.f(), s.n, s.h, s.w, s.c, 0, 0.2f, 0, dt, nullptr) == 0)
      throw Fail{"a bad argument was accepted"};
  } else {
    ok(tg_norm_act_bwd_apply(gz_in, gzp_in, y.p, flags & 2 ? pn.f() : nullptr, mean.f(), rstd.f(), ga.f(), be.f(), two ? ga2.f() : nullptr,
                             two ? be2.f() : nullptr, split, rows ? 1 : 0, gy.p, gathered.f(), R, s.n, s.h, s.w, s.c, flags, 0.2f, dt,
                             nullptr),
       "tg_norm_act_bwd_apply");
    if (flags == 0) {
      const double N = (double)R * hw;
      for (int g = 0; g < s.n; ++g)
        for (int ch = 0; ch < s.c; ++ch) {
          double s1 = 0, s2 = 0;
          for (int r = 0; r < R; ++r) {
            s1 += gathered.f()[((size_t)(r * s.n + g) * 2) * s.c + ch];
            s2 += gathered.f()[((size_t)(r * s.n + g) * 2 + 1) * s.c + ch];
          }
          const double rs = rstd.f()[g * s.c + ch], gm = par(ga, ga2, g, ch);
          for (size_t p = 0; p < hw; ++p) {
            const double yh = (get(y.p, dt, (g * hw + p) * s.c + ch) - mean.f()[g * s.c + ch]) * rs;
            const double want = gm * rs * (gin(g, p, ch) - s1 / N - yh * s2 / N);
            const double got = get(gy.p, dt, (g * hw + p) * s.c + ch);
            if (!(fabs(got - want) <= (dt == TG_F32 ? 1e-5 : dt == TG_F16 ? 2e-3 : 1.6e-2) * (1.0 + fabs(want))))
              throw Fail{"gy differs from the host loop at group " + std::to_string(g) + " pixel " + std::to_string(p)};
          }
        }
    }
    if (tg_norm_act_bwd_apply(gz_in, gzp_in, y.p, nullptr, mean.f(), rstd.f(), ga.f(), be.f(), nullptr, nullptr, split, 0, gy.p,
                              gathered.f(), 0, s.n, s.h, s.w, s.c, 0, 0.2f, dt, nullptr) == 0 ||
        tg_norm_act_bwd_apply(gz_in, gzp_in, y.p, nullptr, mean.f(), rstd.f(), ga.f(), be.f(), nullptr, nullptr, split, 0, gy.p,
                              gathered.f(), R, s.n, s.h, s.w, s.c, 4, 0.2f, dt, nullptr) == 0 ||
        tg_norm_act_bwd_apply(gz_in, gzp_in, y.p, nullptr, mean.f(), rstd.f(), ga.f(), be.f(), nullptr, nullptr, split, 0, nullptr,
                              gathered.f(), R, s.n, s.h, s.w, s.c, 0, 0.2f, dt, nullptr) == 0)
      throw Fail{"a bad argument was accepted"};
  }
  y.check_same("y");
  gz.check_same("gz");
  gzp.check_same("gz_pooled");
  pn.check_same("pn_scale");
  mean.check_same("mean");
  rstd.check_same("rstd");
  ga.check_same("gamma");
  be.check_same("beta");
  ga2.check_same("gamma2");
  be2.check_same("beta2");
  gathered.check_same("gathered");
}

}  // namespace

int main(int argc, char** argv) {
  register_cases();
  if (argc == 2 && !strcmp(argv[1], "--list")) {
    for (const Case& c : cases) printf("%s\n", c.name.c_str());
    return 0;
  }
  if (argc == 3 && !strcmp(argv[1], "--case")) {
    for (const Case& c : cases)
      if (c.name == argv[2]) {
        try {
          if (c.kind == 0) run_moments(c);
          else if (c.kind == 1) run_merge(c);
          else run_backward(c);
        } catch (const Fail& f) {
          fprintf(stderr, "FAIL %s: %s\n", c.name.c_str(), f.why.c_str());
          return 1;
        }
        printf("ok %s\n", c.name.c_str());
        return 0;
      }
    fprintf(stderr, "FAIL %s: no such case\n", argv[2]);
    return 2;
  }
  fprintf(stderr, "usage: syncnorm_bounds --list | syncnorm_bounds --case NAME\n");
  return 2;
}
