// knn_bounds: bounds_main.cpp's sibling for include/twingan_hip_knn.h (TEST INFRASTRUCTURE, built and run by
// tests/test_knn_cpu.py as child processes; nothing loads it into python).  Linked with the AddressSanitizer objects of the
// emulated kernels that build.py build_bounds() leaves under _build_asan/ (all but bounds_main.o).
//
//   knn_bounds --list          the case names, one per line
//   knn_bounds --case NAME     runs one case: exit 0 and "ok NAME", or non-zero with a one-line reason on stderr
//
// Every buffer an entry point reads or writes is a heap allocation of its own whose LAST byte is the last byte of its
// documented size (queries [q, d], gallery [n, d], query_ids [q], dist / idx [q, k], the workspace of exactly
// tg_knn_workspace_bytes, the norms [rows]), so the sanitizer's redzone begins where the code must stop; `o` cases start the
// operands 2 or 4 bytes into their allocation (no 16-byte alignment: the scalar staging), and those bytes must keep their
// fill.  After rc == 0 the inputs are unchanged and the results equal a plain host loop (integer-valued inputs: exact).
#if !defined(__has_feature)
#error "knn_bounds_main.cpp needs clang's __has_feature"
#elif !__has_feature(address_sanitizer)
#error "knn_bounds_main.cpp is only meaningful under -fsanitize=address"
#endif
#include <sanitizer/asan_interface.h>

#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "../../include/twingan_hip_knn.h"

namespace {

struct Fail {
  std::string why;
};

const unsigned char FILL = 0xA5;

struct Buf {
  unsigned char* base = nullptr;
  unsigned char* p = nullptr;
  size_t bytes = 0, front = 0;
  std::vector<unsigned char> before;
  Buf(const char* name, size_t n, size_t front_ = 0) : bytes(n), front(front_) {
    void* q = nullptr;
    if (posix_memalign(&q, 16, n + front_)) throw Fail{"out of memory"};
    base = (unsigned char*)q;
    p = base + front_;
    unsigned char* end = p + n;
    if (__asan_address_is_poisoned(end - 1) || !__asan_address_is_poisoned(end))
      throw Fail{std::string(name) + ": the sanitizer's redzone does not begin at the end of the buffer"};
    memset(base, FILL, n + front_);
  }
  ~Buf() { free(base); }
  void keep() { before.assign(p, p + bytes); }
  void check_front(const char* name) const {
    for (size_t i = 0; i < front; ++i)
      if (base[i] != FILL) throw Fail{std::string(name) + ": the bytes in front of the buffer were written"};
  }
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

struct Case {
  std::string name;
  int kind;      // 0 topk, 1 sqnorm, 2 plan / workspace
  int dtype, q, n, d, k, off, metric, ids;
};
std::vector<Case> cases;

void register_cases() {
  const int shapes[][4] = {{1, 1, 1, 1}, {3, 5, 16, 8}, {33, 257, 24, 8}, {70, 300, 27, 32}};
  for (int dt = 0; dt < 3; ++dt)
    for (const auto& s : shapes)
      for (int off = 0; off < 2; ++off)
        cases.push_back(Case{std::string("tg_knn_topk_") + DT_NAMES[dt] + "_q" + std::to_string(s[0]) + "_n" + std::to_string(s[1]) + "_d" +
                                 std::to_string(s[2]) + "_k" + std::to_string(s[3]) + (off ? "_o" : "_a"),
                             0, dt, s[0], s[1], s[2], s[3], off, 0, 0});
  for (int dt = 0; dt < 3; ++dt) {
    cases.push_back(Case{std::string("tg_knn_topk_") + DT_NAMES[dt] + "_cosine", 0, dt, 5, 140, 40, 4, 0, 1, 0});
    cases.push_back(Case{std::string("tg_knn_topk_") + DT_NAMES[dt] + "_query_ids", 0, dt, 37, 200, 8, 3, 0, 0, 1});
    cases.push_back(Case{std::string("tg_knn_topk_") + DT_NAMES[dt] + "_cosine_query_ids", 0, dt, 37, 200, 8, 3, 0, 1, 1});
    for (int rows : {1, 131})
      for (int off = 0; off < 2; ++off)
        cases.push_back(Case{std::string("tg_knn_sqnorm_") + DT_NAMES[dt] + "_r" + std::to_string(rows) + (off ? "_o" : "_a"), 1, dt, 0, rows,
                             rows == 1 ? 1 : 43, 0, off, 0, 0});
  }
  cases.push_back(Case{"tg_knn_plan_rule", 2, 0, 0, 0, 0, 0, 0, 0, 0});
}

void ok(int rc, const char* what) {
  if (rc != 0) throw Fail{std::string(what) + ": rc " + std::to_string(rc) + " (" + tg_last_error() + ")"};
}

struct Mat {
  Buf* buf;
  std::vector<int> v;      // rows * d
};
Mat make_mat(const char* name, int rows, int d, int dtype, int off) {
  Mat m{new Buf(name, (size_t)rows * d * esize(dtype), off ? esize(dtype) : 0), {}};
  for (size_t i = 0; i < (size_t)rows * d; ++i) {
    m.v.push_back(draw());
    put(m.buf->p, dtype, i, (float)m.v.back());
  }
  m.buf->keep();
  return m;
}

void run_topk(const Case& c) {
  Mat Q = make_mat("queries", c.q, c.d, c.dtype, c.off), G = make_mat("gallery", c.n, c.d, c.dtype, c.off);
  if (c.metric == 1)
    for (int i = 0; i < c.d; ++i) {      // a zero row: cosine distance 1
      G.v[(size_t)2 * c.d + i] = 0;
      put(G.buf->p, c.dtype, (size_t)2 * c.d + i, 0.f);
    }
  G.buf->keep();
  const int64_t offset = (1ll << 33) + 5;
  Buf ids("query_ids", (size_t)c.q * 8);
  for (int i = 0; i < c.q; ++i) {
    const int64_t v = offset + (i % c.n);
    memcpy(ids.p + 8 * i, &v, 8);
  }
  ids.keep();
  int splits = 0;
  ok(tg_knn_plan(c.q, c.n, c.d, c.k, &splits), "tg_knn_plan");
  const size_t ws_bytes = tg_knn_workspace_bytes(c.q, c.n, c.d, c.k);
  if (splits < 1 || ws_bytes != 4 * (2 * (size_t)splits * c.q * c.k + c.q + c.n)) throw Fail{"plan and workspace size disagree"};
  Buf dist("dist", (size_t)c.q * c.k * 4), idx("idx", (size_t)c.q * c.k * 8);
  for (int i = 0; i < c.q * c.k; ++i) {
    const float inf = INFINITY;
    const int64_t none = -1;
    memcpy(dist.p + 4 * i, &inf, 4);
    memcpy(idx.p + 8 * i, &none, 8);
  }
  // the gallery in two chunks when it has more than one row: the table is in/out
  const int n0 = c.n > 1 ? c.n / 2 : c.n;
  for (int part = 0; part < (c.n > 1 ? 2 : 1); ++part) {
    const int lo = part ? n0 : 0, rows = part ? c.n - n0 : n0;
    // each chunk is its own allocation, so the end of the chunk is the end of a buffer
    Buf chunk("gallery chunk", (size_t)rows * c.d * esize(c.dtype), c.off ? esize(c.dtype) : 0);
    memcpy(chunk.p, G.buf->p + (size_t)lo * c.d * esize(c.dtype), chunk.bytes);
    chunk.keep();
    const size_t need = tg_knn_workspace_bytes(c.q, rows, c.d, c.k);
    Buf w2("workspace", need);
    ok(tg_knn_topk(Q.buf->p, c.q, chunk.p, rows, c.d, c.dtype, c.metric, c.k, offset + lo, c.ids ? (const int64_t*)ids.p : nullptr,
                   (float*)dist.p, (int64_t*)idx.p, w2.p, need, nullptr),
       "tg_knn_topk");
    chunk.check_front("the gallery chunk");
    chunk.check_same("the gallery chunk");
  }
  Q.buf->check_front("the queries");
  Q.buf->check_same("the queries");
  ids.check_same("query_ids");
  for (int i = 0; i < c.q; ++i) {
    std::vector<std::pair<double, int64_t>> all;
    double qn = 0;
    for (int t = 0; t < c.d; ++t) qn += (double)Q.v[(size_t)i * c.d + t] * Q.v[(size_t)i * c.d + t];
    for (int j = 0; j < c.n; ++j) {
      if (c.ids && j == i % c.n) continue;
      double gn = 0, dot = 0;
      for (int t = 0; t < c.d; ++t) {
        gn += (double)G.v[(size_t)j * c.d + t] * G.v[(size_t)j * c.d + t];
        dot += (double)Q.v[(size_t)i * c.d + t] * G.v[(size_t)j * c.d + t];
      }
      double dv = qn + gn - 2 * dot;
      if (c.metric == 1) dv = qn * gn == 0 ? 1.0 : 1.0 - dot / (sqrt(qn) * sqrt(gn));
      all.push_back({dv, offset + j});
    }
    std::sort(all.begin(), all.end());
    for (int s = 0; s < c.k; ++s) {
      float gd;
      int64_t gi;
      memcpy(&gd, dist.p + 4 * ((size_t)i * c.k + s), 4);
      memcpy(&gi, idx.p + 8 * ((size_t)i * c.k + s), 8);
      const std::string who = "query " + std::to_string(i) + " slot " + std::to_string(s);
      if (s >= (int)all.size()) {
        if (gi != -1 || !(isinf(gd) && gd > 0)) throw Fail{who + ": not the +inf / -1 filler"};
      } else if (c.metric == 0) {
        if (gi != all[s].second || (double)gd != all[s].first) throw Fail{who + ": differs from the host loop"};
      } else {      // cosine: fp32 against double on small integers; the index too where the double distances leave no doubt
        if (fabs((double)gd - all[s].first) > 1e-5) throw Fail{who + ": cosine distance differs from the host loop"};
        const bool apart = (s == 0 || all[s].first - all[s - 1].first > 1e-4) &&
                           (s + 1 >= (int)all.size() || all[s + 1].first - all[s].first > 1e-4);
        if (apart && gi != all[s].second) throw Fail{who + ": cosine index differs from the host loop"};
      }
    }
  }
  delete Q.buf;
  delete G.buf;
}

void run_sqnorm(const Case& c) {
  Mat X = make_mat("x", c.n, c.d, c.dtype, c.off);
  Buf out("out_f32", (size_t)c.n * 4);
  ok(tg_knn_sqnorm(X.buf->p, c.n, c.d, c.dtype, (float*)out.p, nullptr), "tg_knn_sqnorm");
  X.buf->check_front("x");
  X.buf->check_same("x");
  for (int r = 0; r < c.n; ++r) {
    float want = 0, got;
    for (int t = 0; t < c.d; ++t) want += (float)(X.v[(size_t)r * c.d + t] * X.v[(size_t)r * c.d + t]);
    memcpy(&got, out.p + 4 * r, 4);
    if (got != want) throw Fail{"row " + std::to_string(r) + ": norm differs"};
  }
  delete X.buf;
}

void run_plan() {
  int s = 0;
  ok(tg_knn_plan(1, 1, 1, 1, &s), "tg_knn_plan");
  if (s != 1) throw Fail{"one row, one split"};
  ok(tg_knn_plan(1024, 131072, 4096, 8, &s), "tg_knn_plan");
  if (s != 32) throw Fail{"1024 queries x 131072 rows: 32 splits, got " + std::to_string(s)};
  ok(tg_knn_plan(1, 131072, 4096, 8, &s), "tg_knn_plan");
  if (s != 256) throw Fail{"one query x 131072 rows: 256 splits, got " + std::to_string(s)};
  ok(tg_knn_plan(70, 1000, 128, 32, &s), "tg_knn_plan");
  if (s != 8) throw Fail{"70 x 1000: one split per tile"};
  if (tg_knn_plan(1, 1, 1, 0, &s) == 0 || tg_knn_plan(1, 1, 1, 33, &s) == 0 || tg_knn_plan(1, 1, 0, 1, &s) == 0 ||
      tg_knn_plan(0, 1, 1, 1, &s) == 0 || tg_knn_plan(1, 0, 1, 1, &s) == 0 || tg_knn_plan(1, 1, 1, 1, nullptr) == 0)
    throw Fail{"a bad argument was accepted"};
  if (tg_knn_workspace_bytes(1, 1, 1, 0) != 0 || tg_knn_workspace_bytes(1, 1, 1, 1) != 4 * (2 + 1 + 1)) throw Fail{"workspace size"};
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
          if (c.kind == 0) run_topk(c);
          else if (c.kind == 1) run_sqnorm(c);
          else run_plan();
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
  fprintf(stderr, "usage: knn_bounds --list | knn_bounds --case NAME\n");
  return 2;
}
