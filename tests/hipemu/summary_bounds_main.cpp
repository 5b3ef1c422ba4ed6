// summary_bounds: bounds_main.cpp's sibling for include/twingan_hip_summary.h (TEST INFRASTRUCTURE, built and run by
// tests/test_monitor_cpu.py as child processes; nothing loads it into python).  Linked with the AddressSanitizer objects of
// the emulated kernels that build.py build_bounds() leaves under _build_asan/ (all but bounds_main.o).
//
//   summary_bounds --list          the case names, one per line
//   summary_bounds --case NAME     runs one case: exit 0 and "ok NAME", or non-zero with a one-line reason on stderr
//
// Every buffer an entry point reads or writes is a heap allocation of its own whose LAST byte is the last byte of its
// documented size (the tensor's elements -- for strided rows up to the last VALID element --, the job table, the limits, the
// workspace, the result rows, the grid), so the sanitizer's redzone begins where the code must stop; `o` cases start the
// tensor 4 bytes into its allocation, and those bytes must keep their fill.  After rc == 0 the inputs are unchanged and the
// results agree with a plain host loop (counts, minimum, maximum, sums, the bucket total; every byte of a grid).
#if !defined(__has_feature)
#error "summary_bounds_main.cpp needs clang's __has_feature"
#elif !__has_feature(address_sanitizer)
#error "summary_bounds_main.cpp is only meaningful under -fsanitize=address"
#endif
#include <sanitizer/asan_interface.h>

#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/twingan_hip_summary.h"

namespace {

struct Fail {
  std::string why;
};

const unsigned char FILL = 0xA5;

// `bytes` bytes that end at the sanitizer's redzone, `front` fill bytes in front of what the library gets
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
// values exactly representable in bf16 and fp16: k / 8, |k| <= 64, with zeros among them
float draw() { return (float)((int)(next_u32() % 129) - 64) / 8.0f; }

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
  int kind;      // 0 dense summary, 1 strided summary, 2 mixed table, 3 grid, 4 limits, 5 summary table fill, 6 grid table fill
  int dtype, numel, off, mode;      // mode: summary 0 plain / 1 scale by value / 2 device scalar / 3 both; grid: c
  int rows, cols;
};
std::vector<Case> cases;

void register_cases() {
  for (int dt = 0; dt < 3; ++dt)
    for (int numel : {1, 1027})
      for (int off = 0; off < 2; ++off)
        cases.push_back(Case{std::string("tg_summary_multi_") + DT_NAMES[dt] + "_n" + std::to_string(numel) + (off ? "_o" : "_a"), 0, dt,
                             numel, off, 0, 0, 0});
  for (int dt = 0; dt < 3; ++dt)
    for (int off = 0; off < 2; ++off)
      cases.push_back(Case{std::string("tg_summary_multi_") + DT_NAMES[dt] + "_strided" + (off ? "_o" : "_a"), 1, dt, 0, off, 0, 0, 0});
  for (int mode = 1; mode < 4; ++mode)
    cases.push_back(Case{std::string("tg_summary_multi_f32_n1027_scale") + std::to_string(mode), 0, TG_F32, 1027, 0, mode, 0, 0});
  cases.push_back(Case{"tg_summary_multi_mixed_table", 2, 0, 0, 0, 0, 0, 0});
  for (int dt = 0; dt < 3; ++dt)
    for (int c : {1, 3}) {
      cases.push_back(Case{std::string("tg_image_grid_u8_") + DT_NAMES[dt] + "_1x1_c" + std::to_string(c), 3, dt, 0, 0, c, 1, 1});
      cases.push_back(Case{std::string("tg_image_grid_u8_") + DT_NAMES[dt] + "_3x2_c" + std::to_string(c), 3, dt, 0, 0, c, 3, 2});
    }
  cases.push_back(Case{"tg_summary_limits_exact", 4, 0, 0, 0, 0, 0, 0});
  cases.push_back(Case{"tg_summary_table_fill_exact", 5, 0, 0, 0, 0, 0, 0});
  cases.push_back(Case{"tg_image_grid_table_fill_exact", 6, 0, 0, 0, 0, 0, 0});
}

void ok(int rc, const char* what) {
  if (rc != 0) throw Fail{std::string(what) + ": rc " + std::to_string(rc) + " (" + tg_last_error() + ")"};
}

struct Job {
  Buf* buf;
  int dtype;
  int64_t rows, valid, stride;
  std::vector<float> vals;      // the valid elements in order
};

Job make_job(int dtype, int64_t rows, int64_t valid, int64_t stride, int off) {
  const size_t phys = (size_t)((rows - 1) * stride + valid);
  Job j{new Buf("tensor", phys * esize(dtype), off ? 4 : 0), dtype, rows, valid, stride, {}};
  const float nanv = NAN;
  for (size_t i = 0; i < phys; ++i) put(j.buf->p, dtype, i, (i & 1) ? nanv : 1e30f);      // the padding: must not show
  for (int64_t r = 0; r < rows; ++r)
    for (int64_t c = 0; c < valid; ++c) {
      const float v = draw();
      j.vals.push_back(v);
      put(j.buf->p, dtype, (size_t)(r * stride + c), v);
    }
  j.buf->keep();
  return j;
}

void run_summary(std::vector<Job>& jobs, float scale, bool dev_scale) {
  const int n = (int)jobs.size();
  float pos_host[TG_SUMMARY_POS_LIMITS];
  ok(tg_summary_limits(nullptr, pos_host), "tg_summary_limits");
  Buf limits("limits_dev", sizeof(pos_host));
  memcpy(limits.p, pos_host, sizeof(pos_host));
  limits.keep();
  Buf table("table", tg_summary_table_bytes(n));
  int32_t blocks = 0;
  for (int k = 0; k < n; ++k)
    ok(tg_summary_table_fill(jobs[k].buf->p, jobs[k].dtype, jobs[k].rows, jobs[k].valid, jobs[k].stride, k, k, table.p, &blocks),
       "tg_summary_table_fill");
  table.keep();
  const size_t ws_bytes = tg_summary_workspace_bytes(blocks);
  if (blocks < n || ws_bytes == 0) throw Fail{"no blocks or no workspace for a table with jobs"};
  Buf ws("workspace", ws_bytes);
  Buf stats("stats", (size_t)n * sizeof(TgSummaryStats));
  Buf buckets("buckets", (size_t)n * TG_SUMMARY_BUCKETS * sizeof(uint32_t));
  Buf sdev("scale_dev", sizeof(float));
  const float dev = 0.25f;
  memcpy(sdev.p, &dev, 4);
  sdev.keep();
  ok(tg_summary_multi(table.p, n, blocks, n, scale, dev_scale ? (const float*)sdev.p : nullptr, (const float*)limits.p,
                      (TgSummaryStats*)stats.p, (uint32_t*)buckets.p, ws.p, ws_bytes, nullptr),
     "tg_summary_multi");
  table.check_same("the table");
  limits.check_same("limits_dev");
  sdev.check_same("scale_dev");
  for (int k = 0; k < n; ++k) {
    jobs[k].buf->check_front("the tensor");
    jobs[k].buf->check_same("the tensor");
    TgSummaryStats got;
    memcpy(&got, stats.p + (size_t)k * sizeof(got), sizeof(got));
    double sum = 0, sumsq = 0;
    float mn = FLT_MAX, mx = -FLT_MAX;
    uint32_t num = 0, zeros = 0;
    for (float x : jobs[k].vals) {
      const float v = x * scale * (dev_scale ? dev : 1.0f);      // powers of two: exact in any order
      ++num;
      zeros += v == 0.f;
      mn = fminf(mn, v);
      mx = fmaxf(mx, v);
      sum += v;
      sumsq += (double)v * v;
    }
    const std::string who = "job " + std::to_string(k);
    if (got.num != num || got.zeros != zeros || got.nonfinite != 0) throw Fail{who + ": counts differ (padding read, or elements missed)"};
    if (got.min != mn || got.max != mx) throw Fail{who + ": minimum or maximum differs"};
    if (got.sum != sum || got.sum_squares != sumsq) throw Fail{who + ": sums differ (every term is a multiple of 2^-10: exact in any order)"};
    uint64_t total = 0;
    for (int b = 0; b < TG_SUMMARY_BUCKETS; ++b) {
      uint32_t c;
      memcpy(&c, buckets.p + ((size_t)k * TG_SUMMARY_BUCKETS + b) * 4, 4);
      total += c;
    }
    if (total != num) throw Fail{who + ": the buckets do not add up to num"};
  }
  for (Job& j : jobs) delete j.buf;
}

unsigned char ref_byte(float x) {
  const float f = x * 255.0f;
  if (!(f > 0.f)) return 0;
  return f >= 255.f ? 255 : (unsigned char)(int)f;
}

void run_grid(const Case& cs) {
  const int h = 4, w = 4, c = cs.mode, rows = cs.rows, cols = cs.cols;
  // 3x2: column 0 holds 3 images, column 1 two (its third cell stays empty); 1x1: one image
  const int counts[2] = {rows, rows > 1 ? rows - 1 : 1};
  Buf* src[2] = {nullptr, nullptr};
  std::vector<float> vals[2];
  Buf table("table", tg_image_grid_table_bytes(cols));
  for (int k = 0; k < cols; ++k) {
    const size_t n = (size_t)counts[k] * h * w * c;
    src[k] = new Buf("images", n * esize(cs.dtype));
    for (size_t i = 0; i < n; ++i) {
      const float v = draw() / 6.0f;      // about [-1.3, 1.3]: both clip sides
      float kept = v;
      if (cs.dtype == TG_BF16) {
        uint32_t b;
        memcpy(&b, &v, 4);
        b &= 0xffff0000u;
        memcpy(&kept, &b, 4);
      } else if (cs.dtype == TG_F16) {
        kept = (float)(_Float16)v;
      }
      vals[k].push_back(kept);
      put(src[k]->p, cs.dtype, i, kept);
    }
    src[k]->keep();
    ok(tg_image_grid_table_fill(src[k]->p, cs.dtype, counts[k], c, k, k, table.p), "tg_image_grid_table_fill");
  }
  table.keep();
  Buf grid("grid", (size_t)rows * h * cols * w * 3);
  ok(tg_image_grid_u8(table.p, cols, rows, cols, h, w, grid.p, nullptr), "tg_image_grid_u8");
  table.check_same("the table");
  for (int k = 0; k < cols; ++k) src[k]->check_same("the images");
  for (int y = 0; y < rows * h; ++y)
    for (int x = 0; x < cols * w; ++x)
      for (int ch = 0; ch < 3; ++ch) {
        const int r = y / h, k = x / w;
        unsigned char want = 0;
        if (r < counts[k]) want = ref_byte(vals[k][(((size_t)r * h + y % h) * w + x % w) * c + (c == 3 ? ch : 0)]);
        if (grid.p[((size_t)y * cols * w + x) * 3 + ch] != want)
          throw Fail{"grid byte (" + std::to_string(y) + ", " + std::to_string(x) + ", " + std::to_string(ch) + ") differs"};
      }
  for (int k = 0; k < cols; ++k) delete src[k];
}

void run_case(const Case& cs) {
  if (cs.kind == 0) {
    std::vector<Job> jobs{make_job(cs.dtype, 1, cs.numel, cs.numel, cs.off)};
    run_summary(jobs, (cs.mode & 1) ? 1.0f / 128.0f : 1.0f, (cs.mode & 2) != 0);
  } else if (cs.kind == 1) {
    std::vector<Job> jobs{make_job(cs.dtype, 9, 15, 20, cs.off)};
    run_summary(jobs, 1.0f, false);
  } else if (cs.kind == 2) {
    std::vector<Job> jobs{make_job(TG_F32, 1, 3, 3, 0), make_job(TG_BF16, 1, 20000, 20000, 1), make_job(TG_F16, 9, 15, 20, 0),
                          make_job(TG_F32, 1, 16385, 16385, 1), make_job(TG_F32, 3, 255, 257, 0)};
    run_summary(jobs, 0.5f, true);
  } else if (cs.kind == 3) {
    run_grid(cs);
  } else if (cs.kind == 4) {
    Buf lim("limits", TG_SUMMARY_BUCKETS * sizeof(double)), pos("pos_limits_f32", TG_SUMMARY_POS_LIMITS * sizeof(float));
    ok(tg_summary_limits((double*)lim.p, (float*)pos.p), "tg_summary_limits");
    double d[TG_SUMMARY_BUCKETS];
    memcpy(d, lim.p, sizeof(d));
    for (int i = 1; i < TG_SUMMARY_BUCKETS; ++i)
      if (!(d[i] > d[i - 1])) throw Fail{"the limits do not ascend at " + std::to_string(i)};
    if (d[TG_SUMMARY_POS_LIMITS + 1] != 0.0 || d[TG_SUMMARY_POS_LIMITS + 2] != 1e-12) throw Fail{"0.0 and 1e-12 are not where they belong"};
  } else if (cs.kind == 5) {
    Buf table("table", tg_summary_table_bytes(3));
    Buf x("tensor", 64);
    int32_t blocks = 0;
    for (int k = 0; k < 3; ++k) ok(tg_summary_table_fill(x.p, TG_F32, 1, 16, 16, k, k, table.p, &blocks), "tg_summary_table_fill");
    if (blocks != 3 || tg_summary_workspace_bytes(blocks) == 0) throw Fail{"three one-block jobs did not give three blocks"};
    if (tg_summary_table_fill(x.p, TG_F32, 1ll << 16, 1ll << 16, 1ll << 16, 0, 0, table.p, &blocks) == 0)
      throw Fail{"a job of 2^32 elements was accepted"};
    if (tg_summary_table_fill(x.p, TG_F32, 2, 16, 8, 0, 0, table.p, &blocks) == 0) throw Fail{"row_stride < row_valid was accepted"};
  } else {
    Buf table("table", tg_image_grid_table_bytes(2));
    Buf x("images", 48);
    for (int k = 0; k < 2; ++k) ok(tg_image_grid_table_fill(x.p, TG_BF16, 1, 3, k, k, table.p), "tg_image_grid_table_fill");
    if (tg_image_grid_table_fill(x.p, TG_BF16, 1, 2, 0, 0, table.p) == 0) throw Fail{"c = 2 was accepted"};
  }
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
          run_case(c);
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
  fprintf(stderr, "usage: summary_bounds --list | summary_bounds --case NAME\n");
  return 2;
}
