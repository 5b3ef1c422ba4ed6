// mmd_bounds: bounds_main.cpp's sibling for include/twingan_hip_mmd.h (TEST INFRASTRUCTURE, built and run by
// tests/test_mmd_cpu.py as child processes; nothing loads it into python).  Linked with the AddressSanitizer objects of the
// emulated kernels that build.py build_bounds() leaves under _build_asan/ (all but bounds_main.o).
//
//   mmd_bounds --list          the case names, one per line
//   mmd_bounds --case NAME     runs one case: exit 0 and "ok NAME", or non-zero with a one-line reason on stderr
//
// Every buffer the entry point reads or writes is a heap allocation of its own whose LAST byte is the last byte of its
// documented size (a [m, d], b [n, d], sums [ceil(m / block), ceil(n / block)] fp64, the workspace of exactly
// tg_mmd_workspace_bytes), so the sanitizer's redzone begins where the code must stop; `o` cases start the operands 2 or 4
// bytes into their allocation (no 16-byte alignment: the scalar staging), and those bytes must keep their fill.  After rc == 0
// the inputs are unchanged and the sums equal a plain host loop (rows in {-1, 0, 1}, gamma = 1 / 4: every value exact).
#if !defined(__has_feature)
#error "mmd_bounds_main.cpp needs clang's __has_feature"
#elif !__has_feature(address_sanitizer)
#error "mmd_bounds_main.cpp is only meaningful under -fsanitize=address"
#endif
#include <sanitizer/asan_interface.h>

#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/twingan_hip_mmd.h"

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
int draw() { return (int)(next_u32() % 3) - 1; }      // -1, 0, 1: exact in the three formats

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
  int kind;      // 0 block sums, 1 the same matrix against itself, 2 refusals / workspace
  int dtype, m, n, d, block, degree, off;
};
std::vector<Case> cases;

void register_cases() {
  const int shapes[][5] = {{1, 1, 1, 32, 1}, {3, 5, 16, 32, 2}, {33, 257, 24, 32, 3}, {70, 300, 27, 64, 4}, {70, 333, 40, 128, 3}};
  for (int dt = 0; dt < 3; ++dt) {
    for (const auto& s : shapes)
      for (int off = 0; off < 2; ++off)
        cases.push_back(Case{std::string("tg_mmd_block_sums_") + DT_NAMES[dt] + "_m" + std::to_string(s[0]) + "_n" + std::to_string(s[1]) + "_d" +
                                 std::to_string(s[2]) + "_b" + std::to_string(s[3]) + "_p" + std::to_string(s[4]) + (off ? "_o" : "_a"),
                             0, dt, s[0], s[1], s[2], s[3], s[4], off});
    cases.push_back(Case{std::string("tg_mmd_block_sums_") + DT_NAMES[dt] + "_self", 1, dt, 131, 131, 43, 64, 3, 0});
  }
  cases.push_back(Case{"tg_mmd_block_sums_refusals", 2, 0, 0, 0, 0, 0, 0, 0});
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

// the header's pair value on integers: s exact, gamma = 1 / 4 and coef0 = 1 make t a multiple of 1 / 4, the powers exact
double pair_value(const Mat& A, int i, const Mat& B, int j, int d, int degree) {
  int s = 0;
  for (int t = 0; t < d; ++t) s += A.v[(size_t)i * d + t] * B.v[(size_t)j * d + t];
  const double t = 0.25 * s + 1.0;
  double p = t;
  for (int k = 1; k < degree; ++k) p *= t;
  return p;
}

void check_sums(const Case& c, const Mat& A, const Mat& B, int64_t a0, int64_t b0, int skip, const Buf& sums) {
  const int nbi = (c.m + c.block - 1) / c.block, nbj = (c.n + c.block - 1) / c.block;
  for (int I = 0; I < nbi; ++I)
    for (int J = 0; J < nbj; ++J) {
      double want = 0, got;
      for (int i = I * c.block; i < c.m && i < (I + 1) * c.block; ++i)
        for (int j = J * c.block; j < c.n && j < (J + 1) * c.block; ++j)
          if (!(skip && a0 + i == b0 + j)) want += pair_value(A, i, B, j, c.d, c.degree);
      memcpy(&got, sums.p + 8 * ((size_t)I * nbj + J), 8);
      if (got != want)
        throw Fail{"block (" + std::to_string(I) + ", " + std::to_string(J) + "): " + std::to_string(got) + " differs from the host loop's " +
                   std::to_string(want)};
    }
}

void run_sums(const Case& c) {
  Mat A = make_mat("a", c.m, c.d, c.dtype, c.off), B = make_mat("b", c.n, c.d, c.dtype, c.off);
  const int nbi = (c.m + c.block - 1) / c.block, nbj = (c.n + c.block - 1) / c.block;
  const size_t need = tg_mmd_workspace_bytes(c.m, c.n, c.d, c.block);
  if (need != 8 * (size_t)((c.m + 31) / 32) * ((c.n + 31) / 32)) throw Fail{"workspace size is not one fp64 per 32 x 32 unit"};
  const int64_t a0 = (1ll << 33) + 2, b0 = 1ll << 33;      // the pairs (i, i + 2) are the same index
  for (int skip = 0; skip < 2; ++skip) {
    Buf sums("sums", (size_t)nbi * nbj * 8), ws("workspace", need);
    ok(tg_mmd_block_sums(A.buf->p, c.m, B.buf->p, c.n, c.d, c.dtype, c.degree, 0.25f, 1.0f, c.block, a0, b0, skip, (double*)sums.p, ws.p,
                         need, nullptr),
       "tg_mmd_block_sums");
    check_sums(c, A, B, a0, b0, skip, sums);
  }
  A.buf->check_front("a");
  A.buf->check_same("a");
  B.buf->check_front("b");
  B.buf->check_same("b");
  delete A.buf;
  delete B.buf;
}

void run_self(const Case& c) {
  Mat A = make_mat("a", c.m, c.d, c.dtype, 0);
  const int nb = (c.m + c.block - 1) / c.block;
  const size_t need = tg_mmd_workspace_bytes(c.m, c.m, c.d, c.block);
  Buf sums("sums", (size_t)nb * nb * 8), ws("workspace", need);
  ok(tg_mmd_block_sums(A.buf->p, c.m, A.buf->p, c.m, c.d, c.dtype, c.degree, 0.25f, 1.0f, c.block, 0, 0, 1, (double*)sums.p, ws.p, need, nullptr),
     "tg_mmd_block_sums");
  check_sums(c, A, A, 0, 0, 1, sums);
  A.buf->check_same("a");
  delete A.buf;
}

void run_refusals() {
  if (tg_mmd_workspace_bytes(1, 1, 1, 32) != 8 || tg_mmd_workspace_bytes(33, 65, 7, 64) != 48) throw Fail{"workspace size"};
  if (tg_mmd_workspace_bytes(0, 1, 1, 32) || tg_mmd_workspace_bytes(1, 0, 1, 32) || tg_mmd_workspace_bytes(1, 1, 0, 32) ||
      tg_mmd_workspace_bytes(1, 1, 1, 0) || tg_mmd_workspace_bytes(1, 1, 1, 48) || tg_mmd_workspace_bytes((1ll << 20) + 1, 1, 1, 32))
    throw Fail{"a refused shape has a workspace size"};
  Buf a("a", 4 * 4), b("b", 4 * 4), sums("sums", 8), ws("workspace", 16);
  memset(a.p, 0, a.bytes);
  memset(b.p, 0, b.bytes);
  double* S = (double*)sums.p;
  int i = 0;
#define REFUSED(TEXT_, CALL_)                                                                                              \
  do {                                                                                                                      \
    ++i;                                                                                                                    \
    if ((CALL_) == 0) throw Fail{std::string("refusal ") + std::to_string(i) + " (" + TEXT_ + ") was accepted"};              \
    if (!strstr(tg_last_error(), TEXT_)) throw Fail{std::string("refusal ") + TEXT_ + " reads: " + tg_last_error()};       \
  } while (0)
  REFUSED("NULL", tg_mmd_block_sums(nullptr, 1, b.p, 1, 4, TG_F32, 3, 1.f, 1.f, 32, 0, 0, 0, S, ws.p, 8, nullptr));
  REFUSED("NULL", tg_mmd_block_sums(a.p, 1, nullptr, 1, 4, TG_F32, 3, 1.f, 1.f, 32, 0, 0, 0, S, ws.p, 8, nullptr));
  REFUSED("NULL", tg_mmd_block_sums(a.p, 1, b.p, 1, 4, TG_F32, 3, 1.f, 1.f, 32, 0, 0, 0, nullptr, ws.p, 8, nullptr));
  REFUSED("NULL", tg_mmd_block_sums(a.p, 1, b.p, 1, 4, TG_F32, 3, 1.f, 1.f, 32, 0, 0, 0, S, nullptr, 8, nullptr));
  REFUSED("m = 0", tg_mmd_block_sums(a.p, 0, b.p, 1, 4, TG_F32, 3, 1.f, 1.f, 32, 0, 0, 0, S, ws.p, 8, nullptr));
  REFUSED("n = -1", tg_mmd_block_sums(a.p, 1, b.p, -1, 4, TG_F32, 3, 1.f, 1.f, 32, 0, 0, 0, S, ws.p, 8, nullptr));
  REFUSED("d = 0", tg_mmd_block_sums(a.p, 1, b.p, 1, 0, TG_F32, 3, 1.f, 1.f, 32, 0, 0, 0, S, ws.p, 8, nullptr));
  REFUSED("dtype 3", tg_mmd_block_sums(a.p, 1, b.p, 1, 4, 3, 3, 1.f, 1.f, 32, 0, 0, 0, S, ws.p, 8, nullptr));
  REFUSED("degree = 0", tg_mmd_block_sums(a.p, 1, b.p, 1, 4, TG_F32, 0, 1.f, 1.f, 32, 0, 0, 0, S, ws.p, 8, nullptr));
  REFUSED("degree = 5", tg_mmd_block_sums(a.p, 1, b.p, 1, 4, TG_F32, 5, 1.f, 1.f, 32, 0, 0, 0, S, ws.p, 8, nullptr));
  REFUSED("block = 16", tg_mmd_block_sums(a.p, 1, b.p, 1, 4, TG_F32, 3, 1.f, 1.f, 16, 0, 0, 0, S, ws.p, 8, nullptr));
  REFUSED("block = 48", tg_mmd_block_sums(a.p, 1, b.p, 1, 4, TG_F32, 3, 1.f, 1.f, 48, 0, 0, 0, S, ws.p, 8, nullptr));
  REFUSED("a_index0", tg_mmd_block_sums(a.p, 1, b.p, 1, 4, TG_F32, 3, 1.f, 1.f, 32, -1, 0, 0, S, ws.p, 8, nullptr));
  REFUSED("b_index0", tg_mmd_block_sums(a.p, 1, b.p, 1, 4, TG_F32, 3, 1.f, 1.f, 32, 0, -1, 0, S, ws.p, 8, nullptr));
  REFUSED("workspace of 7 bytes", tg_mmd_block_sums(a.p, 1, b.p, 1, 4, TG_F32, 3, 1.f, 1.f, 32, 0, 0, 0, S, ws.p, 7, nullptr));
  REFUSED("not 8-byte aligned", tg_mmd_block_sums(a.p, 1, b.p, 1, 4, TG_F32, 3, 1.f, 1.f, 32, 0, 0, 0, S, ws.p + 4, 8, nullptr));
#undef REFUSED
  // a refused call writes nothing; the same call with good arguments, on the last 8 bytes of the workspace, runs
  for (size_t k = 0; k < sums.bytes; ++k)
    if (sums.p[k] != FILL) throw Fail{"a refused call wrote the sums"};
  for (size_t k = 0; k < ws.bytes; ++k)
    if (ws.p[k] != FILL) throw Fail{"a refused call wrote the workspace"};
  ok(tg_mmd_block_sums(a.p, 1, b.p, 1, 4, TG_F32, 3, 1.f, 1.f, 32, 0, 0, 0, S, ws.p + 8, 8, nullptr), "tg_mmd_block_sums");
  if (*S != 1.0) throw Fail{"zero rows: the one pair is coef0 ** 3 = 1"};
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
          if (c.kind == 0) run_sums(c);
          else if (c.kind == 1) run_self(c);
          else run_refusals();
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
  fprintf(stderr, "usage: mmd_bounds --list | mmd_bounds --case NAME\n");
  return 2;
}
