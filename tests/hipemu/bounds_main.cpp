// bounds: a stand-alone AddressSanitizer driver over the emulated kernels (TEST INFRASTRUCTURE, built by build.py
// build_bounds(), run by tests/test_bounds_cpu.py as child processes; nothing loads it into python).
//
//   bounds --list          the case names, one per line
//   bounds --case NAME     runs one case: exit 0, or non-zero with a one-line reason on stderr
//
// Every device pointer a case hands to the library is a heap allocation of its own of EXACTLY the byte size
// include/twingan_hip.h documents, so the sanitizer's redzone begins at the first byte the kernel must not touch (each
// allocation asserts that: last byte addressable, next byte poisoned).  After rc == 0 a case checks that its inputs are
// byte-equal to a copy, that no element of a fully written output still holds the pre-fill (0xFF bytes in the first run,
// 0x00 in the second; an element must hold the fill in BOTH to count) and that float outputs are finite.  Values are not
// checked here: the element-wise tests do that.  bounds_cases.inc holds the case table.
#if !defined(__has_feature)
#error "bounds_main.cpp needs clang's __has_feature"
#elif !__has_feature(address_sanitizer)
#error "bounds_main.cpp is only meaningful under -fsanitize=address"
#endif
#include <sanitizer/asan_interface.h>

#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <functional>
#include <string>
#include <vector>

#include "../../include/twingan_hip.h"

namespace {

enum Role { IN, OUT, INOUT, SCRATCH };
// element kinds: the three storage types keep the header's numbers
enum Kind { F32 = TG_F32, BF16 = TG_BF16, F16 = TG_F16, I32 = 8, U8 = 9, I64 = 10 };

size_t esize(int kind) { return kind == F32 || kind == I32 ? 4 : kind == I64 ? 8 : kind == U8 ? 1 : 2; }

uint16_t to_f16(float f) {      // exact for the driver's values (small dyadic rationals); rounds to nearest even otherwise
  uint32_t u;
  memcpy(&u, &f, 4);
  const uint32_t sign = (u >> 16) & 0x8000u;
  const int e = (int)((u >> 23) & 0xff) - 127 + 15;
  uint32_t m = u & 0x7fffffu;
  if (((u >> 23) & 0xff) == 0xff) return (uint16_t)(sign | 0x7c00u | (m ? 0x200u : 0));
  if (e >= 31) return (uint16_t)(sign | 0x7c00u);
  if (e <= 0) {
    if (e < -10) return (uint16_t)sign;
    m |= 0x800000u;
    const int sh = 14 - e;
    uint32_t r = m >> sh;
    const uint32_t rem = m & ((1u << sh) - 1), half = 1u << (sh - 1);
    if (rem > half || (rem == half && (r & 1))) ++r;
    return (uint16_t)(sign | r);
  }
  uint32_t r = ((uint32_t)e << 10) | (m >> 13);
  const uint32_t rem = m & 0x1fffu;
  if (rem > 0x1000u || (rem == 0x1000u && (r & 1))) ++r;
  return (uint16_t)(sign | r);
}

uint16_t to_bf16(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  u += 0x7fffu + ((u >> 16) & 1);
  return (uint16_t)(u >> 16);
}

bool finite_elem(const unsigned char* p, int kind) {
  if (kind == F32) {
    uint32_t u;
    memcpy(&u, p, 4);
    return (u & 0x7f800000u) != 0x7f800000u;
  }
  if (kind != BF16 && kind != F16) return true;
  uint16_t h;
  memcpy(&h, p, 2);
  if (kind == BF16) return (h & 0x7f80u) != 0x7f80u;
  if (kind == F16) return (h & 0x7c00u) != 0x7c00u;
  return true;
}

struct Buf {
  std::string name;
  unsigned char* p = nullptr;
  size_t bytes = 0;
  Role role = IN;
  int kind = F32;
  bool finite = true;
  std::vector<unsigned char> before;
};

struct Fail {
  std::string why;
};

struct Ctx {
  unsigned char fill = 0xFF;
  uint64_t rng = 0x9E3779B97F4A7C15ull;
  std::vector<Buf> bufs;
  bool frozen = false;
  std::vector<std::string> kernels;

  ~Ctx() {
    for (Buf& b : bufs) free(b.p);
  }
  uint32_t next() {
    rng = rng * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng >> 33);
  }
  float val() { return ((int)(next() % 17) - 8) / 8.0f; }      // small integers scaled to about unit size

  void* alloc(const char* name, size_t n, int kind, Role role, bool finite = true) {
    Buf b;
    b.name = name;
    b.bytes = n * esize(kind);
    b.role = role;
    b.kind = kind;
    b.finite = finite;
    if (b.bytes == 0) throw Fail{std::string(name) + ": empty buffer in the case table"};
    void* p = nullptr;
    if (posix_memalign(&p, 256, b.bytes)) throw Fail{"out of memory"};
    b.p = (unsigned char*)p;
    // the sanitizer is live and the redzone starts exactly where the documented size ends
    if (__asan_address_is_poisoned(b.p + b.bytes - 1) || !__asan_address_is_poisoned(b.p + b.bytes) ||
        !__asan_address_is_poisoned(b.p - 1))
      throw Fail{std::string(name) + ": the sanitizer's redzone does not begin at the end of the buffer"};
    memset(b.p, fill, b.bytes);
    bufs.push_back(b);
    return p;
  }
  void put(void* p, size_t i, int kind, float v) {
    if (kind == F32) ((float*)p)[i] = v;
    else if (kind == BF16) ((uint16_t*)p)[i] = to_bf16(v);
    else if (kind == F16) ((uint16_t*)p)[i] = to_f16(v);
    else if (kind == I32) ((int32_t*)p)[i] = (int32_t)v;
    else if (kind == I64) ((int64_t*)p)[i] = (int64_t)v;
    else ((unsigned char*)p)[i] = (unsigned char)v;
  }
  // inputs: seeded values; pos: strictly positive (scales, variances); u8: random bytes
  void* in(const char* name, size_t n, int kind, Role role = IN) {
    void* p = alloc(name, n, kind, role);
    for (size_t i = 0; i < n; ++i) put(p, i, kind, kind == U8 ? (float)(next() & 255) : val());
    return p;
  }
  void* in_pos(const char* name, size_t n, int kind, Role role = IN) {
    void* p = alloc(name, n, kind, role);
    for (size_t i = 0; i < n; ++i) put(p, i, kind, 0.5f + (next() % 9) / 8.0f);
    return p;
  }
  void* in_const(const char* name, size_t n, int kind, float v, Role role = IN) {
    void* p = alloc(name, n, kind, role);
    for (size_t i = 0; i < n; ++i) put(p, i, kind, v);
    return p;
  }
  void* in_bytes(const char* name, const void* src, size_t bytes, Role role = IN) {
    void* p = alloc(name, bytes, U8, role);
    memcpy(p, src, bytes);
    return p;
  }
  void* inout(const char* name, size_t n, int kind) { return in(name, n, kind, INOUT); }
  void* out(const char* name, size_t n, int kind, bool finite = true) { return alloc(name, n, kind, OUT, finite); }
  void* scratch(const char* name, size_t bytes) { return bytes ? alloc(name, bytes, U8, SCRATCH) : nullptr; }

  // right before the call under test (after any preparing calls): inputs are copied, outputs and scratch take the fill
  void go() {
    for (Buf& b : bufs) {
      if (b.role == IN) b.before.assign(b.p, b.p + b.bytes);
      if (b.role == OUT || b.role == SCRATCH) memset(b.p, fill, b.bytes);
    }
    frozen = true;
  }
  void kernel() {
    const char* k = tg_last_kernel();
    kernels.push_back(k ? k : "");
  }
};

void need(int rc, const char* what) {
  if (rc != 0) throw Fail{std::string(what) + ": rc " + std::to_string(rc) + " (" + tg_last_error() + ")"};
}

struct Case {
  std::string name;
  std::function<void(Ctx&)> fn;
};
std::vector<Case> cases;
void add(const std::string& name, std::function<void(Ctx&)> fn) { cases.push_back(Case{name, fn}); }

const char* dname(int dt) { return dt == TG_F32 ? "f32" : dt == TG_BF16 ? "bf16" : "f16"; }

#include "bounds_cases.inc"

int run(const Case& cs) {
  std::vector<std::vector<bool>> held;      // per buffer, per element: still the fill after the first run
  for (int pass = 0; pass < 2; ++pass) {
    Ctx c;
    c.fill = pass ? 0x00 : 0xFF;
    try {
      cs.fn(c);
    } catch (const Fail& f) {
      fprintf(stderr, "FAIL %s: %s\n", cs.name.c_str(), f.why.c_str());
      return 1;
    }
    if (!c.frozen) {
      fprintf(stderr, "FAIL %s: the case never reached its call\n", cs.name.c_str());
      return 1;
    }
    if (pass == 0)
      for (const std::string& k : c.kernels) printf("kernel: %s\n", k.c_str());
    for (size_t bi = 0; bi < c.bufs.size(); ++bi) {
      const Buf& b = c.bufs[bi];
      if (b.role == IN && memcmp(b.p, b.before.data(), b.bytes) != 0) {
        size_t at = 0;
        while (b.p[at] == b.before[at]) ++at;
        fprintf(stderr, "FAIL %s: input %s was written (first at byte %zu of %zu)\n", cs.name.c_str(), b.name.c_str(), at, b.bytes);
        return 1;
      }
      if (b.role != OUT) continue;
      const size_t es = esize(b.kind), n = b.bytes / es;
      if (pass == 0) held.resize(c.bufs.size());
      std::vector<bool>& h = held[bi];
      if (pass == 0) h.assign(n, false);
      for (size_t i = 0; i < n; ++i) {
        bool is_fill = true;
        for (size_t k = 0; k < es; ++k) is_fill = is_fill && b.p[i * es + k] == c.fill;
        if (pass == 0) h[i] = is_fill;
        else if (is_fill && h[i]) {
          fprintf(stderr, "FAIL %s: output %s still holds the fill at element %zu of %zu (never written)\n", cs.name.c_str(),
                  b.name.c_str(), i, n);
          return 1;
        }
        if (b.finite && !is_fill && !finite_elem(b.p + i * es, b.kind)) {
          fprintf(stderr, "FAIL %s: output %s is not finite at element %zu of %zu\n", cs.name.c_str(), b.name.c_str(), i, n);
          return 1;
        }
      }
    }
  }
  printf("ok %s\n", cs.name.c_str());
  return 0;
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
      if (c.name == argv[2]) return run(c);
    fprintf(stderr, "FAIL %s: no such case\n", argv[2]);
    return 2;
  }
  fprintf(stderr, "usage: bounds --list | bounds --case NAME\n");
  return 2;
}
