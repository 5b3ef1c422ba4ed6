// optim_bounds: bounds_main.cpp's sibling for include/twingan_hip_optim.h (TEST INFRASTRUCTURE, built and run by
// tests/test_optimizers_cpu.py as child processes; nothing loads it into python).  Linked with the AddressSanitizer objects of
// the emulated kernels that build.py build_bounds() leaves under _build_asan/ (all but bounds_main.o).
//
//   optim_bounds --list          the case names, one per line
//   optim_bounds --case NAME     runs one case: exit 0 and "ok NAME", or non-zero with a one-line reason on stderr
//
// A case is rule x {plain, ema, skip, apply} x numel x {a, o}: tg_optim_step plain, with the moving average, guarded with skip
// set and guarded with skip clear (both with the average).  Every array is a heap allocation of its own whose LAST byte is the
// last byte of its numel floats, so the sanitizer's redzone begins where the kernel must stop; `o` cases start every array one
// float into its allocation (4-byte aligned only: the element-by-element kernels), and that float must keep its fill.  Slot
// pointers the rule lacks are null.  After rc == 0: the gradient, the guard's state, the weight and the hyper-parameters are
// untouched; theta, the slots and the average are finite; an apply has rewritten EVERY element of theta, of the rule's slots
// and of the average (the inputs are chosen so that each one changes: what "no pre-fill left" is for buffers updated in
// place); a skipped apply has left theta and the slots byte-equal and rewritten every element of the average.
#if !defined(__has_feature)
#error "optim_bounds_main.cpp needs clang's __has_feature"
#elif !__has_feature(address_sanitizer)
#error "optim_bounds_main.cpp is only meaningful under -fsanitize=address"
#endif
#include <sanitizer/asan_interface.h>

#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/twingan_hip_optim.h"

namespace {

struct Fail {
  std::string why;
};

const float FILL = -77.0f;

struct Arr {
  std::string name;
  float* base = nullptr;      // the allocation
  float* p = nullptr;         // what the library gets: base + off
  size_t n = 0;
  int off = 0;
  std::vector<float> before;
};

struct Ctx {
  uint64_t rng = 0x9E3779B97F4A7C15ull;
  std::vector<Arr*> all;
  ~Ctx() {
    for (Arr* a : all) {
      free(a->base);
      delete a;
    }
  }
  uint32_t next() {
    rng = rng * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng >> 33);
  }
  // magnitudes 1/8 .. 7/8 with a random sign: never 0, never 1 (rmsprop's mean square starts at 1 and must move)
  float val() { return (float)(1 + next() % 7) / 8.0f * ((next() & 1) ? 1.f : -1.f); }

  Arr* arr(const char* name, size_t n, int off) {
    Arr* a = new Arr;
    all.push_back(a);
    a->name = name;
    a->n = n;
    a->off = off;
    void* p = nullptr;
    const size_t bytes = (n + off) * sizeof(float);
    if (posix_memalign(&p, 16, bytes)) throw Fail{"out of memory"};
    a->base = (float*)p;
    a->p = a->base + off;
    unsigned char* end = (unsigned char*)p + bytes;
    if (__asan_address_is_poisoned(end - 1) || !__asan_address_is_poisoned(end))
      throw Fail{std::string(name) + ": the sanitizer's redzone does not begin at the end of the buffer"};
    for (int i = 0; i < off; ++i) a->base[i] = FILL;
    return a;
  }
  void keep(Arr* a) { a->before.assign(a->p, a->p + a->n); }
};

const char* RULE_NAMES[] = {"sgd", "momentum", "adagrad", "rmsprop", "adadelta", "ftrl"};
const char* MODES[] = {"plain", "ema", "skip", "apply"};
const int NUMELS[] = {1, 1027};

struct Case {
  std::string name;
  int rule, mode, numel, off;
};
std::vector<Case> cases;

void register_cases() {
  for (int rule = TG_OPT_SGD; rule <= TG_OPT_FTRL; ++rule)
    for (int mode = 0; mode < 4; ++mode)
      for (int numel : NUMELS)
        for (int off = 0; off < 2; ++off)
          cases.push_back(Case{std::string("tg_optim_step_") + RULE_NAMES[rule] + "_" + MODES[mode] + "_n" + std::to_string(numel) +
                                   (off ? "_o" : "_a"),
                               rule, mode, numel, off});
}

void check_front(const Arr* a) {
  for (int i = 0; i < a->off; ++i)
    if (a->base[i] != FILL) throw Fail{a->name + ": the float in front of the array was written"};
}
void check_same(const Arr* a, const char* why) {
  if (memcmp(a->p, a->before.data(), a->n * sizeof(float)) != 0) throw Fail{a->name + " was written (" + why + ")"};
}
void check_rewritten(const Arr* a) {
  for (size_t i = 0; i < a->n; ++i) {
    if (!isfinite(a->p[i])) throw Fail{a->name + " is not finite at element " + std::to_string(i)};
    if (a->p[i] == a->before[i]) throw Fail{a->name + " still holds its old value at element " + std::to_string(i) + " (never written)"};
  }
}

void run_case(const Case& cs) {
  Ctx c;
  const size_t n = (size_t)cs.numel;
  const int ns = tg_optim_slot_count(cs.rule);
  if (ns < 0) throw Fail{"tg_optim_slot_count refused a rule of the header"};
  const bool ema = cs.mode != 0, guarded = cs.mode >= 2, skip = cs.mode == 2;
  Arr* th = c.arr("theta", n, cs.off);
  Arr* g = c.arr("grad", n, cs.off);
  Arr* slot[2] = {nullptr, nullptr};
  for (int s = 0; s < ns; ++s) slot[s] = c.arr(s ? "slot1" : "slot0", n, cs.off);
  Arr* avg = ema ? c.arr("avg", n, cs.off) : nullptr;
  Arr* w = ema ? c.arr("w_dev", 1, 0) : nullptr;
  const float init0 = cs.rule == TG_OPT_RMSPROP ? 1.0f : (cs.rule == TG_OPT_ADAGRAD || cs.rule == TG_OPT_FTRL) ? 0.1f : 0.0f;
  for (size_t i = 0; i < n; ++i) {
    th->p[i] = c.val();
    g->p[i] = c.val() * (guarded ? 4.0f : 1.0f);      // the guarded forms unscale by 1 / 4
    if (slot[0]) slot[0]->p[i] = init0;
    if (slot[1]) slot[1]->p[i] = 0.0f;
    if (avg) avg->p[i] = 10.0f + c.val();
  }
  if (w) w->p[0] = 0.25f;
  // the guard's state, in a heap buffer of exactly its size
  TgLossScaleState* state = nullptr;
  TgLossScaleState state_before;
  if (guarded) {
    if (tg_loss_scale_state_bytes() != sizeof(TgLossScaleState)) throw Fail{"tg_loss_scale_state_bytes disagrees with the header"};
    state = (TgLossScaleState*)malloc(sizeof(TgLossScaleState));
    memset(state, 0, sizeof(*state));
    state->scale = 4.0f;
    state->seed = 4.0f;
    state->inv_scale = 0.25f;
    state->skip = skip ? 1 : 0;
    state_before = *state;
  }
  TgOptimHyper* hyper = (TgOptimHyper*)malloc(sizeof(TgOptimHyper));
  *hyper = TgOptimHyper{0.5f, 0.9f, 0.9f, 1e-8f, -0.5f, 0.0f, 0.0f};
  const TgOptimHyper hyper_before = *hyper;
  for (Arr* a : c.all) c.keep(a);
  // without the guard the scale goes by value; with it the by-value scale is poison that must not be used
  const int rc = tg_optim_step(cs.rule, th->p, g->p, slot[0] ? slot[0]->p : nullptr, slot[1] ? slot[1]->p : nullptr,
                               avg ? avg->p : nullptr, (int64_t)n, hyper, guarded ? NAN : 1.0f, state, w ? w->p : nullptr, nullptr);
  std::string err;
  if (rc != 0) err = std::string("rc ") + std::to_string(rc) + " (" + tg_last_error() + ")";
  try {
    if (rc != 0) throw Fail{err};
    if (memcmp(hyper, &hyper_before, sizeof(hyper_before)) != 0) throw Fail{"hyper was written"};
    if (state && memcmp(state, &state_before, sizeof(state_before)) != 0) throw Fail{"the guard's state was written"};
    for (Arr* a : c.all) check_front(a);
    check_same(g, "an input");
    if (w) check_same(w, "an input");
    if (skip) {
      check_same(th, "a skipped apply");
      for (int s = 0; s < ns; ++s) check_same(slot[s], "a skipped apply");
    } else {
      check_rewritten(th);
      for (int s = 0; s < ns; ++s) check_rewritten(slot[s]);
    }
    if (avg) check_rewritten(avg);
  } catch (...) {
    free(state);
    free(hyper);
    throw;
  }
  free(state);
  free(hyper);
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
  fprintf(stderr, "usage: optim_bounds --list | optim_bounds --case NAME\n");
  return 2;
}
