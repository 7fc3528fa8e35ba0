// The owners of raytracing_c_amd/csrc/rt_mem.h (DevMem, PinnedMem, DevEvent) against the stand-in runtime of tests/c/hip_stub:
// what grow / reset / move / struct assignment call, in which order, and that the byte counter is exact.  Built with
// AddressSanitizer and UndefinedBehaviorSanitizer and run by tests/test_mem_owner.py; needs no GPU and no ROCm.
#include "../../raytracing_c_amd/csrc/rt_mem.h"

#include <utility>
#include <vector>

using namespace hip_stub;

static int g_checks = 0;
#define CHECK(cond)                                                                  \
  do {                                                                               \
    g_checks++;                                                                      \
    if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); exit(1); } \
  } while (0)
// the library's counter equals the stand-in's own sum of live device bytes: checked after every step
#define COUNTER_EXACT() CHECK(g_device_bytes_live.load() == live_bytes(DEVICE))

template <typename M>
static void memory_owner(Kind kind, const char *name) {
  const size_t live0 = live.size();
  {
    M m;
    CHECK(m.get() == nullptr && m.cap == 0 && m.bytes() == 0);
    // a first block; an equal or smaller request keeps it and makes no call
    CHECK(m.grow(100) == hipSuccess && m.get() != nullptr && m.cap == 100);
    CHECK(live.at(m.get()).kind == kind && live.at(m.get()).bytes == 100 * sizeof(*m.get()) && m.bytes() == live.at(m.get()).bytes);
    COUNTER_EXACT();
    auto *p0 = m.get();
    long calls0 = calls;
    CHECK(m.grow(100) == hipSuccess && m.grow(7) == hipSuccess && m.grow(0) == hipSuccess);
    CHECK(m.get() == p0 && m.cap == 100 && calls == calls0);
    CHECK((decltype(p0))m == p0);                                      // the conversion callers pass to HIP and to launchers
    // a larger request frees before it allocates: between the two calls nothing of this owner is live.  The stand-in's failure
    // switch shows it -- the allocation that fails comes after the free, and leaves the live count BELOW what it was
    const size_t before = live.size();
    fail_in = 1;
    CHECK(m.grow(200) != hipSuccess);
    CHECK(m.get() == nullptr && m.cap == 0 && m.bytes() == 0);         // empty after a failed allocation ...
    CHECK(live.size() == before - 1);
    COUNTER_EXACT();
    CHECK(m.grow(200) == hipSuccess && m.get() != nullptr && m.cap == 200);      // ... and the next call tries again
    CHECK(live.size() == before);                                      // never more than before the call: one block, the new one
    COUNTER_EXACT();
    calls0 = calls;
    CHECK(m.grow(300) == hipSuccess && m.cap == 300 && calls == calls0 + 2 && live.size() == before);      // one free, one allocation
    COUNTER_EXACT();
    // a request for no element still yields a pointer: 16 bytes
    M z;
    CHECK(z.grow(0) == hipSuccess && z.get() != nullptr && z.cap == 0 && live.at(z.get()).bytes == 16 && z.bytes() == 16);
    M small;
    CHECK(small.grow(1) == hipSuccess && live.at(small.get()).bytes == (sizeof(*small.get()) > 16 ? sizeof(*small.get()) : 16));
    COUNTER_EXACT();
    calls0 = calls;
    CHECK(z.grow(0) == hipSuccess && calls == calls0);                 // (and keeps it)
    // move construction: the source is empty, nothing is freed
    auto *p1 = m.get();
    calls0 = calls;
    M n(std::move(m));
    CHECK(m.get() == nullptr && m.cap == 0 && n.get() == p1 && n.cap == 300 && calls == calls0);
    // move assignment: the target's old block is freed exactly once (the stand-in aborts on a second time), the source is empty
    auto *pz = z.get();
    z = std::move(n);
    CHECK(n.get() == nullptr && n.cap == 0 && z.get() == p1 && z.cap == 300 && live.count(pz) == 0 && calls == calls0 + 1);
    z = std::move(z);                                                  // (onto itself: nothing happens)
    CHECK(z.get() == p1 && live.count(p1) == 1);
    COUNTER_EXACT();
    // reset, twice
    z.reset();
    CHECK(z.get() == nullptr && z.cap == 0 && live.count(p1) == 0);
    calls0 = calls;
    z.reset();
    CHECK(calls == calls0);
    COUNTER_EXACT();
    // a vector of owners that reallocates moves them
    std::vector<M> v;
    for (int i = 0; i < 9; i++) { v.emplace_back(); CHECK(v.back().grow((size_t)i + 1) == hipSuccess); }
    CHECK(live_count(kind) == 9 + 1);                                  // (+ `small`)
    v.erase(v.begin() + 3);
    CHECK(live_count(kind) == 8 + 1);
    COUNTER_EXACT();
  }                                                                    // the destructors free the rest
  CHECK(live.size() == live0);
  COUNTER_EXACT();
  printf("%s ok\n", name);
}

static void event_owner() {
  {
    DevEvent e;
    CHECK((hipEvent_t)e == nullptr);
    fail_in = 1;
    CHECK(e.ensure() != hipSuccess && (hipEvent_t)e == nullptr);      // a failed creation leaves it empty; the next call tries again
    CHECK(e.ensure(hipEventDisableTiming) == hipSuccess && (hipEvent_t)e != nullptr && live_count(EVENT) == 1);
    hipEvent_t h = e;
    long calls0 = calls;
    CHECK(e.ensure() == hipSuccess && (hipEvent_t)e == h && calls == calls0);      // created once
    DevEvent f(std::move(e));
    CHECK((hipEvent_t)e == nullptr && (hipEvent_t)f == h && calls == calls0);
    DevEvent g;
    CHECK(g.ensure() == hipSuccess);
    hipEvent_t old = g;
    g = std::move(f);
    CHECK((hipEvent_t)f == nullptr && (hipEvent_t)g == h && live.count(old) == 0 && live_count(EVENT) == 1);
    g.reset();
    g.reset();
    CHECK((hipEvent_t)g == nullptr && live_count(EVENT) == 0);
    std::vector<DevEvent> v;
    for (int i = 0; i < 5; i++) { v.emplace_back(); CHECK(v.back().ensure() == hipSuccess); }
    CHECK(live_count(EVENT) == 5);
  }
  CHECK(live.empty());
  printf("DevEvent ok\n");
}

// A struct of owners, as the library's per-device states are: assigning a default-constructed one frees every member once.
namespace {
struct State {
  DevMem<unsigned char> slots;
  DevEvent              done[4];
  DevMem<float>         staging[2];
  PinnedMem<int>        host;
  std::vector<DevEvent> timed;
  int                   next = 0;
};
}  // namespace

static void struct_of_owners() {
  State *S = new State();                                              // (on the heap, like the library's device slots)
  CHECK(S->slots.grow(256) == hipSuccess && S->staging[0].grow(10) == hipSuccess && S->staging[1].grow(20) == hipSuccess);
  CHECK(S->host.grow(8) == hipSuccess && S->done[1].ensure() == hipSuccess && S->done[3].ensure() == hipSuccess);
  S->timed.emplace_back();
  CHECK(S->timed[0].ensure() == hipSuccess);
  S->next = 3;
  CHECK(live_count(DEVICE) == 3 && live_count(PINNED) == 1 && live_count(EVENT) == 3);
  CHECK(g_device_bytes_live.load() == 256 + 40 + 80);
  COUNTER_EXACT();
  const long calls0 = calls;
  *S = State();
  CHECK(live.empty() && calls == calls0 + 7 && S->next == 0 && S->slots.get() == nullptr);      // seven resources, seven calls
  COUNTER_EXACT();
  CHECK(S->slots.grow(64) == hipSuccess);                              // usable again
  COUNTER_EXACT();
  delete S;
  CHECK(live.empty());
  printf("struct of owners ok\n");
}

int main() {
  memory_owner<DevMem<float>>(DEVICE, "DevMem");
  memory_owner<DevMem<State *>>(DEVICE, "DevMem of 8-byte elements");
  memory_owner<PinnedMem<unsigned char>>(PINNED, "PinnedMem");
  event_owner();
  struct_of_owners();
  CHECK(live.empty() && g_device_bytes_live.load() == 0);              // nothing is left, and the counter says so
  printf("%d checks\n", g_checks);
  return 0;
}
