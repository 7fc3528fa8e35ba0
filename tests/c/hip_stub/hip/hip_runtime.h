// Stand-in for <hip/hip_runtime.h>, for tests/c/mem_owner.cpp only: raytracing_c_amd/csrc/rt_mem.h compiles against it unchanged,
// on a machine without ROCm, and its owners then manage plain malloc blocks that AddressSanitizer and LeakSanitizer watch.
//
// What it assumes of the real runtime (all that rt_mem.h uses of it):
//   hipMalloc(void **, size_t), hipHostMalloc(void **, size_t, unsigned)   return hipSuccess and a block, or an error
//   hipFree(void *), hipHostFree(void *)                                   give a block of the matching call back
//   hipEventCreateWithFlags(hipEvent_t *, unsigned), hipEventDestroy(hipEvent_t)
//   hipEventDefault == 0 (so that ensure() equals hipEventCreate), hipHostMallocDefault, hipEventDisableTiming
// What it adds for the test: every live block with its size and kind (hip_stub::live), the number of calls made (hip_stub::calls),
// and a switch that makes the n-th allocation from now fail (hip_stub::fail_in).  Giving back what is not live, or through the
// call of the other kind, aborts.
#pragma once

#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <map>

typedef enum { hipSuccess = 0, hipErrorOutOfMemory = 2 } hipError_t;
typedef struct ihipEvent_t *hipEvent_t;
enum { hipEventDefault = 0u, hipEventDisableTiming = 2u, hipHostMallocDefault = 0u };

namespace hip_stub {
enum Kind { DEVICE, PINNED, EVENT };
struct Block { Kind kind; size_t bytes; };
inline std::map<void *, Block> live;
inline long calls = 0;                   // every stub call, successful or not
inline long fail_in = 0;                 // n > 0: the n-th allocation (memory or event) from now fails, once

inline size_t live_count(Kind k) { size_t n = 0; for (auto &kv : live) n += kv.second.kind == k; return n; }
inline long   live_bytes(Kind k) { long n = 0; for (auto &kv : live) if (kv.second.kind == k) n += (long)kv.second.bytes; return n; }

inline hipError_t take(void **p, size_t bytes, Kind k) {
  calls++;
  if (fail_in > 0 && --fail_in == 0) return hipErrorOutOfMemory;      // (*p is left as it was, like the runtime)
  *p = malloc(bytes ? bytes : 1);
  live[*p] = {k, bytes};
  return hipSuccess;
}
inline hipError_t give(void *p, Kind k) {
  calls++;
  if (!p) return hipSuccess;
  auto it = live.find(p);
  if (it == live.end() || it->second.kind != k) { fprintf(stderr, "hip_stub: %p given back twice or through the wrong call\n", p); abort(); }
  live.erase(it);
  free(p);
  return hipSuccess;
}
}  // namespace hip_stub

inline hipError_t hipMalloc(void **p, size_t bytes) { return hip_stub::take(p, bytes, hip_stub::DEVICE); }
inline hipError_t hipFree(void *p) { return hip_stub::give(p, hip_stub::DEVICE); }
inline hipError_t hipHostMalloc(void **p, size_t bytes, unsigned) { return hip_stub::take(p, bytes, hip_stub::PINNED); }
inline hipError_t hipHostFree(void *p) { return hip_stub::give(p, hip_stub::PINNED); }
inline hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) { return hip_stub::take((void **)e, 8, hip_stub::EVENT); }
inline hipError_t hipEventDestroy(hipEvent_t e) { return hip_stub::give(e, hip_stub::EVENT); }
