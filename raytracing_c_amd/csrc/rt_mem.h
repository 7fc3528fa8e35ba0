// rt_mem.h -- the owners of what the host side gets from the HIP runtime: device memory (DevMem), pinned host memory (PinnedMem)
// and events (DevEvent).  Move-only; the destructor gives the resource back, so a struct of owners needs no free list: assigning
// a default-constructed struct (S = QueryState()) or deleting it frees every member exactly once.  The owners know nothing of
// devices: whoever grows, resets or destroys one holds the mutex, and has the device current, that the code did before them.
// No owner may have static storage duration (rt_host.h): its destructor would call into a HIP runtime that is gone at exit.
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstddef>
#include <cstdint>

#pragma GCC visibility push(hidden)      // (no weak template symbol of this header joins a library's export list)

// Device bytes the DevMem owners of this library hold right now, on all devices (rt_diag_device_bytes_live): a leak is a number
// that does not come back, whatever the card's other tenants allocate meanwhile.
inline std::atomic<int64_t> g_device_bytes_live{0};

struct DeviceAllocator {
  static hipError_t alloc(void **p, size_t bytes) {
    hipError_t e = hipMalloc(p, bytes);
    if (e == hipSuccess) g_device_bytes_live += (int64_t)bytes;
    return e;
  }
  static void free(void *p, size_t bytes) {
    (void)hipFree(p);
    g_device_bytes_live -= (int64_t)bytes;
  }
};
struct PinnedAllocator {
  static hipError_t alloc(void **p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
  static void free(void *p, size_t) { (void)hipHostFree(p); }
};

template <typename T, typename A>
struct OwnedMem {
  T     *p = nullptr;
  size_t cap = 0;                      // elements

  OwnedMem() = default;
  OwnedMem(const OwnedMem &) = delete;
  OwnedMem &operator=(const OwnedMem &) = delete;
  OwnedMem(OwnedMem &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
  OwnedMem &operator=(OwnedMem &&o) noexcept {
    if (this != &o) {
      reset();
      p = o.p; cap = o.cap;
      o.p = nullptr; o.cap = 0;
    }
    return *this;
  }
  ~OwnedMem() { reset(); }

  size_t bytes() const { return !p ? 0 : (cap * sizeof(T) > 16 ? cap * sizeof(T) : 16); }      // of the block held
  void reset() {
    if (p) A::free(p, bytes());
    p = nullptr;
    cap = 0;
  }
  // Room for `want` elements (at least 16 bytes, so that a request for none still yields a pointer).  A block that is large enough
  // stays: same pointer, no call.  Otherwise the old block is freed BEFORE the new one is allocated -- the peak does not rise, the
  // contents are lost -- and a failed allocation leaves the owner empty, for the next call to try again.
  hipError_t grow(size_t want) {
    if (p && cap >= want) return hipSuccess;
    reset();
    const size_t n = want * sizeof(T) > 16 ? want * sizeof(T) : 16;
    hipError_t e = A::alloc((void **)&p, n);
    if (e != hipSuccess) { p = nullptr; return e; }
    cap = want;
    return hipSuccess;
  }
  T *get() const { return p; }
  operator T *() const { return p; }
};
template <typename T> using DevMem = OwnedMem<T, DeviceAllocator>;
template <typename T> using PinnedMem = OwnedMem<T, PinnedAllocator>;

struct DevEvent {
  hipEvent_t e = nullptr;

  DevEvent() = default;
  DevEvent(const DevEvent &) = delete;
  DevEvent &operator=(const DevEvent &) = delete;
  DevEvent(DevEvent &&o) noexcept : e(o.e) { o.e = nullptr; }
  DevEvent &operator=(DevEvent &&o) noexcept {
    if (this != &o) {
      reset();
      e = o.e;
      o.e = nullptr;
    }
    return *this;
  }
  ~DevEvent() { reset(); }

  void reset() {
    if (e) (void)hipEventDestroy(e);
    e = nullptr;
  }
  hipError_t ensure(unsigned flags = hipEventDefault) { return e ? hipSuccess : hipEventCreateWithFlags(&e, flags); }      // created once
  operator hipEvent_t() const { return e; }
};

#pragma GCC visibility pop
