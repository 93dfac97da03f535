// A stand-in for the HIP runtime's header, for tests/native/hip_block_test.cpp only: the five calls csrc/hip_block.h
// makes, on top of malloc.  It counts the live blocks, the waits for a stream and the allocations, can make the k-th
// allocation from now fail, and aborts on a block freed twice or never handed out.
#pragma once

#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <set>

typedef int hipError_t;
typedef struct hipStubStream *hipStream_t;
constexpr hipError_t hipSuccess = 0, hipErrorOutOfMemory = 2;
constexpr unsigned hipHostMallocMapped = 2, hipHostMallocCoherent = 0x40000000;

namespace hip_stub {
inline std::set<void *> &live_device() {
  static std::set<void *> s;
  return s;
}
inline std::set<void *> &live_pinned() {
  static std::set<void *> s;
  return s;
}
inline long &allocations() {
  static long n = 0;
  return n;
}
inline long &stream_waits() {
  static long n = 0;
  return n;
}
inline unsigned &last_pinned_flags() {
  static unsigned f = 0;
  return f;
}
// > 0: the allocation that many calls from now fails (1 = the next one); 0 = none
inline long &fail_in() {
  static long k = 0;
  return k;
}
inline size_t live() { return live_device().size() + live_pinned().size(); }

inline hipError_t allocate(std::set<void *> &pool, void **p, size_t bytes) {
  ++allocations();
  if (fail_in() > 0 && --fail_in() == 0) {
    *p = nullptr;
    return hipErrorOutOfMemory;
  }
  *p = std::malloc(bytes ? bytes : 1);
  pool.insert(*p);
  return hipSuccess;
}
inline hipError_t release(std::set<void *> &pool, void *p, const char *what) {
  if (!p) return hipSuccess;
  if (pool.erase(p) != 1) {
    std::printf("FAILED %s of a block that is not live (freed twice, or of the other kind)\n", what);
    std::abort();
  }
  std::free(p);
  return hipSuccess;
}
}  // namespace hip_stub

template <class T>
hipError_t hipMalloc(T **p, size_t bytes) {
  return hip_stub::allocate(hip_stub::live_device(), (void **)p, bytes);
}
template <class T>
hipError_t hipHostMalloc(T **p, size_t bytes, unsigned flags) {
  hip_stub::last_pinned_flags() = flags;
  return hip_stub::allocate(hip_stub::live_pinned(), (void **)p, bytes);
}
inline hipError_t hipFree(void *p) { return hip_stub::release(hip_stub::live_device(), p, "hipFree"); }
inline hipError_t hipHostFree(void *p) { return hip_stub::release(hip_stub::live_pinned(), p, "hipHostFree"); }
inline hipError_t hipStreamSynchronize(hipStream_t) {
  ++hip_stub::stream_waits();
  return hipSuccess;
}
