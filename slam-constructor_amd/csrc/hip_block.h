// hip_block.h -- owners of hipMalloc / hipHostMalloc blocks and the one way such blocks grow: the only way the library
// holds a block (the three planes of a DeviceMap, which change hands, excepted).  Needs the runtime header, SLAMHIP_OK
// and SLAMHIP_CHECK and nothing else; slamhip_internal.h includes it behind SLAMHIP_CHECK: include that one.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <initializer_list>

namespace slamhip {

// A hipMalloc / hipHostMalloc block and its owner: freed when the owner goes, so that no error return between an
// allocation and the store of its pointer can leak it.  Move-only; nothing else.
template <class T, bool kPinned>
class HipBlock {
  T *p_ = nullptr;

 public:
  HipBlock() = default;
  HipBlock(const HipBlock &) = delete;
  HipBlock &operator=(const HipBlock &) = delete;
  HipBlock(HipBlock &&o) noexcept : p_(o.p_) { o.p_ = nullptr; }
  HipBlock &operator=(HipBlock &&o) noexcept {
    if (this != &o) {
      reset();
      p_ = o.p_;
      o.p_ = nullptr;
    }
    return *this;
  }
  ~HipBlock() { reset(); }
  T *get() const { return p_; }
  explicit operator bool() const { return p_ != nullptr; }
  void reset() {
    if (p_) {
      if constexpr (kPinned) hipHostFree(p_);
      else hipFree(p_);
    }
    p_ = nullptr;
  }
  // `count` elements in place of what was held (a failed allocation leaves the owner empty)
  hipError_t alloc(size_t count, unsigned pinned_flags = 0) {
    reset();
    if constexpr (kPinned) return hipHostMalloc(&p_, sizeof(T) * count, pinned_flags);
    else return hipMalloc(&p_, sizeof(T) * count);
  }
};
template <class T>
using DeviceBuf = HipBlock<T, false>;
template <class T>
using PinnedBuf = HipBlock<T, true>;
constexpr unsigned kPinnedCoherent = hipHostMallocMapped | hipHostMallocCoherent;

// Blocks that share the capacity `cap` and have to hold `need` units: nothing, or the streams waited for (what runs on
// them may read the blocks that go away), `floor` doubled up to `need`, and `body(grown)` -- the callers' alloc,
// hipMemsetAsync and host memset calls -- run under a stored capacity of zero.  alloc frees first and a failed one
// leaves its owner empty, so an error return never leaves an old capacity over a null block: the capacity is stored
// only behind a body that returned SLAMHIP_OK.
template <class Cap, class Body>
int grow_blocks(std::initializer_list<hipStream_t> streams, Cap &cap, size_t need, size_t floor, Body &&body) {
  if (need <= (size_t)cap) return SLAMHIP_OK;
  for (hipStream_t s : streams) SLAMHIP_CHECK(hipStreamSynchronize(s));
  size_t grown = floor;
  while (grown < need) grown *= 2;
  cap = 0;
  const int rc = body(grown);
  if (rc == SLAMHIP_OK) cap = (Cap)grown;
  return rc;
}

// ... and the lone block of `per` elements a unit
template <class T, bool kPinned, class Cap>
int grow_block(hipStream_t stream, HipBlock<T, kPinned> &block, Cap &cap, size_t need, size_t floor, size_t per = 1,
               unsigned pinned_flags = 0) {
  return grow_blocks({stream}, cap, need, floor, [&](size_t grown) -> int {
    SLAMHIP_CHECK(block.alloc(per * grown, pinned_flags));
    return SLAMHIP_OK;
  });
}

}  // namespace slamhip
