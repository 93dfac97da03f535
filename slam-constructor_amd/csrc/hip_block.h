// hip_block.h -- owners of hipMalloc / hipHostMalloc blocks, the one way such a block grows, and a scanner's per-beam
// tables resident in HBM.  Part of slamhip_internal.h, which includes it behind SLAMHIP_CHECK: include that one.
#pragma once

#include <hip/hip_runtime.h>

#include "scan_filter.h"

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

// A block that holds `cap` units of `per` elements and has to hold `need`: nothing, or the stream waited for (what runs
// on it may read the block that goes away) and `floor` doubled up to `need` units allocated in its place.  alloc frees
// first and a failed one leaves the owner empty, so the stored capacity is zero from the free to the success: an error
// return never leaves an old capacity over a null block.
template <class T, bool kPinned, class Cap>
int grow_block(hipStream_t stream, HipBlock<T, kPinned> &block, Cap &cap, size_t need, size_t floor, size_t per = 1,
               unsigned pinned_flags = 0) {
  if (need <= (size_t)cap) return SLAMHIP_OK;
  SLAMHIP_CHECK(hipStreamSynchronize(stream));
  size_t grown = floor;
  while (grown < need) grown *= 2;
  cap = 0;
  SLAMHIP_CHECK(block.alloc(per * grown, pinned_flags));
  cap = (Cap)grown;
  return SLAMHIP_OK;
}

// A scanner's per-beam tables (ScanTables, scan_filter.h) resident in HBM, where the assembly kernels gather them: ONE
// block of `planes` planes of cap() doubles, cos | sin | viny_f [| angle].
class ScanTablesDevice {
  DeviceBuf<double> d_;
  int cap_ = 0, planes_ = 0;
  const double *plane(int q) const { return q < planes_ ? d_.get() + (size_t)q * (size_t)cap_ : nullptr; }

 public:
  // `t` to HBM on `stream`, behind what still reads the tables held so far; 3 planes, or 4 with the angles.  The copies
  // are asynchronous from pageable memory: the caller waits for the stream before `t` may change.
  int upload(hipStream_t stream, const ScanTables &t, int planes) {
    const size_t n = t.cos_a.size(), bytes = sizeof(double) * n;
    if (planes != planes_) cap_ = 0;
    const int rc = grow_block(stream, d_, cap_, n, 2048, planes);
    if (rc) return rc;
    planes_ = planes;
    const std::vector<double> *src[4] = {&t.cos_a, &t.sin_a, &t.viny_f, &t.angle};
    for (int q = 0; q < planes; ++q)
      SLAMHIP_CHECK(hipMemcpyAsync(d_.get() + (size_t)q * (size_t)cap_, src[q]->data(), bytes, hipMemcpyHostToDevice, stream));
    return SLAMHIP_OK;
  }
  size_t cap() const { return (size_t)cap_; }
  const double *cos() const { return plane(0); }
  const double *sin() const { return plane(1); }
  const double *viny() const { return plane(2); }
  const double *angle() const { return plane(3); }  // (null where the block holds three planes)
};

}  // namespace slamhip
