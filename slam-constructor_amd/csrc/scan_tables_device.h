// scan_tables_device.h -- a scanner's per-beam tables resident in HBM.  Part of slamhip_internal.h (behind hip_block.h).
#pragma once

#include <vector>

#include "hip_block.h"
#include "scan_filter.h"

namespace slamhip {

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
