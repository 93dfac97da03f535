// scan_assemble_device.h -- one point of the scan block from the RAW scan's staged arrays and the resident per-beam
// tables (ScanAssembleArgs, slamhip_internal.h).  The ONE statement of that arithmetic: k_scan_assemble
// (score_kernels.hip) writes its five values to the scan block, the lone co-resident hill-climbing chain
// (hc_resident.hip, RAW) keeps them in registers / LDS -- the same operations on the same operands, the same bits.
#pragma once

#include <hip/hip_runtime.h>

#include "slamhip_internal.h"

namespace slamhip {

struct ScanPoint {
  double range, cos_a, sin_a, weight, factor;
};

// point q < a.n of the scan
__device__ __forceinline__ ScanPoint scan_assemble_point(const ScanAssembleArgs &a, int q) {
  ScanPoint p;
  p.range = a.h_range[q];
  const int i = a.h_kept ? a.h_kept[q] : q;
  p.cos_a = a.tab_cos[i];
  p.sin_a = a.tab_sin[i];
  // weighting 0: the host's 1.0 / k; 1: the host's own product, operand for operand (f64 sqrt is correctly rounded
  // on both sides, the one multiplication has nothing to contract with); 2: made on the host
  p.weight = a.h_weight ? a.h_weight[q] : (a.tab_viny ? a.tab_viny[i] * sqrt(p.range) : a.w_even);
  p.factor = a.h_factor ? a.h_factor[q] : 1.0;
  return p;
}

}  // namespace slamhip
