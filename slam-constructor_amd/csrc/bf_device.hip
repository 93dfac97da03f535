// bf_device.hip -- the brute-force matcher as ONE flat sweep + a device arg-max.
//
//   BruteForcePoseEnumerator / BruteForceScanMatcher   src/core/scan_matchers/brute_force_scan_matcher.h:10-81
//   PoseEnumerationScanMatcher::process_scan           src/core/scan_matchers/pose_enumeration_scan_matcher.h:31-77
//   (the 201 x 201 search-space sweep of src/utils/pose2D_search_space_evaluator.cpp:154-184)
//
// A brute-force enumerator hands out the same poses whatever the scorer says (accept_changes_future() == false in
// matchers.h), so nothing has to be replayed between batches: the whole pose list is made on the device
// (k_bf_poses: base + the enumerator's own accumulated offsets, the additions it makes, so the bits it makes),
// scored by K1 / K2 in one launch at the flat sweep's rate, and reduced by two small kernels (k_bf_scan: a block-wise
// prefix scan of the walk, one candidate per thread; k_bf_decide: every candidate against the walk's state in front
// of it) to what the reference's loop returns -- the FIRST pose holding the maximum under a strict `best <
// candidate` (:56), NaN never accepted -- with the checked default mode's test riding along: a comparison of the walk whose two canonical sums lie within
// 2^-40 of each other while their term vectors differ (64-bit fingerprints) sets a flag, and the host then runs the
// match on the host-driven path, which settles such comparisons from beam-order sums.
#include <hip/hip_runtime.h>

#include "bf_argmax_device.h"
#include "bf_device.h"

namespace slamhip {

__global__ __launch_bounds__(256) void k_bf_poses(BfPoseArgs a) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n) return;
  double x, y, th;
  bf_pose_of(i, a.init, a.base, a.off, a.nx, a.ny, &x, &y, &th);  // (bf_argmax_device.h: the batch makes its poses by it too)
  a.poses[3 * i] = x;
  a.poses[3 * i + 1] = y;
  a.poses[3 * i + 2] = th;
}

// Stage 1 and stage 2 of the arg-max (bf_scan_body, bf_decide_body: bf_argmax_device.h, shared with the batch's
// kernels).  The last block of the decide stage to finish publishes the result.
__global__ __launch_bounds__(kBfBlock) void k_bf_scan(BfArgmaxArgs a) {
  bf_scan_body(blockIdx.x, a.scores, a.n, a.pidx, a.agg_s, a.agg_i);
}

__global__ __launch_bounds__(kBfBlock) void k_bf_decide(BfArgmaxArgs a) {
  if (bf_decide_body(blockIdx.x, gridDim.x, a.scores, a.fprints, a.n, a.verify, a.pidx, a.agg_s, a.agg_i, a.counters, a.out)) {
    __threadfence_system();
    __hip_atomic_store(&a.out->seq, a.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

hipError_t launch_bf_poses(const BfPoseArgs &a, hipStream_t stream) {
  hipLaunchKernelGGL(k_bf_poses, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, stream, a);
  return hipGetLastError();
}
hipError_t launch_bf_argmax(const BfArgmaxArgs &a, hipStream_t stream) {
  const unsigned blocks = (unsigned)((a.n - 1 + kBfBlock - 1) / kBfBlock);
  if (blocks == 0 || blocks > (unsigned)kBfMaxBlocks) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_bf_scan, dim3(blocks), dim3(kBfBlock), 0, stream, a);
  hipLaunchKernelGGL(k_bf_decide, dim3(blocks), dim3(kBfBlock), 0, stream, a);
  return hipGetLastError();
}

}  // namespace slamhip
