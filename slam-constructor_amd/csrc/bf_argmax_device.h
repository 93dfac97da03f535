// bf_argmax_device.h -- the device bodies of the brute-force arg-max, shared by the lone sweep's kernels (k_bf_scan,
// k_bf_decide: bf_device.hip) and the batch's (k_bf_scan_batch, k_bf_decide_batch: bf_batch.hip, grid.y = job): one
// definition of the walk's rule, so a job of a batch gets the lone sweep's answer.
//   PoseEnumerationScanMatcher::process_scan   src/core/scan_matchers/pose_enumeration_scan_matcher.h:48-69
#pragma once

#include <hip/hip_runtime.h>

#include "bf_device.h"

namespace slamhip {

// (score, index) of the walk's best so far; a later element replaces it only when STRICTLY greater -- the
// reference's `best < candidate` (ties and NaN are rejections), so the fold is associative and the first maximum wins
struct BfBest {
  double s;
  long long i;
};
__device__ __forceinline__ BfBest bf_fold(const BfBest &earlier, const BfBest &later) {
  return later.s > earlier.s ? later : earlier;
}
__device__ __forceinline__ BfBest bf_shfl_up(const BfBest &v, int d) {
  BfBest o;
  o.s = __shfl_up(v.s, d, 64);
  o.i = __shfl_up(v.i, d, 64);
  return o;
}
constexpr int kBfBlock = 1024;

// Stage 1, one candidate per thread (coalesced): the inclusive scan of the walk inside block `blk` of 1024 candidates.
// Every candidate learns the best of the candidates in front of it in ITS block (pidx, -1 = none); the block's own
// best goes to agg.  (workgroups of kBfBlock threads)
__device__ __forceinline__ void bf_scan_body(unsigned blk, const double *scores, long long n, long long *pidx, double *agg_s,
                                             long long *agg_i) {
  __shared__ double s_ws[16];
  __shared__ long long s_wi[16];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const long long e = 1 + (long long)blk * kBfBlock + t;
  BfBest v{-__builtin_inf(), -1};
  if (e < n) {
    const double s = scores[e];
    if (s == s) v = BfBest{s, e};  // (a NaN is never accepted: it takes part as -infinity)
  }
  BfBest inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const BfBest o = bf_shfl_up(inc, d);
    if (lane >= d) inc = bf_fold(o, inc);
  }
  if (lane == 63) {
    s_ws[wave] = inc.s;
    s_wi[wave] = inc.i;
  }
  __syncthreads();
  BfBest before{-__builtin_inf(), -1};  // the waves in front of this one
  for (int w = 0; w < wave; ++w) before = bf_fold(before, BfBest{s_ws[w], s_wi[w]});
  BfBest excl = bf_shfl_up(inc, 1);
  if (lane == 0) excl = BfBest{-__builtin_inf(), -1};
  excl = bf_fold(before, excl);
  if (e < n) pidx[e] = excl.i;
  if (t == kBfBlock - 1) {
    const BfBest all = bf_fold(before, inc);
    agg_s[blk] = all.s;
    agg_i[blk] = all.i;
  }
}

// Stage 2, same grid (`blocks` blocks per sweep): a candidate meets the walk's state in front of it -- the initial pose
// folded with the blocks before its own and with its block's prefix -- with the reference's exact rule and the checked
// mode's closeness test.  counters: the sweep's three words (accepts, ambiguous, blocks done -- zero between matches).
// The last block of the sweep to finish writes the result to *out (everything but `seq`) and zeroes the counters; its
// thread 0 gets `true` back and publishes, behind a system fence, whatever its kernel publishes.
__device__ __forceinline__ bool bf_decide_body(unsigned blk, unsigned blocks, const double *scores,
                                               const unsigned long long *fprints, long long n, int verify, const long long *pidx,
                                               const double *agg_s, const long long *agg_i, unsigned *counters, BfHostOut *out) {
  __shared__ double s_in_s;
  __shared__ long long s_in_i;
  __shared__ int s_last;
  const int t = threadIdx.x, lane = t & 63;
  const long long e = 1 + (long long)blk * kBfBlock + t;
  if (t == 0) {
    BfBest b{scores[0], 0};
    for (unsigned j = 0; j < blk; ++j) b = bf_fold(b, BfBest{agg_s[j], agg_i[j]});
    s_in_s = b.s;
    s_in_i = b.i;
  }
  __syncthreads();
  bool acc = false, amb = false;
  if (e < n) {
    BfBest prev{s_in_s, s_in_i};
    const long long pi = pidx[e];
    if (pi >= 0) prev = bf_fold(prev, BfBest{scores[pi], pi});
    const double s = scores[e];
    if (verify) {
      const double diff = __builtin_fabs(s - prev.s);
      const double as = __builtin_fabs(s), ab = __builtin_fabs(prev.s);
      if (diff <= (as > ab ? as : ab) * 9.094947017729282e-13) {
        // close: settled only when the two term vectors are identical (equal fingerprints AND equal sums)
        amb = fprints[e] != fprints[prev.i] || __double_as_longlong(s) != __double_as_longlong(prev.s);
      }
    }
    acc = prev.s < s;
  }
  const unsigned long long accs = __ballot(acc), ambs = __ballot(amb);
  if (lane == 0) {
    if (accs) atomicAdd(counters + 0, (unsigned)__popcll(accs));
    if (ambs) atomicOr(counters + 1, 1u);
  }
  __syncthreads();
  if (t == 0) {
    __threadfence();
    s_last = atomicAdd(counters + 2, 1u) + 1u == blocks ? 1 : 0;
  }
  __syncthreads();
  if (!(s_last && t == 0)) return false;
  __threadfence();
  BfBest b{scores[0], 0};
  for (unsigned j = 0; j < blocks; ++j) b = bf_fold(b, BfBest{agg_s[j], agg_i[j]});
  out->best_index = b.i;
  out->best_score = b.s;
  out->accepts = (long long)__hip_atomic_load(counters + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  out->ambiguous = (int)__hip_atomic_load(counters + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(counters + 0, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(counters + 1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(counters + 2, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return true;
}

// pose i of a sweep: 0 is the match's initial pose (scored first, pose_enumeration_scan_matcher.h:40-47); i > 0 is the
// base plus the enumerator's accumulated offsets, x fastest, then y, then theta -- its additions, so its bits
__device__ __forceinline__ void bf_pose_of(long long i, const double *init, const double *base, const double *off, int nx, int ny,
                                           double *x, double *y, double *th) {
  *x = init[0];
  *y = init[1];
  *th = init[2];
  if (i > 0) {
    const long long j = i - 1;
    const int ix = (int)(j % nx);
    const long long r = j / nx;
    const int iy = (int)(r % ny), it = (int)(r / ny);
    *x = base[0] + off[ix];
    *y = base[1] + off[nx + iy];
    *th = base[2] + off[nx + ny + it];
  }
}

}  // namespace slamhip
