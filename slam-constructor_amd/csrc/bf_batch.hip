// bf_batch.hip -- K brute-force sweeps of ONE matcher in three launches (slamhip_matcher_set_bf_streams + the two batch
// calls): score, scan, decide, grid.y = job.
//
//   BruteForcePoseEnumerator / BruteForceScanMatcher   src/core/scan_matchers/brute_force_scan_matcher.h:10-81
//   PoseEnumerationScanMatcher::process_scan           src/core/scan_matchers/pose_enumeration_scan_matcher.h:31-77
//
// A lone sweep (bf_device.hip) is four dependent launches around a few microseconds of device work; K of them cost K
// times that with the chip idle.  All jobs of a matcher share the offsets and the pose count, so one grid covers them:
// blockIdx.y picks the job's entry of a table in HBM (workgroup-uniform: its map and scan views come in as scalar
// loads), blockIdx.x the job's block.  Every statement of arithmetic is the lone sweep's own -- the scorer's body
// (score_point_body, score_device.h), the poses (bf_pose_of), the walk (bf_scan_body, bf_decide_body) -- so job j
// gets the bits a lone sweep over its scan, map and poses gets.  There is no pose array and no pose launch: a scoring
// workgroup makes its poses itself.
#include <hip/hip_runtime.h>

#include "bf_argmax_device.h"
#include "bf_batch.h"
#include "kernel_pick.h"
#include "score_device.h"

namespace slamhip {

// KB > 0: every job has at most 256 KB beams (beams b >= n_j add nothing: the sum and the fingerprint are those of the
// lone call's own KB); KB == 0: the generic form, any beam count.
template <int MODEL, int KB, bool FPRINT>
__global__ __launch_bounds__(kScoreBlock) void k_bf_score_batch(BfBatchArgs a, const BfJobView *__restrict__ jobs) {
  __shared__ double s_pose[kScoreMaxPosesPerBlock][4];
  __shared__ double s_part[kScoreMaxPosesPerBlock][4];
  __shared__ unsigned long long s_hpart[FPRINT ? kScoreMaxPosesPerBlock : 1][4];
  const BfJobView &jv = jobs[blockIdx.y];
  const MapView map = jv.map;
  const ScanView scan = jv.scan;
  const int t = threadIdx.x;
  const int n = scan.n;
  const int p0 = (int)blockIdx.x * a.poses_per_block;
  const int npb = min(a.poses_per_block, a.n - p0);
  double pose_x = 0.0, pose_y = 0.0, pose_th = 0.0;
  if (t < npb) bf_pose_of(p0 + t, jv.init, jv.base, a.off, a.nx, a.ny, &pose_x, &pose_y, &pose_th);
  constexpr int KR = KB > 0 ? KB : 1;
  double br[KR], bc[KR], bs[KR], bw[KR], bf[KR];
  score_point_load_beams<KB>(scan, n, t, br, bc, bs, bw, bf);
  if (t < npb) {
    double pose_sn, pose_cs;
    sincos(pose_th, &pose_sn, &pose_cs);
    s_pose[t][0] = pose_x;
    s_pose[t][1] = pose_y;
    s_pose[t][2] = pose_sn;
    s_pose[t][3] = pose_cs;
  }
  __syncthreads();
  score_point_body<MODEL, KB, false, FPRINT>(map, scan, a.oie, n, p0, npb, s_pose, s_part, s_hpart, br, bc, bs, bw, bf, nullptr,
                                             a.scores + jv.at, FPRINT ? a.fprints + jv.at : nullptr);
}

__global__ __launch_bounds__(kBfBlock) void k_bf_scan_batch(BfBatchArgs a, const BfJobView *__restrict__ jobs) {
  const BfJobView &jv = jobs[blockIdx.y];
  bf_scan_body(blockIdx.x, a.scores + jv.at, a.n, a.pidx + jv.at, a.agg_s + jv.blk, a.agg_i + jv.blk);
}

// The last block of job k writes the job's entry; the job that finds every entry written publishes the call's ONE
// completion word (the lone kernel's ordering: fence, results, system-scope release store).
__global__ __launch_bounds__(kBfBlock) void k_bf_decide_batch(BfBatchArgs a, const BfJobView *__restrict__ jobs) {
  const BfJobView &jv = jobs[blockIdx.y];
  if (bf_decide_body(blockIdx.x, gridDim.x, a.scores + jv.at, a.verify ? a.fprints + jv.at : nullptr, a.n, a.verify,
                     a.pidx + jv.at, a.agg_s + jv.blk, a.agg_i + jv.blk, a.counters + 3 * blockIdx.y, a.out + blockIdx.y)) {
    __threadfence_system();  // (the entry is on its way before the job is counted)
    unsigned *jobs_done = a.counters + 3 * (size_t)a.n_jobs;
    const unsigned before = __hip_atomic_fetch_add(jobs_done, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (before + 1u == (unsigned)a.n_jobs) {
      __hip_atomic_store(jobs_done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __threadfence_system();
      __hip_atomic_store(a.done, a.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

typedef void (*BfScoreKernel)(BfBatchArgs, const BfJobView *);
template <int MODEL, bool FP>
static BfScoreKernel bf_score_kernel(int kb) {
  switch (kb) {
    case 1: return k_bf_score_batch<MODEL, 1, FP>;
    case 2: return k_bf_score_batch<MODEL, 2, FP>;
    case 3: return k_bf_score_batch<MODEL, 3, FP>;
    case 4: return k_bf_score_batch<MODEL, 4, FP>;
    case 5: return k_bf_score_batch<MODEL, 5, FP>;
    default: return k_bf_score_batch<MODEL, 0, FP>;
  }
}

// what every launch of a call checks first, in this order, and the arguments as launched (poses_per_block picked)
static hipError_t bf_batch_checked(const BfBatchArgs &args, int max_beams, BfBatchArgs *out) {
  BfBatchArgs a = args;
  if (a.n_jobs <= 0 || a.n_jobs > 65535 || a.n < 2 || max_beams <= 0) return hipErrorInvalidValue;
  if ((long long)a.n_jobs * a.n > kBfBatchMaxPoses) return refuse_launch("the batch's sweeps outgrow the scratch budget");
  if (a.poses_per_block <= 0) a.poses_per_block = pick_poses_per_block((long long)a.n_jobs * a.n);
  if (a.poses_per_block > kScoreMaxPosesPerBlock) a.poses_per_block = kScoreMaxPosesPerBlock;
  *out = a;
  return hipSuccess;
}

// the scoring launch of checked arguments
static hipError_t bf_batch_score(const BfBatchArgs &a, int cell_model, int max_beams, hipStream_t stream) {
  const int kb = (max_beams + kScoreBlock - 1) / kScoreBlock;
  const bool fp = a.verify != 0;
  const BfScoreKernel score = pick_cell_model(cell_model, [&](auto m) -> BfScoreKernel {
    constexpr int M = decltype(m)::value;
    return fp ? bf_score_kernel<M, true>(kb) : bf_score_kernel<M, false>(kb);
  });
  const dim3 grid_score((unsigned)((a.n + a.poses_per_block - 1) / a.poses_per_block), (unsigned)a.n_jobs);
  return launch_kernel(score, grid_score, dim3(kScoreBlock), 0, stream, nullptr, nullptr, a, a.jobs);
}

hipError_t launch_bf_batch_score(const BfBatchArgs &args, int cell_model, int max_beams, hipStream_t stream) {
  BfBatchArgs a;
  const hipError_t e = bf_batch_checked(args, max_beams, &a);
  if (e != hipSuccess) return e;
  return bf_batch_score(a, cell_model, max_beams, stream);
}

hipError_t launch_bf_batch(const BfBatchArgs &args, int cell_model, int max_beams, hipStream_t stream) {
  BfBatchArgs a;
  hipError_t e = bf_batch_checked(args, max_beams, &a);
  if (e != hipSuccess) return e;
  const unsigned blocks = (unsigned)((a.n - 1 + kBfBlock - 1) / kBfBlock);
  if (blocks == 0 || blocks > (unsigned)kBfMaxBlocks) return hipErrorInvalidValue;
  e = bf_batch_score(a, cell_model, max_beams, stream);
  if (e != hipSuccess) return e;
  e = launch_kernel(k_bf_scan_batch, dim3(blocks, (unsigned)a.n_jobs), dim3(kBfBlock), 0, stream, nullptr, nullptr, a, a.jobs);
  if (e != hipSuccess) return e;
  return launch_kernel(k_bf_decide_batch, dim3(blocks, (unsigned)a.n_jobs), dim3(kBfBlock), 0, stream, nullptr, nullptr, a, a.jobs);
}

}  // namespace slamhip
