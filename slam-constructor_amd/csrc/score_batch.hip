// score_batch.hip -- the pose sets of K jobs, each over its own map and scan, in ONE scoring launch
// (slamhip_score_poses_batch): the job-table forms of k_score_point, k_score_window and k_sum_sequential.
//
//   WeightedMeanPointProbabilitySPE::estimate_scan_probability   src/core/scan_matchers/weighted_mean_point_probability_spe.h:97-133
//
// A lone scoring call is a launch and a hand-over around a few microseconds of device work; K robots, K map hypotheses
// under one scan or K heat maps cost K times that with the chip idle.  Here the call's poses lie in one flat array, job
// after job, and the grid is flat too: workgroup b reads entry b of a block table (score_batch_plan.h) -- its job and
// the first of its poses --, then its job's entry of the job table.  Both addresses are workgroup-uniform, so the map
// and scan views come in as scalar loads, as in k_bf_score_batch.  A workgroup serves ONE job; pose counts may differ
// from job to job (grid.y = job would launch the largest job's workgroups for every job).  Every statement of
// arithmetic is the lone kernels' own -- score_point_body, score_window_body (score_device.h) -- so a job gets the
// bits the lone call over its scan, map and poses gets, whatever the other jobs of the call are and however many
// poses a workgroup takes.  Independent workgroups: no flags, no spins, nothing that needs them resident together.
#include <hip/hip_runtime.h>

#include "kernel_pick.h"
#include "score_batch.h"
#include "score_device.h"

namespace slamhip {

// the poses of workgroup (job view jv, first pose p0) into s_pose: x, y, sin, cos -- k_score_point's prologue over the
// job's slice of the flat arrays.  Returns with the pose's loads issued and its sincos done; the caller's barrier follows.
__device__ __forceinline__ void score_batch_stage_poses(const ScoreBatchArgs &a, const ScoreJobView &jv, int p0, int npb,
                                                        double (*s_pose)[4]) {
  const int t = threadIdx.x;
  if (t < npb) {
    const long long p = jv.at + p0 + t;
    const double th = a.poses[3 * p + 2];
    double sn, cs;
    if (a.pose_sc) {
      sn = a.pose_sc[2 * p];
      cs = a.pose_sc[2 * p + 1];
    } else {
      sincos(th, &sn, &cs);
    }
    s_pose[t][0] = a.poses[3 * p];
    s_pose[t][1] = a.poses[3 * p + 1];
    s_pose[t][2] = sn;
    s_pose[t][3] = cs;
  }
}

// KB > 0: every job has at most 256 KB beams (beams b >= n_j add nothing: the sum and the fingerprint are those of the
// lone call's own KB); KB == 0: the generic form, any beam count.  WRITE_TERMS, FPRINT: as k_score_point.
template <int MODEL, int KB, bool WRITE_TERMS, bool FPRINT>
__global__ __launch_bounds__(kScoreBlock) void k_score_point_batch(ScoreBatchArgs a) {
  __shared__ double s_pose[kScoreMaxPosesPerBlock][4];
  __shared__ double s_part[kScoreMaxPosesPerBlock][4];
  __shared__ unsigned long long s_hpart[FPRINT ? kScoreMaxPosesPerBlock : 1][4];
  const score_plan::Block blk = a.blocks[blockIdx.x];
  const ScoreJobView &jv = a.jobs[blk.job];
  const MapView map = jv.map;
  const ScanView scan = jv.scan;
  const int t = threadIdx.x;
  const int n = scan.n;
  const int p0 = blk.first_pose;
  const int npb = min(a.poses_per_block, jv.n_poses - p0);
  // (the beam constants' loads stand between the pose's loads and its sincos, as in k_score_point)
  double pose_x = 0.0, pose_y = 0.0, pose_th = 0.0, pose_sn = 0.0, pose_cs = 0.0;
  if (t < npb) {
    const long long p = jv.at + p0 + t;
    pose_th = a.poses[3 * p + 2];
    pose_x = a.poses[3 * p];
    pose_y = a.poses[3 * p + 1];
    if (a.pose_sc) {
      pose_sn = a.pose_sc[2 * p];
      pose_cs = a.pose_sc[2 * p + 1];
    }
  }
  constexpr int KR = KB > 0 ? KB : 1;
  double br[KR], bc[KR], bs[KR], bw[KR], bf[KR];
  score_point_load_beams<KB>(scan, n, t, br, bc, bs, bw, bf);
  if (t < npb) {
    if (!a.pose_sc) sincos(pose_th, &pose_sn, &pose_cs);
    s_pose[t][0] = pose_x;
    s_pose[t][1] = pose_y;
    s_pose[t][2] = pose_sn;
    s_pose[t][3] = pose_cs;
  }
  __syncthreads();
  score_point_body<MODEL, KB, WRITE_TERMS, FPRINT>(map, scan, a.oie, n, p0, npb, s_pose, s_part, s_hpart, br, bc, bs, bw, bf,
                                                   WRITE_TERMS ? a.terms + jv.term_at : nullptr, a.scores + jv.at,
                                                   FPRINT ? a.fprints + jv.at : nullptr);
}

template <int MODEL>
__global__ __launch_bounds__(kScoreBlock) void k_score_window_batch(ScoreBatchArgs a) {
  __shared__ double s_pose[kScoreMaxPosesPerBlock][4];
  __shared__ double s_part[kScoreMaxPosesPerBlock][4];
  __shared__ unsigned long long s_hpart[kScoreMaxPosesPerBlock][4];
  const score_plan::Block blk = a.blocks[blockIdx.x];
  const ScoreJobView &jv = a.jobs[blk.job];
  const MapView map = jv.map;
  const ScanView scan = jv.scan;
  const int p0 = blk.first_pose;
  const int npb = min(a.poses_per_block, jv.n_poses - p0);
  score_batch_stage_poses(a, jv, p0, npb, s_pose);
  __syncthreads();
  score_window_body<MODEL>(map, scan, a.oie, a.oope, a.half_v, a.half_h, scan.n, p0, npb, s_pose, s_part, s_hpart,
                           a.terms ? a.terms + jv.term_at : nullptr, a.scores + jv.at, a.fprints ? a.fprints + jv.at : nullptr);
}

// the reference's sequential beam-order sum (k_sum_sequential), one lane per pose of the flat array
__global__ __launch_bounds__(64) void k_sum_sequential_batch(ScoreBatchArgs a) {
  const long long q = (long long)blockIdx.x * 64 + threadIdx.x;
  if (q < a.total_poses) {
    const ScoreJobView &jv = a.jobs[score_plan::job_of_pose(a.pose_at, a.n_jobs, q)];
    const int n = jv.scan.n;
    const double tot_w = jv.scan.tot_w;
    const double *row = a.terms + jv.term_at + (size_t)(q - jv.at) * n;
    double acc = 0.0;
    for (int b = 0; b < n; ++b) acc = acc + row[b];
    a.scores[q] = (tot_w == 0.0) ? __builtin_nan("") : acc / tot_w;
  }
}

typedef void (*ScoreBatchKernel)(ScoreBatchArgs);
template <int MODEL, bool WT, bool FP>
static ScoreBatchKernel point_batch_kernel(int kb) {
  switch (kb) {
    case 1: return k_score_point_batch<MODEL, 1, WT, FP>;
    case 2: return k_score_point_batch<MODEL, 2, WT, FP>;
    case 3: return k_score_point_batch<MODEL, 3, WT, FP>;
    case 4: return k_score_point_batch<MODEL, 4, WT, FP>;
    case 5: return k_score_point_batch<MODEL, 5, WT, FP>;
    default: return k_score_point_batch<MODEL, 0, WT, FP>;
  }
}

hipError_t launch_score_batch(const ScoreBatchArgs &args, int cell_model, int sum_order, int max_beams, hipStream_t stream,
                              int *launches) {
  ScoreBatchArgs a = args;
  *launches = 0;
  if (a.n_blocks <= 0 || a.total_poses <= 0) return hipSuccess;
  if (a.n_jobs <= 0 || max_beams <= 0 || a.poses_per_block < 1 || a.poses_per_block > kScoreMaxPosesPerBlock)
    return hipErrorInvalidValue;
  const bool wt = sum_order == SLAMHIP_SUM_SEQUENTIAL;
  if (wt && !a.terms) return hipErrorInvalidValue;
  if (wt) a.fprints = nullptr;
  if (!wt) a.terms = nullptr;
  ScoreBatchKernel kernel = nullptr;
  if (a.oope == SLAMHIP_OOPE_MAX || a.oope == SLAMHIP_OOPE_MEAN || a.oope == SLAMHIP_OOPE_OVERLAP) {
    kernel = pick_cell_model(cell_model, [](auto m) -> ScoreBatchKernel { return k_score_window_batch<decltype(m)::value>; });
  } else if (a.oope == SLAMHIP_OOPE_OBSTACLE) {
    const int kb = (max_beams + kScoreBlock - 1) / kScoreBlock;
    kernel = pick_cell_model(cell_model, [&](auto m) -> ScoreBatchKernel {
      constexpr int M = decltype(m)::value;
      return wt ? point_batch_kernel<M, true, false>(kb)
                : (a.fprints ? point_batch_kernel<M, false, true>(kb) : point_batch_kernel<M, false, false>(kb));
    });
  } else {
    return refuse_launch("the shared scoring launch covers the 1-cell and the window OOPEs");
  }
  hipError_t e = launch_kernel(kernel, dim3((unsigned)a.n_blocks), dim3(kScoreBlock), 0, stream, nullptr, nullptr, a);
  if (e != hipSuccess) return e;
  *launches = 1;
  if (wt) {
    e = launch_kernel(k_sum_sequential_batch, dim3((unsigned)((a.total_poses + 63) / 64)), dim3(64), 0, stream, nullptr, nullptr, a);
    if (e != hipSuccess) return e;
    *launches = 2;
  }
  return hipSuccess;
}

}  // namespace slamhip
