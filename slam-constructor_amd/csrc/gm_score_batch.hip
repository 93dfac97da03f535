// gm_score_batch.hip -- the pose sets of K jobs over the particles' OWN maps (the copy-on-write tile pool of a GMapping
// filter, tile_pool.h) in one scoring launch and one carry launch: slamhip_gmapping_particle_score_poses.
//
//   GmappingOccupancyObservationPE   src/slams/gmapping/gmapping_occupancy_observation_pe.h:17-38
//
// k_score_gmapping_jobs is the job-table form of K3 (k_score_gmapping / k_score_gmapping_wide, score_kernels.hip): the grid
// is flat, workgroup b reads entry b of a block table (score_batch_plan.h) -- its job and its pose of that job --, then
// its job's entry of the job table: the scan, the tile-table row of the particle's slot, the offset into the call's flat
// pose / score / side-output arrays.  All of them are workgroup-uniform addresses read before any store: scalar loads,
// as in k_score_point_batch and k_bf_score_batch.  The map view -- pool, virtual extent, tiles per row -- is the call's.
// Every statement of arithmetic is gm_score_pose_wide's (gm_score_device.h: gm_fresh_value, the run resolution, the
// canonical 256-thread sum), which the lone kernels and the chains score through: a pose gets the bits the lone call
// gets for it over the same cells, whichever of the two workgroup sizes runs and whatever the other jobs are.
// Scans differ in length from job to job: the kernel is instantiated on KB = ceil(longest scan / 256) and sizes its LDS
// for it; beams b >= n of a shorter job add nothing (every loop of the body is guarded by b < n), and the first 256
// threads add a job's terms t, t + 256, ... in that order whatever KB is: the sum's bits are those of the lone call's
// own KB (the argument k_bf_score_batch makes).
//
// k_gm_carry_jobs carries each job's run cache from pose to pose (gm_carry.h): one lane per job walks the job's side
// outputs in pose order, starting from an empty cache, and reads weights and factors from the job's scan in HBM.
#include <hip/hip_runtime.h>

#include "gm_score_batch.h"
#include "gm_score_device.h"
#include "kernel_pick.h"

namespace slamhip {

// NT = 1024: K3's wide form (phase A over sixteen waves) for calls that leave the chip empty; NT = 256: one pose per
// workgroup of four waves -- through tile tables that beat the multi-pose body at every size (launch_score) -- in the
// XCD-chunked block order: consecutive blocks are consecutive poses of one job, i.e. one particle's tiles, and XCD x
// takes the x-th contiguous eighth of them (the grid is rounded up to a multiple of 8; a.n_blocks is the real count).
template <int KB, int NT>
__global__ __launch_bounds__(NT) void k_score_gmapping_jobs(GmScoreBatchArgs a) {
  extern __shared__ double s_dyn[];  // gm_score_pose_wide's arrays
  __shared__ double s_pose1[4];
  __shared__ double s_part1[4];
  __shared__ double s_unknown[4];
  __shared__ int s_run0_len;
  const int t = threadIdx.x;
  int vb = (int)blockIdx.x;
  if (NT == kGmBlock && (gridDim.x & 7u) == 0u && gridDim.x >= 16u) {
    vb = (int)(blockIdx.x & 7) * (int)(gridDim.x >> 3) + (int)(blockIdx.x >> 3);
  }
  if (vb >= a.n_blocks) return;  // (the whole workgroup, before any barrier)
  const score_plan::Block blk = a.blocks[vb];
  const GmScoreJob &jv = a.jobs[blk.job];
  const ScanView scan = jv.scan;
  const int n = scan.n;
  const long long p = jv.at + blk.first_pose;
  const int *tiles = a.tables + (size_t)jv.slot * a.table_stride;
  // pose loads first, every thread's first beam right behind them: see k_score_gmapping_wide
  double pose_x = 0.0, pose_y = 0.0, pose_th = 0.0, pose_sn = 0.0, pose_cs = 0.0;
  if (t == 0) {
    pose_th = a.poses[3 * p + 2];
    pose_x = a.poses[3 * p];
    pose_y = a.poses[3 * p + 1];
    if (a.pose_sc) {
      pose_sn = a.pose_sc[2 * p];
      pose_cs = a.pose_sc[2 * p + 1];
    }
  }
  const bool has0 = t < n;
  const double r0 = has0 ? scan.range[t] : 0.0, ca0 = has0 ? scan.cos_a[t] : 0.0, sa0 = has0 ? scan.sin_a[t] : 0.0;
  if (t == 64) {
    s_unknown[0] = a.map.unknown[0];
    s_unknown[1] = a.map.unknown[1];
    s_unknown[2] = a.map.unknown[2];
  }
  if (t == 0) {
    if (!a.pose_sc) sincos(pose_th, &pose_sn, &pose_cs);
    s_pose1[0] = pose_x;
    s_pose1[1] = pose_y;
    s_pose1[2] = pose_sn;
    s_pose1[3] = pose_cs;
    s_run0_len = n;
  }
  __syncthreads();
  double score;
  gm_score_pose_wide<KB, NT>(a.map, scan, a.gm, tiles, s_unknown, s_pose1[0], s_pose1[1], s_pose1[2], s_pose1[3], r0, ca0, sa0,
                             s_dyn, &s_run0_len, s_part1, a.info + p, &score);
  if (t == 0) a.scores[p] = score;
}

__global__ __launch_bounds__(64) void k_gm_carry_jobs(GmScoreBatchArgs a) {
  const int k = (int)(blockIdx.x * 64 + threadIdx.x);
  if (k >= a.n_jobs) return;
  const GmScoreJob &jv = a.jobs[k];
  int n_carried = 0;
  if (jv.n_poses > 0) {
    GmCarryCache cr = gm_carry_empty();
    n_carried = gm_carry_walk(cr, jv.n_poses, a.info + jv.at, jv.scan.weight, jv.scan.factor, jv.scan.tot_w, a.scores + jv.at);
  }
  a.carried[k] = n_carried;
}

// dynamic LDS of a workgroup of nt threads: the 256-thread body keeps its terms in registers and has no helper lanes
static size_t gm_jobs_lds_bytes(int kb, int nt) {
  if (nt == kGmBlock) return (size_t)kb * kGmBlock * sizeof(double) + 4 * (size_t)kb * sizeof(int2) + 4 * (size_t)kb * sizeof(int);
  return gm_chain_lds_bytes(kb, nt);
}

hipError_t launch_gm_score_batch(const GmScoreBatchArgs &a, long long total_poses, int max_beams, hipStream_t stream,
                                 hipEvent_t ev[4], int *launches) {
  *launches = 0;
  if (a.n_blocks <= 0 || total_poses <= 0) return hipSuccess;
  if (a.n_jobs <= 0 || max_beams <= 0 || (long long)a.n_blocks != total_poses) return hipErrorInvalidValue;
  const int kb = (max_beams + kGmBlock - 1) / kGmBlock;
  if (kb > 8) return refuse_launch("the GMapping kernel holds at most 2048 filtered beams per scan");
  const bool wide = total_poses <= kGmBatchWideBelow;
  const auto score = [&](auto kb_c) {
    constexpr int K = decltype(kb_c)::value;
    if (wide)
      return launch_kernel(k_score_gmapping_jobs<K, 1024>, dim3((unsigned)a.n_blocks), dim3(1024), gm_jobs_lds_bytes(K, 1024),
                           stream, ev[0], ev[1], a);
    const unsigned grid = a.n_blocks >= 16 ? ((unsigned)a.n_blocks + 7u) / 8u * 8u : (unsigned)a.n_blocks;
    return launch_kernel(k_score_gmapping_jobs<K, kGmBlock>, dim3(grid), dim3(kGmBlock), gm_jobs_lds_bytes(K, kGmBlock), stream,
                         ev[0], ev[1], a);
  };
  hipError_t e = hipSuccess;
  switch (kb) {
    case 1: e = score(int_c<1>{}); break;
    case 2: e = score(int_c<2>{}); break;
    case 3: e = score(int_c<3>{}); break;
    case 4: e = score(int_c<4>{}); break;
    case 5: e = score(int_c<5>{}); break;
    case 6: e = score(int_c<6>{}); break;
    case 7: e = score(int_c<7>{}); break;
    default: e = score(int_c<8>{}); break;
  }
  if (e != hipSuccess) return e;
  *launches = 1;
  e = launch_kernel(k_gm_carry_jobs, dim3((unsigned)((a.n_jobs + 63) / 64)), dim3(64), 0, stream, ev[2], ev[3], a);
  if (e != hipSuccess) return e;
  *launches = 2;
  return hipSuccess;
}

}  // namespace slamhip
