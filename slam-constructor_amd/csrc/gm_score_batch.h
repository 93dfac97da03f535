// gm_score_batch.h -- what gm_score_batch.hip and its host driver (slamhip_gmapping_particle_score_poses, gmapping.cpp)
// share: the pose sets of K jobs, each over ONE particle's copy-on-write map and its own scan, in one scoring launch
// and one carry launch.
#pragma once

#include <hip/hip_runtime.h>

#include "score_batch_plan.h"
#include "slamhip_internal.h"

namespace slamhip {

// one job of the call: its scan as the lone call would score through it, the tile-table row of its particle's slot and
// where its slices of the call's flat arrays begin.  (An empty job's entry is all zeros: no workgroup reads it, the carry
// launch finds n_poses == 0.)
struct GmScoreJob {
  ScanView scan;
  long long at;  // first of the job's poses (x 3 doubles), sin / cos pairs (x 2), scores and side outputs
  int n_poses;
  int slot;
};

struct GmScoreBatchArgs {
  MapView map;                      // the pool's view: payload = the pool, pitch = tiles per table row, width / height =
                                    // the virtual extent; nbr_ok: the tiles' masks hold for gm.fullness_th
  GmParams gm;
  const int *tables;                // the current generation's tile tables, table_stride ints a slot
  int table_stride;
  int n_jobs, n_blocks;
  const GmScoreJob *jobs;           // n_jobs entries
  const score_plan::Block *blocks;  // one entry per workgroup of the scoring grid: (job, pose of the job)
  const double *poses;              // total poses x 3
  const double *pose_sc;            // total poses x 2 (sin, cos) made by the host; null = device sincos
  double *scores;                   // total poses
  GmPoseInfo *info;                 // total poses: the scoring launch's side outputs, the carry launch's input
  int *carried;                     // n_jobs: poses of the job whose first run took the carried value
};

// poses in a call up to which a pose gets a workgroup of 1024 threads (launch_score's finding for K3 over tile tables)
constexpr long long kGmBatchWideBelow = 160;

// The two launches on `stream`: k_score_gmapping_jobs (one pose per workgroup; 1024 threads up to kGmBatchWideBelow poses,
// else 256) and k_gm_carry_jobs (one lane per job).  max_beams: the most points of a job's scan, at most 2048.
// ev[0..1] / ev[2..3]: optional event pairs that ride on the scoring / the carry dispatch.
hipError_t launch_gm_score_batch(const GmScoreBatchArgs &a, long long total_poses, int max_beams, hipStream_t stream,
                                 hipEvent_t ev[4], int *launches);

}  // namespace slamhip
