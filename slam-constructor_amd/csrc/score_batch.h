// score_batch.h -- what score_batch.hip and its host driver (slamhip_score_poses_batch, slamhip_api.cpp) share: the pose
// sets of K jobs, each over its own map and scan, in one scoring launch.
#pragma once

#include <hip/hip_runtime.h>

#include "score_batch_plan.h"
#include "slamhip_internal.h"

namespace slamhip {

// one job of the call: its map and scan as the lone call would score through them, and where its slices of the call's
// flat arrays begin
struct ScoreJobView {
  MapView map;
  ScanView scan;
  long long at;       // first of the job's poses (x 3 doubles), sin / cos pairs (x 2) and scores
  long long term_at;  // first of the job's n_poses x scan.n terms (SLAMHIP_SUM_SEQUENTIAL only)
  int n_poses;
  int reserved_;
};

struct ScoreBatchArgs {
  const ScoreJobView *jobs;          // n_jobs entries
  const score_plan::Block *blocks;   // one entry per workgroup of the scoring grid
  const long long *pose_at;          // n_jobs + 1 (the summing launch finds a pose's job in it)
  const double *poses;               // total_poses x 3
  const double *pose_sc;             // total_poses x 2 (sin, cos) made by the host; null = device sincos
  double *scores;                    // total_poses
  double *terms;                     // SLAMHIP_SUM_SEQUENTIAL only
  unsigned long long *fprints;       // total_poses term-vector fingerprints next to the scores (the default sum order
                                     // only); null = none
  long long total_poses;
  int n_jobs, n_blocks;
  int poses_per_block;
  int oie, oope;
  double half_v, half_h;  // the window OOPEs: half the analysis area's extent
};

// One scoring launch on `stream` -- k_score_point_batch for SLAMHIP_OOPE_OBSTACLE, k_score_window_batch for the three
// window OOPEs -- and for SLAMHIP_SUM_SEQUENTIAL the beam-order summing launch behind it.  cell_model: the effective
// model of every job's view; max_beams: the most points of a job's scan.  *launches: kernels launched.
hipError_t launch_score_batch(const ScoreBatchArgs &a, int cell_model, int sum_order, int max_beams, hipStream_t stream,
                              int *launches);

}  // namespace slamhip
