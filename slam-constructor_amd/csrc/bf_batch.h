// bf_batch.h -- what bf_batch.hip and its host driver (bf_batch_run, matchers.cpp) share: K brute-force sweeps of one
// matcher in three launches.
#pragma once

#include <hip/hip_runtime.h>

#include "bf_device.h"
#include "slamhip_internal.h"

namespace slamhip {

// one job of the call: its map and scan as the lone sweep would score through them, its two poses, and where its
// slices of the call's flat arrays begin
struct BfJobView {
  MapView map;
  ScanView scan;
  double init[3];  // pose 0 of the job's sweep
  double base[3];  // the base its enumerator stream has latched (BfPoseArgs::base)
  long long at;    // first element of the job's n scores / fingerprints / prefix indices
  long long blk;   // first element of the job's per-block aggregates (ceil((n - 1) / 1024) of them)
};

struct BfBatchArgs {
  const BfJobView *jobs;  // n_jobs entries in HBM, staged once per call
  const double *off;      // the matcher's offsets (BfPoseArgs::off)
  int nx, ny, nt;
  int n;                  // poses per job: 1 + nx ny nt (all jobs of a matcher share it)
  int n_jobs;
  int oie;
  int poses_per_block;
  int verify;
  double *scores;                // n_jobs x n
  unsigned long long *fprints;   // n_jobs x n (verify only)
  long long *pidx;               // n_jobs x n
  double *agg_s;
  long long *agg_i;
  unsigned *counters;  // three words per job (BfArgmaxArgs::counters), then ONE word: jobs whose result is written
  BfHostOut *out;      // pinned, n_jobs entries (their `seq` stays unused)
  unsigned *done;      // pinned: `seq` once the last job has written its entry
  unsigned seq;
};

// the most beams of a job the shared launches score, and the most poses (K x n) their scratch is sized for
constexpr int kBfBatchMaxBeams = 4096;
constexpr long long kBfBatchMaxPoses = 1ll << 24;

// score, scan, decide: three launches on `stream`.  cell_model: the effective model of every job's view; max_beams: the
// most beams of a job.
hipError_t launch_bf_batch(const BfBatchArgs &a, int cell_model, int max_beams, hipStream_t stream);
// the first of the three alone (slamhip_matcher_bf_peaks_batch: its own kernels read the scores); verify 0, a.n >= 2
hipError_t launch_bf_batch_score(const BfBatchArgs &a, int cell_model, int max_beams, hipStream_t stream);

}  // namespace slamhip
