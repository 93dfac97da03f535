// bf_peaks_device.h -- what bf_peaks.hip and its host driver (bf_peaks_run, matchers.cpp) share: the peaks of K score
// volumes in three launches behind the scoring launch.  The rule itself is bf_peaks.h.
#pragma once

#include <hip/hip_runtime.h>

#include "bf_peaks.h"

namespace slamhip {

// pinned, per job
struct BfPeaksHostOut {
  long long n_found;    // kept peaks
  long long n_written;  // min(n_found, max_peaks) records of the job's slice of `out`
};

struct BfPeaksArgs {
  const double *volumes;  // job j's volume: volumes + j * job_stride, nx ny nt doubles (x fastest, y, theta)
  long long job_stride;
  int nx, ny, nt;
  int rx, ry, rt;
  int n_jobs;
  int max_peaks;
  double min_ratio, min_score;
  long long bound;  // B of bf_peaks.h: survivor records per job
  // scratch: per lattice point the best key of its in-plane window (index -1: none), per job the lattice maximum as an
  // ordered 64-bit key (0: no non-NaN score) and the survivors appended -- both zero between calls --, the survivors
  double *plane_s;
  int *plane_i;
  unsigned long long *job_max;
  unsigned *job_count;
  BfPeakKey *survivors;  // n_jobs x bound
  // pinned results: n_jobs entries, n_jobs x max_peaks records
  BfPeaksHostOut *out_hdr;
  BfPeakKey *out;
};

// the tile shapes of the in-plane kernel (outputs per workgroup, x by y) and the radius class each serves
constexpr int kBfPeaksSmallHalo = 8, kBfPeaksSmallTx = 32, kBfPeaksSmallTy = 8;
constexpr int kBfPeaksLargeHalo = 32, kBfPeaksLargeTx = 16, kBfPeaksLargeTy = 8;

// plane, theta + compaction, ordering on `stream`; the results are in the pinned blocks once the stream has drained.
// *launched grows by one per kernel that went out (slamhip_matcher_bf_peaks_stats counts launches where they are made).
hipError_t launch_bf_peaks(const BfPeaksArgs &a, hipStream_t stream, long long *launched);

}  // namespace slamhip
