// gm_carry.h -- the GMapping OOPE's run cache carried from pose to pose, as a walk over the scoring kernels' per-pose
// side outputs.  One text for the host and the device (k_gm_carry_jobs, gm_score_batch.hip); no HIP, no other header of
// the library: tests/native/gm_carry_test.cpp compiles this file alone with g++.
//   GmappingOccupancyObservationPE::_cached_coord / _cached_prob   src/slams/gmapping/gmapping_occupancy_observation_pe.h:21-24,36-37
// The reference's estimator keeps ONE (cell, value) pair: a beam whose end cell equals the cached cell takes the cached
// value, any other beam computes its value and caches it.  Inside a pose that makes every maximal run of equal end
// cells take the value of its first beam, which the scoring kernels resolve themselves (gm_score_device.h); ACROSS poses
// the first run of a pose takes the value the previous pose ended with when it starts in the cell that pose ended in.
// The kernels score every pose from an empty cache and leave what this walk needs to put the carried value in.
#pragma once

#if defined(__HIPCC__)
#define SLAMHIP_GM_CARRY_HD __host__ __device__
#else
#define SLAMHIP_GM_CARRY_HD
#endif

namespace slamhip {

// per-pose side outputs of the GMapping kernel for the carry-in fix-up
struct GmPoseInfo {
  int first_cx, first_cy;  // cell of beam 0
  int last_cx, last_cy;    // cell of the last beam
  double v0;               // fresh value of the first run
  double last_v;           // resolved value of the last run (before any carry-in)
  int run0_len;            // beams in the first run (they all hold v0)
  int last_head;           // beam index heading the last run (0 => the last run is run 0)
};

// the estimator's cache between two poses; prob == -1: empty (no value of the OOPE is negative)
struct GmCarryCache {
  int cx, cy;
  double prob;
};
SLAMHIP_GM_CARRY_HD inline GmCarryCache gm_carry_empty() { return GmCarryCache{0, 0, -1.0}; }

// One pose: what the cache `cr` does to its score, and what the pose leaves in the cache.  The operations of
// gm_carry_fixup (slamhip_api.cpp) in its order: the terms of the first run are taken out with the fresh value and put
// in with the carried one, beam after beam; a pose that is ONE run hands the carried value on.  weight / factor: the
// scan's per-beam arrays; tot_w: its weight sum (0: the score is NaN and stays so).  True when the first run took the
// carried value instead of its fresh one.
SLAMHIP_GM_CARRY_HD inline bool gm_carry_pose(GmCarryCache &cr, const GmPoseInfo &gi, const double *weight,
                                              const double *factor, double tot_w, double *score) {
  bool carried = false;
  double last_v = gi.last_v;
  if (cr.prob != -1.0 && gi.first_cx == cr.cx && gi.first_cy == cr.cy) {
    const double c = cr.prob;
    if (c != gi.v0) {
      double delta = 0.0;
      for (int b = 0; b < gi.run0_len; ++b) delta += (c * weight[b]) * factor[b] - (gi.v0 * weight[b]) * factor[b];
      if (tot_w != 0.0) *score += delta / tot_w;
      carried = true;
    }
    if (gi.last_head == 0) last_v = c;
  }
  cr.cx = gi.last_cx;
  cr.cy = gi.last_cy;
  cr.prob = last_v;
  return carried;
}

// A job: n_poses poses scored in the order given by one estimator object whose cache is `cr` when it starts (an empty
// one for a job of slamhip_gmapping_particle_score_poses) and holds the last pose's entry afterwards.  info / scores: the
// job's slices.  Returns the number of poses whose first run took the carried value.
// The side outputs are read kCarryChunk poses at a time -- independent loads, issued together -- ahead of the serial
// walk over them: one lane of the device walks a job, and a load per pose in the loop's dependency chain was a trip to
// memory per pose.
constexpr int kCarryChunk = 8;
SLAMHIP_GM_CARRY_HD inline int gm_carry_walk(GmCarryCache &cr, int n_poses, const GmPoseInfo *info, const double *weight,
                                             const double *factor, double tot_w, double *scores) {
  int n_carried = 0;
  for (int p0 = 0; p0 < n_poses; p0 += kCarryChunk) {
    GmPoseInfo gi[kCarryChunk];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = 0; j < kCarryChunk; ++j) gi[j] = info[p0 + j < n_poses ? p0 + j : n_poses - 1];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = 0; j < kCarryChunk; ++j) {
      if (p0 + j < n_poses && gm_carry_pose(cr, gi[j], weight, factor, tot_w, scores + p0 + j)) ++n_carried;
    }
  }
  return n_carried;
}

}  // namespace slamhip
