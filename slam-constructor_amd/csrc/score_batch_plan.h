// score_batch_plan.h -- the planning of slamhip_score_poses_batch (the pose sets of K jobs, each over its own map and
// scan, through shared launches: score_batch.hip).  Pure host arithmetic, no HIP: which route a call takes, where a
// job's slices of the call's flat pose / score / term arrays begin, and which workgroup of the flat scoring grid
// scores which poses of which job.  tests/native/score_batch_plan_test.cpp compiles this header alone with g++.
#pragma once

#include <cstddef>
#include <vector>

#if defined(__HIPCC__)
#define SLAMHIP_SCORE_PLAN_HD __host__ __device__
#else
#define SLAMHIP_SCORE_PLAN_HD
#endif

namespace slamhip {
namespace score_plan {

// SLAMHIP_SUM_SEQUENTIAL keeps every (pose, beam) term of the call in HBM between its two launches: sum of n_k x beams_k
// doubles.  A call whose term array is longer takes the lone route, job after job (whose own term arrays come and go
// one at a time).  2^24 doubles = 128 MiB, the order of the batched brute-force sweeps' scratch (kBfBatchMaxPoses,
// bf_batch.h); a fixed bound, not a measured one.
constexpr long long kMaxTerms = 1ll << 24;
// the flat scoring grid is one-dimensional
constexpr long long kMaxBlocks = (1ll << 31) - 1;

struct JobShape {
  int n_poses;  // >= 0
  int beams;    // points of the job's scan (not looked at for an empty job)
};

// Workgroup b of the scoring grid serves ONE job: poses [first_pose, first_pose + poses_per_block) of job `job`,
// clipped to the job's count.  (Two ints: the kernels read an entry as one 8-byte scalar load.)
struct Block {
  int job, first_pose;
};

enum Route {
  kRouteNothing = 0,  // no job has a pose
  kRouteLone = 1,     // every non-empty job through the lone call, in job order
  kRouteShared = 2,   // every non-empty job in the shared launches
};

struct Plan {
  Route route = kRouteNothing;
  int poses_per_block = 1;
  int non_empty = 0, max_beams = 0;
  long long total_poses = 0, total_terms = 0;
  std::vector<long long> pose_at;  // K + 1: job k's poses and scores are [pose_at[k], pose_at[k + 1]) of the flat arrays
  std::vector<long long> term_at;  // K + 1: ... its terms [term_at[k], term_at[k + 1]), pose-major (SEQUENTIAL only)
  std::vector<Block> blocks;       // kRouteShared only
};

// lone_only: the configuration is one the shared launches do not cover (the GMapping OOPE, SLAMHIP_POSE_TRIG_RAW_EXACT);
// sequential: SLAMHIP_SUM_SEQUENTIAL.  What goes lone: such a configuration, a call with a single non-empty job (nothing
// to share), a beam-order call whose terms outgrow kMaxTerms, a grid beyond kMaxBlocks.
inline Route route_of(bool lone_only, bool sequential, int non_empty, long long total_terms, long long n_blocks) {
  if (non_empty == 0) return kRouteNothing;
  if (lone_only || non_empty == 1) return kRouteLone;
  if (sequential && total_terms > kMaxTerms) return kRouteLone;
  if (n_blocks > kMaxBlocks) return kRouteLone;
  return kRouteShared;
}

inline long long blocks_of(long long n_poses, int poses_per_block) {
  return (n_poses + poses_per_block - 1) / poses_per_block;
}

// poses_per_block: pick_poses_per_block(total poses) (kernel_pick.h), the caller's to hand in -- results do not depend
// on it; total_poses_of() below gives its argument.
inline long long total_poses_of(const std::vector<JobShape> &jobs) {
  long long total = 0;
  for (const JobShape &j : jobs) total += j.n_poses > 0 ? j.n_poses : 0;
  return total;
}

inline Plan make_plan(const std::vector<JobShape> &jobs, int poses_per_block, bool lone_only, bool sequential) {
  Plan p;
  p.poses_per_block = poses_per_block < 1 ? 1 : poses_per_block;
  long long n_blocks = 0;
  for (const JobShape &j : jobs) {
    const long long n = j.n_poses > 0 ? j.n_poses : 0;
    p.pose_at.push_back(p.total_poses);
    p.term_at.push_back(p.total_terms);
    if (n == 0) continue;
    ++p.non_empty;
    if (j.beams > p.max_beams) p.max_beams = j.beams;
    p.total_poses += n;
    p.total_terms += n * (long long)(j.beams > 0 ? j.beams : 0);
    n_blocks += blocks_of(n, p.poses_per_block);
  }
  p.pose_at.push_back(p.total_poses);
  p.term_at.push_back(p.total_terms);
  p.route = route_of(lone_only, sequential, p.non_empty, p.total_terms, n_blocks);
  if (p.route != kRouteShared) return p;
  p.blocks.reserve((size_t)n_blocks);
  for (int k = 0; k < (int)jobs.size(); ++k)
    for (long long at = 0; at < jobs[(size_t)k].n_poses; at += p.poses_per_block) p.blocks.push_back(Block{k, (int)at});
  return p;
}

// ---- arena --------------------------------------------------------------------------------------------------------
// What the host sends for a shared call is ONE pinned block mirrored by one block in HBM and moved by one copy: the
// job table, pose_at, the block table, the poses and -- SLAMHIP_POSE_TRIG_HOST -- their sin / cos pairs.  Byte
// offsets, each a multiple of 16.
struct Arena {
  size_t jobs = 0, pose_at = 0, blocks = 0, poses = 0, pose_sc = 0, bytes = 0;
};
inline Arena arena_of(const Plan &p, size_t n_jobs, size_t sizeof_job_view, bool host_trig) {
  Arena a;
  size_t at = 0;
  auto take = [&](size_t bytes) {
    const size_t here = at;
    at = (at + bytes + 15) / 16 * 16;
    return here;
  };
  a.jobs = take(n_jobs * sizeof_job_view);
  a.pose_at = take((n_jobs + 1) * sizeof(long long));
  a.blocks = take(p.blocks.size() * sizeof(Block));
  a.poses = take(3 * (size_t)p.total_poses * sizeof(double));
  a.pose_sc = take(host_trig ? 2 * (size_t)p.total_poses * sizeof(double) : 0);
  a.bytes = at;
  return a;
}

// the job of flat pose q: the last k with pose_at[k] <= q (pose_at ascends, pose_at[0] = 0, q < pose_at[n_jobs]); a job
// without poses (pose_at[k] == pose_at[k + 1]) is never returned.  The beam-order summing launch has one lane per pose.
SLAMHIP_SCORE_PLAN_HD inline int job_of_pose(const long long *pose_at, int n_jobs, long long q) {
  int lo = 0, hi = n_jobs;  // pose_at[lo] <= q < pose_at[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (pose_at[mid] <= q) lo = mid;
    else hi = mid;
  }
  return lo;
}

}  // namespace score_plan
}  // namespace slamhip
