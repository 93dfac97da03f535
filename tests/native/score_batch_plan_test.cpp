// score_batch_plan_test.cpp -- csrc/score_batch_plan.h alone, with a host compiler: the block table of the flat scoring
// grid (every workgroup inside one job, every pose of every job covered exactly once, empty jobs without workgroups),
// the offsets of the flat arrays, the routing (configurations the shared launches do not cover, a single job, the
// beam-order budget at its edge), the arena's slices, and the bisection the summing launch finds a pose's job with.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "score_batch_plan.h"

using namespace slamhip::score_plan;

#define CHECK(cond)                                                         \
  do {                                                                      \
    if (!(cond)) {                                                          \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);         \
      std::exit(1);                                                         \
    }                                                                       \
  } while (0)

// pick_poses_per_block (csrc/kernel_pick.h, which needs the HIP runtime's header) restated: the thresholds the totals
// below are chosen at
static int poses_per_block_of(long long n) { return n >= 8192 ? 8 : (n >= 2048 ? 4 : (n >= 1024 ? 2 : 1)); }

static void check_shared(const std::vector<JobShape> &jobs, int ppb, bool sequential) {
  const Plan p = make_plan(jobs, ppb, false, sequential);
  const int K = (int)jobs.size();
  CHECK(p.route == kRouteShared);
  CHECK(p.poses_per_block == ppb);
  CHECK((int)p.pose_at.size() == K + 1 && (int)p.term_at.size() == K + 1);
  CHECK(p.pose_at[0] == 0 && p.term_at[0] == 0);
  long long poses = 0, terms = 0;
  int non_empty = 0, max_beams = 0;
  for (int k = 0; k < K; ++k) {
    CHECK(p.pose_at[(size_t)k] == poses && p.term_at[(size_t)k] == terms);
    poses += jobs[(size_t)k].n_poses;
    terms += (long long)jobs[(size_t)k].n_poses * jobs[(size_t)k].beams;
    if (jobs[(size_t)k].n_poses > 0) {
      ++non_empty;
      if (jobs[(size_t)k].beams > max_beams) max_beams = jobs[(size_t)k].beams;
    }
  }
  CHECK(p.pose_at[(size_t)K] == poses && p.term_at[(size_t)K] == terms);
  CHECK(p.total_poses == poses && p.total_terms == terms && total_poses_of(jobs) == poses);
  CHECK(p.non_empty == non_empty && p.max_beams == max_beams);
  // every pose of every job in exactly one workgroup, every workgroup inside one job, jobs in order
  std::vector<std::vector<int>> seen((size_t)K);
  for (int k = 0; k < K; ++k) seen[(size_t)k].assign((size_t)jobs[(size_t)k].n_poses, 0);
  int last_job = -1, last_first = -1;
  for (const Block &b : p.blocks) {
    CHECK(b.job >= 0 && b.job < K);
    const int n = jobs[(size_t)b.job].n_poses;
    CHECK(n > 0);  // (an empty job has no workgroup)
    CHECK(b.first_pose >= 0 && b.first_pose < n && b.first_pose % ppb == 0);
    CHECK(b.job > last_job || (b.job == last_job && b.first_pose > last_first));
    last_job = b.job;
    last_first = b.first_pose;
    const int npb = n - b.first_pose < ppb ? n - b.first_pose : ppb;
    CHECK(npb >= 1);
    for (int q = 0; q < npb; ++q) ++seen[(size_t)b.job][(size_t)(b.first_pose + q)];
  }
  long long blocks = 0;
  for (int k = 0; k < K; ++k) {
    for (int v : seen[(size_t)k]) CHECK(v == 1);
    blocks += blocks_of(jobs[(size_t)k].n_poses, ppb);
  }
  CHECK((long long)p.blocks.size() == blocks);
  // the summing launch's bisection: flat pose q belongs to the job whose slice holds it
  for (int k = 0; k < K; ++k)
    for (long long q = p.pose_at[(size_t)k]; q < p.pose_at[(size_t)k + 1]; ++q)
      CHECK(job_of_pose(p.pose_at.data(), K, q) == k);
  // the arena: slices in order, 16-byte aligned, none overlapping, the sin / cos pairs only where the host makes them
  for (int host_trig = 0; host_trig < 2; ++host_trig) {
    const Arena a = arena_of(p, (size_t)K, 176, host_trig != 0);
    CHECK(a.jobs == 0 && a.pose_at >= (size_t)K * 176 && a.blocks >= a.pose_at + ((size_t)K + 1) * 8);
    CHECK(a.poses >= a.blocks + p.blocks.size() * sizeof(Block) && a.pose_sc >= a.poses + 24 * (size_t)poses);
    CHECK(a.bytes >= a.pose_sc + (host_trig ? 16 * (size_t)poses : 0) && a.bytes < a.pose_sc + 16 * (size_t)poses + 16);
    CHECK(a.pose_at % 16 == 0 && a.blocks % 16 == 0 && a.poses % 16 == 0 && a.pose_sc % 16 == 0 && a.bytes % 16 == 0);
  }
}

int main() {
  static_assert(sizeof(Block) == 8, "a block table entry is one 8-byte load");
  // ragged counts with an empty job in the middle, at the totals where pick_poses_per_block changes its answer -- and
  // under every other poses-per-workgroup value as well (results must not depend on it, so any may be handed in)
  const int counts[4][3] = {{1, 3, 1019}, {1, 3, 1020}, {2, 5, 2041}, {5, 8178, 9}};
  const int want_ppb[4] = {1, 2, 4, 8};
  for (int c = 0; c < 4; ++c) {
    const std::vector<JobShape> jobs = {{counts[c][0], 65}, {counts[c][1], 65}, {0, 65}, {counts[c][2], 65}};
    CHECK(poses_per_block_of(total_poses_of(jobs)) == want_ppb[c]);
    for (int ppb : {1, 2, 4, 8, 16})
      for (int seq = 0; seq < 2; ++seq) check_shared(jobs, ppb, seq != 0);
  }
  // empty jobs at both ends, different beam counts
  check_shared({{0, 7}, {4, 1}, {0, 0}, {9, 1281}, {0, 3}}, 4, true);
  check_shared({{17, 256}, {16, 257}}, 16, false);

  // ---- routing
  CHECK(make_plan({}, 1, false, false).route == kRouteNothing);
  CHECK(make_plan({{0, 5}, {0, 9}}, 1, false, false).route == kRouteNothing);
  {
    const Plan p = make_plan({{0, 5}, {0, 9}}, 1, true, true);
    CHECK(p.route == kRouteNothing && p.blocks.empty() && p.total_poses == 0 && p.pose_at.size() == 3);
  }
  CHECK(make_plan({{3, 5}, {4, 9}}, 1, true, false).route == kRouteLone);     // GMapping OOPE, RAW_EXACT
  CHECK(make_plan({{0, 5}, {4, 9}, {0, 1}}, 1, false, false).route == kRouteLone);  // a single job with poses
  CHECK(make_plan({{3, 5}, {4, 9}}, 1, false, false).route == kRouteShared);
  {
    const Plan p = make_plan({{3, 5}, {4, 9}}, 1, true, false);  // a lone plan still says where every job's scores go
    CHECK(p.blocks.empty() && p.pose_at[1] == 3 && p.pose_at[2] == 7 && p.non_empty == 2);
  }
  // the beam-order budget: 2^24 terms go through the shared launches, one more does not; the default order has none
  static_assert(kMaxTerms == (1ll << 24), "the documented budget");
  {
    const std::vector<JobShape> at = {{4096, 2048}, {4096, 2048}};          // 2 x 2^23
    const std::vector<JobShape> over = {{4096, 2048}, {4096, 2048}, {1, 1}};  // + 1
    CHECK(make_plan(at, 8, false, true).total_terms == kMaxTerms);
    CHECK(make_plan(at, 8, false, true).route == kRouteShared);
    CHECK(make_plan(over, 8, false, true).total_terms == kMaxTerms + 1);
    CHECK(make_plan(over, 8, false, true).route == kRouteLone);
    CHECK(make_plan(over, 8, false, false).route == kRouteShared);
    CHECK(route_of(false, true, 2, kMaxTerms, 10) == kRouteShared && route_of(false, true, 2, kMaxTerms + 1, 10) == kRouteLone);
    CHECK(route_of(false, false, 2, 0, kMaxBlocks) == kRouteShared && route_of(false, false, 2, 0, kMaxBlocks + 1) == kRouteLone);
  }
  std::printf("ok score batch plan\n");
  return 0;
}
