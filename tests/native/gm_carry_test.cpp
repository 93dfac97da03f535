// gm_carry_test.cpp -- csrc/gm_carry.h alone, with a host compiler: the walk that carries the GMapping OOPE's run cache
// from pose to pose over the scoring kernels' side outputs, against a plain per-beam simulation of the reference's cache
// (GmappingOccupancyObservationPE: one cached coordinate and one cached value; a beam whose end cell repeats the cached
// coordinate takes the cached value, any other beam takes its fresh value and caches it).
//
// The kernels score every pose from an EMPTY cache; the simulation gives that too (the cache emptied in front of every
// pose): from it the side outputs (GmPoseInfo) and the scores the walk starts from.  The simulation with the cache kept
// over the job's poses gives what the walk has to arrive at.  All values, weights and factors are small dyadic
// rationals and tot_w a power of two (or 0), so every sum and quotient here is exact and the comparison is bit for bit
// whatever the order of the additions.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gm_carry.h"

using namespace slamhip;

#define CHECK(cond)                                                         \
  do {                                                                      \
    if (!(cond)) {                                                          \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);         \
      std::exit(1);                                                         \
    }                                                                       \
  } while (0)

static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd(uint32_t below) {
  g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(g_state >> 33) % below;
}

struct Cell {
  int x, y;
};
struct RefCache {  // the reference's two members; `has`: anything cached yet
  bool has = false;
  Cell at{0, 0};
  double v = 0.0;
  double value(Cell c, double fresh) {
    if (has && c.x == at.x && c.y == at.y) return v;
    has = true;
    at = c;
    v = fresh;
    return fresh;
  }
};

struct Pose {
  std::vector<Cell> cell;     // end cell per beam
  std::vector<double> fresh;  // the value the beam would compute
};

static double score_of(const std::vector<double> &val, const std::vector<double> &w, const std::vector<double> &f, double tot_w) {
  double acc = 0.0;
  for (size_t b = 0; b < val.size(); ++b) acc = acc + val[b] * w[b] * f[b];
  return tot_w == 0.0 ? std::nan("") : acc / tot_w;
}

static bool same_bits(double a, double b) {
  if (std::isnan(a) || std::isnan(b)) return std::isnan(a) && std::isnan(b);
  return std::memcmp(&a, &b, sizeof(a)) == 0;
}

struct Counts {
  long long jobs = 0, poses = 0, carried = 0, spanning = 0, whole = 0, zero_w = 0, single = 0;
};

// one job: n beams, the given poses
static void check_job(const std::vector<Pose> &poses, const std::vector<double> &w, const std::vector<double> &f, double tot_w,
                      Counts &cnt) {
  const int P = (int)poses.size();
  const int n = (int)w.size();
  std::vector<GmPoseInfo> info((size_t)P);
  std::vector<double> scores((size_t)P), want((size_t)P);
  RefCache kept;  // the job's estimator object
  int want_carried = 0;
  for (int p = 0; p < P; ++p) {
    const Pose &ps = poses[(size_t)p];
    CHECK((int)ps.cell.size() == n && (int)ps.fresh.size() == n);
    // what the kernel sees: an empty cache in front of the pose
    RefCache empty;
    std::vector<double> v0((size_t)n), v1((size_t)n);
    for (int b = 0; b < n; ++b) v0[(size_t)b] = empty.value(ps.cell[(size_t)b], ps.fresh[(size_t)b]);
    GmPoseInfo &gi = info[(size_t)p];
    gi.first_cx = ps.cell[0].x;
    gi.first_cy = ps.cell[0].y;
    gi.last_cx = ps.cell[(size_t)n - 1].x;
    gi.last_cy = ps.cell[(size_t)n - 1].y;
    gi.v0 = ps.fresh[0];
    gi.last_v = v0[(size_t)n - 1];
    int run0 = 1;
    while (run0 < n && ps.cell[(size_t)run0].x == ps.cell[0].x && ps.cell[(size_t)run0].y == ps.cell[0].y) ++run0;
    gi.run0_len = run0;
    int head = n - 1;
    while (head > 0 && ps.cell[(size_t)head - 1].x == ps.cell[(size_t)head].x && ps.cell[(size_t)head - 1].y == ps.cell[(size_t)head].y) --head;
    gi.last_head = head;
    scores[(size_t)p] = score_of(v0, w, f, tot_w);
    // what the reference computes: the cache kept from the pose before
    const bool hit = kept.has && kept.at.x == ps.cell[0].x && kept.at.y == ps.cell[0].y;
    if (hit && kept.v != ps.fresh[0]) {
      ++want_carried;
      if (run0 == n) ++cnt.whole;
      ++cnt.spanning;
    }
    for (int b = 0; b < n; ++b) v1[(size_t)b] = kept.value(ps.cell[(size_t)b], ps.fresh[(size_t)b]);
    want[(size_t)p] = score_of(v1, w, f, tot_w);
  }
  GmCarryCache cr = gm_carry_empty();
  CHECK(cr.prob == -1.0);
  const int got_carried = gm_carry_walk(cr, P, info.data(), w.data(), f.data(), tot_w, scores.data());
  CHECK(got_carried == want_carried);
  for (int p = 0; p < P; ++p) CHECK(same_bits(scores[(size_t)p], want[(size_t)p]));
  if (P == 0) {
    CHECK(cr.prob == -1.0);
  } else {
    CHECK(kept.has && cr.cx == kept.at.x && cr.cy == kept.at.y && same_bits(cr.prob, kept.v));
  }
  cnt.jobs += 1;
  cnt.poses += P;
  cnt.carried += want_carried;
  if (tot_w == 0.0) ++cnt.zero_w;
  if (n == 1) ++cnt.single;
}

static Pose random_pose(int n, const Cell *start, int mode) {
  // mode 0: short runs over a few cells; 1: the whole pose one run; 2: long runs
  Pose ps;
  Cell c = start ? *start : Cell{(int)rnd(3) - 1, (int)rnd(3) - 1};
  for (int b = 0; b < n; ++b) {
    const uint32_t stay = mode == 1 ? 1u : (mode == 2 ? rnd(8) : rnd(2));
    if (b > 0 && !stay) c = Cell{(int)rnd(3) - 1, (int)rnd(3) - 1};  // (may draw the same cell again: the run goes on)
    ps.cell.push_back(c);
    ps.fresh.push_back((double)rnd(65) / 64.0);
  }
  return ps;
}

int main() {
  const double tot_ws[] = {0.0, 0.5, 1.0, 4.0};
  const int pose_counts[] = {0, 1, 2, 7, 8, 9, 16, 17, 40};  // (around the walk's chunk of 8)
  const int beam_counts[] = {1, 2, 3, 17, 40};
  const double ws[] = {0.25, 0.5, 1.0, 2.0}, fs[] = {0.5, 1.0};
  Counts cnt;
  for (int rep = 0; rep < 40; ++rep) {
    for (int P : pose_counts) {
      for (int n : beam_counts) {
        std::vector<double> w((size_t)n), f((size_t)n);
        for (int b = 0; b < n; ++b) {
          w[(size_t)b] = ws[rnd(4)];
          f[(size_t)b] = fs[rnd(2)];
        }
        std::vector<Pose> poses;
        for (int p = 0; p < P; ++p) {
          // half of the poses start in the cell the pose before ended in: a run that spans the pose boundary
          const Cell *start = (p > 0 && rnd(2)) ? &poses.back().cell.back() : nullptr;
          poses.push_back(random_pose(n, start, (int)rnd(3)));
        }
        check_job(poses, w, f, tot_ws[rnd(4)], cnt);
      }
    }
  }
  // three poses that are ONE run each over the same cell: the first pose's value is handed through to the third
  {
    const std::vector<double> w{1.0, 0.5, 2.0}, f{1.0, 1.0, 0.5};
    std::vector<Pose> poses(3);
    const double fresh[3] = {0.25, 0.75, 0.5};
    for (int p = 0; p < 3; ++p)
      for (int b = 0; b < 3; ++b) {
        poses[(size_t)p].cell.push_back(Cell{4, -2});
        poses[(size_t)p].fresh.push_back(b == 0 ? fresh[p] : 0.125);
      }
    Counts one;
    check_job(poses, w, f, 1.0, one);
    CHECK(one.carried == 2 && one.whole == 2);
  }
  CHECK(cnt.carried > 100 && cnt.whole > 10 && cnt.zero_w > 10 && cnt.single > 10 && cnt.poses > cnt.carried);
  std::printf("jobs %lld poses %lld carried %lld whole-pose runs carried %lld\n", cnt.jobs, cnt.poses, cnt.carried, cnt.whole);
  std::printf("ok gm carry\n");
  return 0;
}
