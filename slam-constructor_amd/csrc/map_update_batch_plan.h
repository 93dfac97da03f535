// map_update_batch_plan.h -- the planning of slamhip_map_append_scan_batch (K scans into K resident maps through shared
// launches of the gather kernels, map_update_gather.h).  Pure host arithmetic, no HIP: which jobs share a launch
// (rounds), which go through the lone call and where, how a map's window grows, where every job's buffers lie in the
// per-context arena, and which workgroups of the two flat grids belong to which job.
// tests/native/map_update_batch_plan_test.cpp compiles this header alone with g++.
#pragma once

#include <algorithm>
#include <cstddef>
#include <vector>

#if defined(__HIPCC__)
#define SLAMHIP_PLAN_HD __host__ __device__
#else
#define SLAMHIP_PLAN_HD
#endif

namespace slamhip {
namespace mu_plan {

constexpr size_t kAlign = 256;  // every slice of the arena starts on a multiple of this (bytes)
inline size_t align_up(size_t x, size_t a = kAlign) { return (x + a - 1) / a * a; }

// capacities grow by doubling from `floor_` (never shrink)
inline size_t grow_capacity(size_t current, size_t need, size_t floor_) {
  size_t cap = std::max(current, std::max(floor_, (size_t)1));
  while (cap < need) cap *= 2;
  return cap;
}

// ---- rounds -------------------------------------------------------------------------------------------------------
// A job is EMPTY (n <= 0 or every beam range-gated: takes no part), LONE (the shared launches do not cover it: it runs
// through the lone entry point) or shared.  Steps run in the order of the list.  A round holds jobs on distinct maps;
// a job whose map the open round already holds closes that round (so the two updates of one map keep job order); a
// lone job on a map of the open round closes it too, otherwise it simply runs in front of the open round -- the maps
// differ, so their order does not matter, and per map the order of the jobs is the order of the steps.
struct JobKind {
  int map_id;
  bool lone, empty;
};
struct Step {
  bool lone;
  std::vector<int> jobs;  // a lone step: one job
};
inline std::vector<Step> plan_steps(const std::vector<JobKind> &jobs) {
  std::vector<Step> steps;
  Step open{false, {}};
  std::vector<int> open_maps;
  auto holds = [&](int map_id) { return std::find(open_maps.begin(), open_maps.end(), map_id) != open_maps.end(); };
  auto close = [&]() {
    if (!open.jobs.empty()) steps.push_back(open);
    open.jobs.clear();
    open_maps.clear();
  };
  for (int k = 0; k < (int)jobs.size(); ++k) {
    const JobKind &j = jobs[k];
    if (j.empty) continue;
    if (holds(j.map_id)) close();
    if (j.lone) {
      steps.push_back(Step{true, {k}});
      continue;
    }
    open.jobs.push_back(k);
    open_maps.push_back(j.map_id);
  }
  close();
  return steps;
}

// ---- windows ------------------------------------------------------------------------------------------------------
struct Window {
  int width, height, origin_x, origin_y;
};
struct CellBox {  // external cells an update can touch: the robot's cell and the beams' end cells
  int lo_x, lo_y, hi_x, hi_y;
};
// growth of an unbounded map by the lone rule: the window grows to hold the box, by a fifth of the side or by what
// the box needs, whichever is more, on the sides the box leaves.  0: unchanged, 1: grown, -1: beyond 2^31 cells.
inline int grow_window(Window *w, const CellBox &bb) {
  const long long lo_x = (long long)bb.lo_x + w->origin_x, hi_x = (long long)bb.hi_x + w->origin_x;
  const long long lo_y = (long long)bb.lo_y + w->origin_y, hi_y = (long long)bb.hi_y + w->origin_y;
  if (!(lo_x < 0 || lo_y < 0 || hi_x >= w->width || hi_y >= w->height)) return 0;
  auto side = [](long long need, int dim) { return need > 0 ? std::max(need, (long long)dim / 5 + 1) : 0ll; };
  const long long px = side(-lo_x, w->width), ax = side(hi_x - (w->width - 1), w->width);
  const long long py = side(-lo_y, w->height), ay = side(hi_y - (w->height - 1), w->height);
  const long long nw = px + w->width + ax, nh = py + w->height + ay;
  if (nw * nh > (1ll << 31)) return -1;
  *w = Window{(int)nw, (int)nh, w->origin_x + (int)px, w->origin_y + (int)py};
  return 1;
}
// the key window of an update: the box in internal cells, clipped to the map (n_bins 0: nothing inside)
struct KeyWindow {
  int x0, y0, w, h;
  long long n_bins;
};
inline KeyWindow key_window(const Window &m, const CellBox &bb) {
  const long long x0 = std::max(0ll, (long long)bb.lo_x + m.origin_x), y0 = std::max(0ll, (long long)bb.lo_y + m.origin_y);
  const long long x1 = std::min((long long)m.width - 1, (long long)bb.hi_x + m.origin_x);
  const long long y1 = std::min((long long)m.height - 1, (long long)bb.hi_y + m.origin_y);
  if (x1 < x0 || y1 < y0) return KeyWindow{0, 0, 0, 0, 0};
  return KeyWindow{(int)x0, (int)y0, (int)(x1 - x0 + 1), (int)(y1 - y0 + 1), (x1 - x0 + 1) * (y1 - y0 + 1)};
}

// ---- arena --------------------------------------------------------------------------------------------------------
// One device allocation per context, carved per job of a round.  Its head is the UPLOAD region -- what the host sends:
// scan block, point flags, the first key slot of every beam -- mirrored by one pinned staging block and filled by one
// copy; behind it the work buffers of the kernels.  The irregular-marker words live in a pool of their own: they are
// all zero between calls (the cells that find one set clear it), which a region re-carved by every call could not
// promise.
struct JobShape {
  int n;                // beams
  unsigned total;       // key slots: the sum of the beams' walk lengths
  long long n_bins;     // cells of the key window
};
struct JobSlices {
  // upload region (byte offsets; the same in the staging block and in the arena)
  size_t scan;          // range | cos | sin | quality: 4 n doubles
  size_t occ;           // n ints
  size_t host_offsets;  // n unsigned
  // work region (byte offsets from the arena's start)
  size_t lines, beam_end, beam_inv, beam_info, counts, offsets, keys, bad;
  size_t irr;           // WORD offset into the marker pool (n_bins + 1 words)
};
struct ArenaLayout {
  std::vector<JobSlices> jobs;
  size_t upload_bytes = 0, arena_bytes = 0, irr_words = 0;
};
inline ArenaLayout plan_arena(const std::vector<JobShape> &shapes, size_t sizeof_line, size_t sizeof_beam) {
  ArenaLayout L;
  L.jobs.resize(shapes.size());
  size_t at = 0;
  auto take = [&](size_t bytes) {
    const size_t here = at;
    at = align_up(at + bytes);
    return here;
  };
  for (size_t k = 0; k < shapes.size(); ++k) {
    const size_t n = (size_t)std::max(shapes[k].n, 0);
    L.jobs[k].scan = take(4 * n * sizeof(double));
    L.jobs[k].occ = take(n * sizeof(int));
    L.jobs[k].host_offsets = take(n * sizeof(unsigned));
  }
  L.upload_bytes = at;
  size_t irr = 0;
  for (size_t k = 0; k < shapes.size(); ++k) {
    const size_t n = (size_t)std::max(shapes[k].n, 0);
    JobSlices &s = L.jobs[k];
    s.lines = take(n * sizeof_line);
    s.beam_end = take(2 * n * sizeof(double));
    s.beam_inv = take(2 * n * sizeof(double));
    s.beam_info = take(n * sizeof_beam);
    s.counts = take(n * sizeof(unsigned));
    s.offsets = take((n + 1) * sizeof(unsigned));
    s.keys = take((size_t)shapes[k].total * sizeof(unsigned));
    s.bad = take(((n + 7) & ~(size_t)7) + 8);  // (read eight beams at a time)
    s.irr = irr;
    irr += (size_t)std::max(shapes[k].n_bins, 0ll) + 1;
  }
  L.arena_bytes = at;
  L.irr_words = irr;
  return L;
}

// ---- grids --------------------------------------------------------------------------------------------------------
// Both launches are FLAT: job after job, a job's workgroups side by side (k_mu_lines: one per beam; k_mu_cells: the
// near workgroups of the job, four cells each, in front of its far ones, 16 x 16 cells each).  A table of K + 1
// first-workgroup numbers says where a job starts; a workgroup finds its job by bisection.  (grid.y = job would
// launch max-over-jobs workgroups for every job: windows differ by an order of magnitude between robots.)
struct JobGrid {
  unsigned line_blocks, near_blocks, far_blocks;
};
inline JobGrid job_grid(int n, int key_w, int key_h, int near_r) {
  const unsigned side = 2u * (unsigned)near_r + 1u;
  return JobGrid{(unsigned)n, (side * side + 3u) / 4u, (unsigned)(((key_w + 15) / 16) * ((key_h + 15) / 16))};
}
struct GridPlan {
  std::vector<unsigned> line_off, cell_off;  // K + 1 entries each; the last one is the grid size
  bool fits = true;                          // both grids below 2^31 workgroups
};
inline GridPlan plan_grid(const std::vector<JobGrid> &jobs) {
  GridPlan g;
  unsigned long long lines = 0, cells = 0;
  for (const JobGrid &j : jobs) {
    g.line_off.push_back((unsigned)lines);
    g.cell_off.push_back((unsigned)cells);
    lines += j.line_blocks;
    cells += (unsigned long long)j.near_blocks + j.far_blocks;
  }
  g.line_off.push_back((unsigned)lines);
  g.cell_off.push_back((unsigned)cells);
  g.fits = lines < (1ull << 31) && cells < (1ull << 31);
  return g;
}
// the job of workgroup `block`: the last j with off[j] <= block (off ascends, off[0] = 0, block < off[n_jobs]);
// jobs without workgroups (off[j] == off[j + 1]) are never returned
SLAMHIP_PLAN_HD inline int find_job(const unsigned *off, int n_jobs, unsigned block) {
  int lo = 0, hi = n_jobs;  // off[lo] <= block < off[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (off[mid] <= block) lo = mid;
    else hi = mid;
  }
  return lo;
}

}  // namespace mu_plan
}  // namespace slamhip
