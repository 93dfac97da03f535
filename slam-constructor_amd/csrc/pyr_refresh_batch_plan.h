// pyr_refresh_batch_plan.h -- the planning of slamhip_pyramid_refresh_batch (K pyramids refreshed through shared
// launches, map_pyramid.hip).  Pure host arithmetic, no HIP: which jobs share a round, which go through the lone call,
// every job's clipped window per level, where a job leaves the flat per-level launches for the one-workgroup tail, which
// workgroups of a flat grid belong to which job, and where everything lies in the job table the kernels read.
// tests/native/pyr_refresh_batch_plan_test.cpp compiles this header alone with g++.
#pragma once

#include <algorithm>
#include <cstddef>
#include <vector>

#if defined(__HIPCC__)
#define SLAMHIP_PYR_PLAN_HD __host__ __device__
#else
#define SLAMHIP_PYR_PLAN_HD
#endif

namespace slamhip {
namespace pyr_plan {

constexpr int kThreads = 256;   // threads of a workgroup of both kernels (kPyrThreads)
constexpr size_t kAlign = 256;  // every part of the table starts on a multiple of this (bytes)
inline size_t align_up(size_t x, size_t a = kAlign) { return (x + a - 1) / a * a; }

// ---- jobs ---------------------------------------------------------------------------------------------------------
struct LevelGeom {  // one level above the fine map, as pyr::plan_levels planned it
  int width, height, origin_x, origin_y;
};
struct Job {
  int pyramid;              // equal for jobs that name the same pyramid, different otherwise
  int n_levels;             // levels above the fine map; the last one is the 1 x 1 level
  const LevelGeom *levels;  // n_levels of them
  int fine_w, fine_h, fine_ox, fine_oy;
  int x0, y0, w, h;  // INTERNAL fine window
  bool stale;        // the pyramid's maps are not the ones its levels were made over
  bool lone;         // a level carries a probability plane: the shared launches do not keep it
};
struct Window {  // cells [cx0, cx0 + cw) x [cy0, cy0 + ch) of a level, internal
  int cx0, cy0, cw, ch;
  long long cells() const { return (long long)cw * ch; }
};

inline bool window_inside(const Job &j) {
  return j.w > 0 && j.h > 0 && j.x0 >= 0 && j.y0 >= 0 && (long long)j.x0 + j.w <= j.fine_w && (long long)j.y0 + j.h <= j.fine_h;
}

// the cells of level lv (1-based) whose blocks meet the job's fine window, clipped to the level: floor(x / 2^lv) of the
// EXTERNAL coordinates of the window's corners (pyr::level_window); the top level is its one cell.  False: none.
inline bool level_window(const Job &j, int lv, Window *out) {
  const LevelGeom &g = j.levels[lv - 1];
  long long cx0 = 0, cy0 = 0, cx1 = 0, cy1 = 0;
  if (lv != j.n_levels) {
    cx0 = (long long)((j.x0 - j.fine_ox) >> lv) + g.origin_x;
    cx1 = (long long)((j.x0 + j.w - 1 - j.fine_ox) >> lv) + g.origin_x;
    cy0 = (long long)((j.y0 - j.fine_oy) >> lv) + g.origin_y;
    cy1 = (long long)((j.y0 + j.h - 1 - j.fine_oy) >> lv) + g.origin_y;
  }
  cx0 = std::max(cx0, 0ll);
  cy0 = std::max(cy0, 0ll);
  cx1 = std::min(cx1, (long long)g.width - 1);
  cy1 = std::min(cy1, (long long)g.height - 1);
  if (cx1 < cx0 || cy1 < cy0) return false;
  *out = Window{(int)cx0, (int)cy0, (int)(cx1 - cx0 + 1), (int)(cy1 - cy0 + 1)};
  return true;
}

// ---- the plan -----------------------------------------------------------------------------------------------------
// Steps run in the order of the list, so per pyramid the order of the jobs is the order of the steps.  A round holds
// jobs on distinct pyramids (within one launch a second window's level-2 cells could read level-1 cells the first is
// writing): a job whose pyramid the open round holds closes it.  A lone job closes the open round and runs at its place.
//
// A round's launches: one FLAT launch per level for the jobs whose window at that level has more than kThreads cells --
// job after job, ceil(cells / kThreads) workgroups each, block_off saying where a job's begin -- and one TAIL launch, a
// workgroup per job walking the job's levels from tail_from (the first with at most kThreads cells; a level's window
// never has more cells than the one below it) to the top.
//
// The table (one per call, every round's parts in it): the entries -- one per (job, level), a flat launch's side by
// side, then a job's tail run side by side --, the block offsets of the flat launches, the tail runs (first entry, count).
struct EntryRef {
  int job, level;
  Window win;
};
struct FlatLaunch {
  int level;
  std::vector<int> jobs;            // of the call
  std::vector<unsigned> block_off;  // jobs + 1 entries; the last one is the grid size
  size_t entry_at, off_at;          // index of the first entry / of block_off[0] among the table's offsets
};
struct TailRun {
  int job, tail_from;
  size_t entry_at;
  int n_entries;
};
struct Step {
  bool lone;
  std::vector<int> jobs;  // a lone step: one job
  std::vector<FlatLaunch> flat;
  std::vector<TailRun> tail;  // one per job, in job order
  size_t run_at;              // index of the first tail run among the table's runs
};
struct Stats {
  int rounds = 0, jobs_shared = 0, jobs_lone = 0, launches = 0;  // launches: of the shared rounds
};
struct Plan {
  std::vector<Step> steps;
  std::vector<EntryRef> entries;
  size_t n_offsets = 0, n_runs = 0;
  // the table in bytes: entries | offsets (unsigned) | runs (two ints each)
  size_t off_bytes_at = 0, run_bytes_at = 0, table_bytes = 0;
  Stats stats;
};

enum { kOk = 0, kStale = 1, kWindow = 2, kTooLarge = 3 };

// Plans a call.  A refusal (a stale pyramid, a window outside its fine map -- in job order, the first one found -- or a
// flat grid of 2^31 workgroups) leaves *out as it was.
inline int plan_call(const std::vector<Job> &jobs, size_t sizeof_entry, Plan *out) {
  for (const Job &j : jobs) {
    if (j.stale) return kStale;
    if (!window_inside(j)) return kWindow;
  }
  Plan p;
  auto plan_round = [&](Step *st) -> bool {
    int top_flat = 0;
    std::vector<std::vector<Window>> win(st->jobs.size());
    std::vector<int> tail_from(st->jobs.size());
    for (size_t k = 0; k < st->jobs.size(); ++k) {
      const Job &j = jobs[st->jobs[k]];
      win[k].resize(j.n_levels + 1);
      tail_from[k] = j.n_levels;
      for (int lv = j.n_levels; lv >= 1; --lv) {
        if (!level_window(j, lv, &win[k][lv])) win[k][lv] = Window{0, 0, 0, 0};  // (cannot happen for a window inside)
        if (win[k][lv].cells() <= kThreads && tail_from[k] == lv + 1) tail_from[k] = lv;
      }
      // (the top level is one cell, so the scan above starts a tail there; it has grown downwards while the windows fit)
      top_flat = std::max(top_flat, tail_from[k] - 1);
    }
    for (int lv = 1; lv <= top_flat; ++lv) {
      FlatLaunch f;
      f.level = lv;
      f.entry_at = p.entries.size();
      f.off_at = p.n_offsets;
      unsigned long long blocks = 0;
      for (size_t k = 0; k < st->jobs.size(); ++k) {
        if (lv >= tail_from[k]) continue;
        f.jobs.push_back(st->jobs[k]);
        f.block_off.push_back((unsigned)blocks);
        blocks += (unsigned long long)((win[k][lv].cells() + kThreads - 1) / kThreads);
        p.entries.push_back(EntryRef{st->jobs[k], lv, win[k][lv]});
      }
      if (blocks >= (1ull << 31)) return false;
      f.block_off.push_back((unsigned)blocks);
      p.n_offsets += f.block_off.size();
      st->flat.push_back(f);
    }
    st->run_at = p.n_runs;
    for (size_t k = 0; k < st->jobs.size(); ++k) {
      const Job &j = jobs[st->jobs[k]];
      TailRun t{st->jobs[k], tail_from[k], p.entries.size(), j.n_levels - tail_from[k] + 1};
      for (int lv = tail_from[k]; lv <= j.n_levels; ++lv) p.entries.push_back(EntryRef{st->jobs[k], lv, win[k][lv]});
      st->tail.push_back(t);
    }
    p.n_runs += st->tail.size();
    p.stats.rounds += 1;
    p.stats.jobs_shared += (int)st->jobs.size();
    p.stats.launches += (int)st->flat.size() + 1;
    return true;
  };
  Step open{false, {}, {}, {}, 0};
  auto holds = [&](int pyramid) {
    for (int k : open.jobs)
      if (jobs[k].pyramid == pyramid) return true;
    return false;
  };
  auto close = [&]() -> bool {
    if (open.jobs.empty()) return true;
    if (!plan_round(&open)) return false;
    p.steps.push_back(open);
    open = Step{false, {}, {}, {}, 0};
    return true;
  };
  for (int k = 0; k < (int)jobs.size(); ++k) {
    if (jobs[k].lone || holds(jobs[k].pyramid)) {
      if (!close()) return kTooLarge;
    }
    if (jobs[k].lone) {
      p.steps.push_back(Step{true, {k}, {}, {}, 0});
      p.stats.jobs_lone += 1;
      continue;
    }
    open.jobs.push_back(k);
  }
  if (!close()) return kTooLarge;
  p.off_bytes_at = align_up(p.entries.size() * sizeof_entry);
  p.run_bytes_at = align_up(p.off_bytes_at + p.n_offsets * sizeof(unsigned));
  p.table_bytes = align_up(p.run_bytes_at + p.n_runs * 2 * sizeof(int));
  *out = std::move(p);
  return kOk;
}

// the job of workgroup `block` of a flat launch: the last j with off[j] <= block (off ascends, off[0] = 0,
// block < off[n_jobs]; every job of a flat launch has at least one workgroup)
SLAMHIP_PYR_PLAN_HD inline int find_job(const unsigned *off, int n_jobs, unsigned block) {
  int lo = 0, hi = n_jobs;  // off[lo] <= block < off[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (off[mid] <= block) lo = mid;
    else hi = mid;
  }
  return lo;
}

}  // namespace pyr_plan
}  // namespace slamhip
