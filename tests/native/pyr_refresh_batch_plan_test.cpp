// Native test of csrc/pyr_refresh_batch_plan.h (the planning of slamhip_pyramid_refresh_batch): plain C++, run as an
// ordinary executable by tests/test_pyr_refresh_plan_host.py, plainly and under -fsanitize=address,undefined.
#include <algorithm>
#include <cstdio>
#include <map>
#include <utility>
#include <vector>

#include "pyr_refresh_batch_plan.h"

using namespace slamhip::pyr_plan;

static int g_failed = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);  \
      ++g_failed;                                                    \
    }                                                                \
  } while (0)

// the levels over a fine map of w x h cells with external (0, 0) at internal (ox, oy), by the rule of include/slamhip.h
// "map pyramid": halving levels with tight windows up to the first k with 2^k >= max(ox, w - ox, oy, h - oy), then 1 x 1
struct Pyramid {
  int w, h, ox, oy;
  std::vector<LevelGeom> levels;
};
static Pyramid make_pyramid(int w, int h, int ox, int oy) {
  Pyramid p{w, h, ox, oy, {}};
  const long long x_lo = -ox, x_hi = w - 1 - ox, y_lo = -oy, y_hi = h - 1 - oy;
  int k_last = 0;
  while (x_lo < -(1ll << k_last) || x_hi >= (1ll << k_last) || y_lo < -(1ll << k_last) || y_hi >= (1ll << k_last)) ++k_last;
  for (int k = 1; k <= k_last; ++k) {
    const int X0 = (int)x_lo >> k, X1 = (int)x_hi >> k, Y0 = (int)y_lo >> k, Y1 = (int)y_hi >> k;
    p.levels.push_back(LevelGeom{X1 - X0 + 1, Y1 - Y0 + 1, -X0, -Y0});
  }
  p.levels.push_back(LevelGeom{1, 1, 0, 0});
  return p;
}
static Job job_of(const Pyramid &p, int key, int x0, int y0, int w, int h) {
  return Job{key, (int)p.levels.size(), p.levels.data(), p.w, p.h, p.ox, p.oy, x0, y0, w, h, false, false};
}

// floor(v / 2^k) without a shift: what the plan's windows must agree with
static long long floor_div_pow2(long long v, int k) {
  const long long d = 1ll << k;
  return v >= 0 ? v / d : -((-v + d - 1) / d);
}

static const size_t kEntry = 144;  // (any entry size: the layout is in units of it)

// Every property of a plan the kernels rely on.
static void check_plan(const std::vector<Job> &jobs, const Plan &pl) {
  // who computes (job, level, cell): exactly one entry
  std::map<std::pair<int, int>, std::vector<int>> assigned;  // (job, level) -> count per cell of the level
  int rounds = 0, shared = 0, lone = 0, launches = 0;
  std::vector<int> seen_job(jobs.size(), 0);
  size_t next_off = 0, next_run = 0, next_entry = 0;
  for (size_t s = 0; s < pl.steps.size(); ++s) {
    const Step &st = pl.steps[s];
    if (st.lone) {
      CHECK(st.jobs.size() == 1 && jobs[st.jobs[0]].lone && st.flat.empty() && st.tail.empty());
      ++lone;
      seen_job[st.jobs[0]] += 1;
      continue;
    }
    ++rounds;
    shared += (int)st.jobs.size();
    launches += (int)st.flat.size() + 1;
    // equal pyramids never share a round; job order is kept
    for (size_t a = 0; a < st.jobs.size(); ++a) {
      seen_job[st.jobs[a]] += 1;
      CHECK(!jobs[st.jobs[a]].lone);
      for (size_t b = a + 1; b < st.jobs.size(); ++b) {
        CHECK(jobs[st.jobs[a]].pyramid != jobs[st.jobs[b]].pyramid);
        CHECK(st.jobs[a] < st.jobs[b]);
      }
    }
    CHECK(st.tail.size() == st.jobs.size());
    int want_level = 1;
    for (const FlatLaunch &f : st.flat) {
      CHECK(f.level == want_level++);
      CHECK(!f.jobs.empty() && f.block_off.size() == f.jobs.size() + 1);
      CHECK(f.entry_at == next_entry && f.off_at == next_off);
      next_off += f.block_off.size();
      // block offsets partition the grid: job k has ceil(cells / kThreads) >= 1 workgroups, found by bisection
      CHECK(f.block_off[0] == 0);
      for (size_t k = 0; k < f.jobs.size(); ++k) {
        const EntryRef &e = pl.entries[f.entry_at + k];
        CHECK(e.job == f.jobs[k] && e.level == f.level);
        CHECK(e.win.cells() > kThreads);
        const unsigned blocks = (unsigned)((e.win.cells() + kThreads - 1) / kThreads);
        CHECK(f.block_off[k + 1] - f.block_off[k] == blocks);
        CHECK(find_job(f.block_off.data(), (int)f.jobs.size(), f.block_off[k]) == (int)k);
        CHECK(find_job(f.block_off.data(), (int)f.jobs.size(), f.block_off[k + 1] - 1) == (int)k);
        // the job's tail starts above this level
        for (const TailRun &t : st.tail)
          if (t.job == e.job) CHECK(t.tail_from > f.level);
      }
      next_entry += f.jobs.size();
    }
    CHECK(st.run_at == next_run);
    next_run += st.tail.size();
    for (size_t k = 0; k < st.tail.size(); ++k) {
      const TailRun &t = st.tail[k];
      const Job &j = jobs[t.job];
      CHECK(t.job == st.jobs[k] && t.entry_at == next_entry && t.n_entries == j.n_levels - t.tail_from + 1 && t.n_entries >= 1);
      // the tail starts at the FIRST level whose clipped window has at most kThreads cells and runs to the top
      for (int lv = 1; lv <= j.n_levels; ++lv) {
        Window w{};
        CHECK(level_window(j, lv, &w));
        CHECK((w.cells() <= kThreads) == (lv >= t.tail_from));
      }
      for (int i = 0; i < t.n_entries; ++i) {
        const EntryRef &e = pl.entries[t.entry_at + i];
        CHECK(e.job == t.job && e.level == t.tail_from + i && e.win.cells() <= kThreads && e.win.cells() >= 1);
      }
      CHECK(pl.entries[t.entry_at + t.n_entries - 1].level == j.n_levels);
      next_entry += (size_t)t.n_entries;
    }
  }
  CHECK(next_entry == pl.entries.size() && next_off == pl.n_offsets && next_run == pl.n_runs);
  for (int c : seen_job) CHECK(c == 1);
  CHECK(pl.stats.rounds == rounds && pl.stats.jobs_shared == shared && pl.stats.jobs_lone == lone && pl.stats.launches == launches);
  // per pyramid the order of the jobs is the order of the steps
  std::vector<int> order;
  for (const Step &st : pl.steps)
    for (int k : st.jobs) order.push_back(k);
  for (size_t a = 0; a < order.size(); ++a)
    for (size_t b = a + 1; b < order.size(); ++b)
      if (jobs[order[a]].pyramid == jobs[order[b]].pyramid) CHECK(order[a] < order[b]);
  // the table: parts in order, aligned, no overlap
  CHECK(pl.off_bytes_at % kAlign == 0 && pl.run_bytes_at % kAlign == 0 && pl.table_bytes % kAlign == 0);
  CHECK(pl.off_bytes_at >= pl.entries.size() * kEntry);
  CHECK(pl.run_bytes_at >= pl.off_bytes_at + pl.n_offsets * sizeof(unsigned));
  CHECK(pl.table_bytes >= pl.run_bytes_at + pl.n_runs * 2 * sizeof(int));
  // every coarse cell whose block meets a job's window is assigned exactly once, and no other cell is
  for (const EntryRef &e : pl.entries) {
    const Job &j = jobs[e.job];
    const LevelGeom &g = j.levels[e.level - 1];
    std::vector<int> &cnt = assigned[{e.job, e.level}];
    cnt.resize((size_t)g.width * g.height, 0);
    CHECK(e.win.cx0 >= 0 && e.win.cy0 >= 0 && e.win.cx0 + e.win.cw <= g.width && e.win.cy0 + e.win.ch <= g.height);
    for (int y = 0; y < e.win.ch; ++y)
      for (int x = 0; x < e.win.cw; ++x) cnt[(size_t)(e.win.cy0 + y) * g.width + (e.win.cx0 + x)] += 1;
  }
  for (size_t k = 0; k < jobs.size(); ++k) {
    const Job &j = jobs[k];
    if (j.lone) continue;
    for (int lv = 1; lv <= j.n_levels; ++lv) {
      const LevelGeom &g = j.levels[lv - 1];
      std::vector<int> want((size_t)g.width * g.height, 0);
      for (int y = j.y0; y < j.y0 + j.h; ++y)
        for (int x = j.x0; x < j.x0 + j.w; ++x) {
          const long long cx = lv == j.n_levels ? 0 : floor_div_pow2(x - j.fine_ox, lv) + g.origin_x;
          const long long cy = lv == j.n_levels ? 0 : floor_div_pow2(y - j.fine_oy, lv) + g.origin_y;
          CHECK(cx >= 0 && cy >= 0 && cx < g.width && cy < g.height);
          want[(size_t)cy * g.width + (size_t)cx] = 1;
        }
      CHECK((assigned[{(int)k, lv}]) == want);
    }
  }
}

static bool same_plan(const Plan &a, const Plan &b) {
  if (a.entries.size() != b.entries.size() || a.steps.size() != b.steps.size() || a.n_offsets != b.n_offsets ||
      a.n_runs != b.n_runs || a.table_bytes != b.table_bytes || a.off_bytes_at != b.off_bytes_at || a.run_bytes_at != b.run_bytes_at)
    return false;
  if (a.stats.rounds != b.stats.rounds || a.stats.jobs_shared != b.stats.jobs_shared || a.stats.jobs_lone != b.stats.jobs_lone ||
      a.stats.launches != b.stats.launches)
    return false;
  for (size_t i = 0; i < a.entries.size(); ++i) {
    const EntryRef &x = a.entries[i], &y = b.entries[i];
    if (x.job != y.job || x.level != y.level || x.win.cx0 != y.win.cx0 || x.win.cy0 != y.win.cy0 || x.win.cw != y.win.cw ||
        x.win.ch != y.win.ch)
      return false;
  }
  return true;
}

int main() {
  const Pyramid big = make_pyramid(37, 29, 11, 20), small = make_pyramid(9, 9, 4, 5), oblong = make_pyramid(520, 12, 3, 9),
                tiny = make_pyramid(2, 2, 1, 1), bench = make_pyramid(2000, 2000, 1000, 1000), corner = make_pyramid(600, 600, 0, 0);
  CHECK(tiny.levels.size() == 1 && bench.levels.size() == 11);
  CHECK(oblong.levels[0].width == 261);  // external x in [-3, 516]: level-1 cells -2 .. 258

  // ---- one job per shape and window; whole maps, corners, windows across the external axes
  {
    std::vector<Job> jobs = {job_of(big, 0, 0, 0, 37, 29),      job_of(small, 1, 0, 0, 1, 1),   job_of(oblong, 2, 0, 0, 520, 12),
                             job_of(tiny, 3, 0, 0, 2, 2),       job_of(bench, 4, 700, 700, 600, 600),
                             job_of(corner, 5, 599, 599, 1, 1)};
    Plan pl;
    CHECK(plan_call(jobs, kEntry, &pl) == kOk);
    check_plan(jobs, pl);
    CHECK(pl.stats.rounds == 1 && pl.stats.jobs_shared == 6 && pl.stats.jobs_lone == 0);
    // the 600 x 600 window: 300^2, 150^2, 76^2, 38^2, 20^2 = 400 cells flat, 10^2 = 100 in the tail
    CHECK(pl.steps[0].tail[4].tail_from == 6 && pl.steps[0].flat.size() == 5 && pl.stats.launches == 6);
    CHECK(pl.steps[0].flat[0].jobs.size() == 3);  // big, oblong, bench: level 1 above 256 cells; small, tiny, corner not
  }
  // ---- level windows of exactly 256 and 257 cells on either side of the split (the oblong map, one row of level 1)
  {
    // fine x in [1, 512] internal = external [-2, 509]: level-1 cells -1 .. 254 = 256 cells; one more fine column: 257
    std::vector<Job> jobs = {job_of(oblong, 0, 1, 9, 512, 1)};
    Plan pl;
    CHECK(plan_call(jobs, kEntry, &pl) == kOk);
    check_plan(jobs, pl);
    Window w{};
    CHECK(level_window(jobs[0], 1, &w) && w.cells() == 256);
    CHECK(pl.steps[0].flat.empty() && pl.steps[0].tail[0].tail_from == 1 && pl.stats.launches == 1);
    jobs = {job_of(oblong, 0, 1, 9, 514, 1)};
    CHECK(plan_call(jobs, kEntry, &pl) == kOk);
    check_plan(jobs, pl);
    CHECK(level_window(jobs[0], 1, &w) && w.cells() == 257);
    CHECK(pl.steps[0].flat.size() == 1 && pl.steps[0].flat[0].block_off.back() == 2 && pl.steps[0].tail[0].tail_from == 2);
  }
  // ---- rounds: equal pyramids never share one; a lone job runs at its place
  {
    Job lone = job_of(small, 1, 2, 2, 3, 3);
    lone.lone = true;
    std::vector<Job> jobs = {job_of(big, 0, 0, 0, 5, 5), job_of(small, 1, 0, 0, 9, 9), job_of(big, 0, 30, 20, 7, 9),
                             job_of(bench, 2, 0, 0, 2000, 2000), lone, job_of(small, 1, 8, 8, 1, 1), job_of(big, 0, 3, 3, 1, 1),
                             job_of(big, 0, 3, 3, 2, 2)};
    Plan pl;
    CHECK(plan_call(jobs, kEntry, &pl) == kOk);
    check_plan(jobs, pl);
    CHECK(pl.stats.rounds == 4 && pl.stats.jobs_lone == 1 && pl.stats.jobs_shared == 7);
    CHECK(pl.steps.size() == 5 && pl.steps[2].lone);
    // ---- a refused call leaves the plan as it was
    const Plan before = pl;
    std::vector<Job> bad = jobs;
    bad[6].stale = true;
    CHECK(plan_call(bad, kEntry, &pl) == kStale && same_plan(pl, before));
    const int outside[][4] = {{-1, 0, 2, 2}, {0, -1, 2, 2}, {36, 0, 2, 1}, {0, 28, 1, 2}, {0, 0, 0, 1}, {0, 0, 1, 0}, {0, 0, 38, 1},
                              {2147483647, 0, 2, 1}};
    for (const auto &o : outside) {
      bad = jobs;
      bad[2] = job_of(big, 0, o[0], o[1], o[2], o[3]);
      CHECK(plan_call(bad, kEntry, &pl) == kWindow && same_plan(pl, before));
    }
    CHECK(plan_call(jobs, kEntry, &pl) == kOk && same_plan(pl, before));  // (and the same jobs plan the same)
  }
  // ---- no jobs: an empty plan
  {
    Plan pl;
    CHECK(plan_call({}, kEntry, &pl) == kOk);
    CHECK(pl.steps.empty() && pl.entries.empty() && pl.stats.launches == 0 && pl.table_bytes == 0);
  }
  // ---- every window of a small off-centre map
  {
    const Pyramid p = make_pyramid(13, 7, 9, 2);
    for (int x0 = 0; x0 < 13; x0 += 2)
      for (int y0 = 0; y0 < 7; ++y0)
        for (int w = 1; x0 + w <= 13; w += 3)
          for (int h = 1; y0 + h <= 7; h += 2) {
            std::vector<Job> jobs = {job_of(p, 0, x0, y0, w, h)};
            Plan pl;
            CHECK(plan_call(jobs, kEntry, &pl) == kOk);
            check_plan(jobs, pl);
          }
  }
  if (g_failed) {
    std::printf("%d checks failed\n", g_failed);
    return 1;
  }
  std::printf("ok pyr refresh batch plan\n");
  return 0;
}
