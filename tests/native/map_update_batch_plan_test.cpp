// map_update_batch_plan_test.cpp -- csrc/map_update_batch_plan.h on the host alone: rounds and lone steps over random job
// lists, window growth, arena slices, block-offset tables, capacities.  Built by tests/test_map_update_batch_host.py
// with g++ -fsanitize=address,undefined; exits 0 and prints "ok" when every check holds.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <set>
#include <utility>
#include <vector>

#include "map_update_batch_plan.h"

using namespace slamhip::mu_plan;

static int g_fail = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      ++g_fail;                                                            \
    }                                                                      \
  } while (0)

static void check_steps(const std::vector<JobKind> &jobs) {
  const std::vector<Step> steps = plan_steps(jobs);
  std::vector<int> seen(jobs.size(), 0);
  std::map<int, int> last_job_of_map;  // in step order: per map the jobs must ascend
  for (const Step &s : steps) {
    CHECK(!s.jobs.empty());
    if (s.lone) CHECK(s.jobs.size() == 1);
    std::set<int> maps;
    for (size_t i = 0; i < s.jobs.size(); ++i) {
      const int k = s.jobs[i];
      CHECK(k >= 0 && k < (int)jobs.size());
      CHECK(!jobs[k].empty);
      CHECK(jobs[k].lone == s.lone);
      CHECK(maps.insert(jobs[k].map_id).second);  // no round holds a map twice
      if (i) CHECK(s.jobs[i - 1] < k);
      ++seen[k];
    }
    for (int k : s.jobs) {
      auto it = last_job_of_map.find(jobs[k].map_id);
      if (it != last_job_of_map.end()) CHECK(it->second < k);  // job order kept per map
      last_job_of_map[jobs[k].map_id] = k;
    }
  }
  for (size_t k = 0; k < jobs.size(); ++k) CHECK(seen[k] == (jobs[k].empty ? 0 : 1));
}

static void test_rounds() {
  {  // distinct maps: one round
    std::vector<JobKind> j{{0, false, false}, {1, false, false}, {2, false, false}};
    const auto s = plan_steps(j);
    CHECK(s.size() == 1 && !s[0].lone && s[0].jobs == (std::vector<int>{0, 1, 2}));
  }
  {  // jobs 0 and 2 on one map: two rounds, {0, 1} and {2}
    std::vector<JobKind> j{{7, false, false}, {3, false, false}, {7, false, false}};
    const auto s = plan_steps(j);
    CHECK(s.size() == 2 && s[0].jobs == (std::vector<int>{0, 1}) && s[1].jobs == (std::vector<int>{2}));
  }
  {  // a lone job on a map of the open round cuts it; one on another map does not
    std::vector<JobKind> j{{0, false, false}, {1, true, false}, {2, false, false}, {0, true, false}, {3, false, false}};
    const auto s = plan_steps(j);
    CHECK(s.size() == 4);
    CHECK(s[0].lone && s[0].jobs == (std::vector<int>{1}));
    CHECK(!s[1].lone && s[1].jobs == (std::vector<int>{0, 2}));
    CHECK(s[2].lone && s[2].jobs == (std::vector<int>{3}));
    CHECK(!s[3].lone && s[3].jobs == (std::vector<int>{4}));
    check_steps(j);
  }
  {  // a shared job behind a lone one on its map, the round open: order per map kept
    std::vector<JobKind> j{{5, false, false}, {9, true, false}, {9, false, false}, {9, true, false}, {9, false, false}};
    check_steps(j);
    const auto s = plan_steps(j);
    CHECK(s.size() == 4);
  }
  {  // empty jobs take no part, all empty: no step
    std::vector<JobKind> j{{0, false, true}, {0, true, true}};
    CHECK(plan_steps(j).empty());
    CHECK(plan_steps({}).empty());
  }
  std::mt19937 rng(12345);
  for (int it = 0; it < 2000; ++it) {
    const int n = (int)(rng() % 24), n_maps = 1 + (int)(rng() % 6);
    std::vector<JobKind> j;
    for (int k = 0; k < n; ++k) j.push_back(JobKind{(int)(rng() % n_maps), rng() % 4 == 0, rng() % 7 == 0});
    check_steps(j);
  }
}

static void test_windows() {
  Window w{21, 13, 10, 6};
  CHECK(grow_window(&w, CellBox{-10, -6, 10, 6}) == 0);  // the box is the window
  CHECK(w.width == 21 && w.height == 13);
  Window g = w;
  CHECK(grow_window(&g, CellBox{-12, 0, 3, 3}) == 1);  // two cells to the left: a fifth of the side + 1 = 5
  CHECK(g.width == 26 && g.origin_x == 15 && g.height == 13 && g.origin_y == 6);
  g = w;
  CHECK(grow_window(&g, CellBox{0, 0, 40, 30}) == 1);  // what the box needs, where that is more
  CHECK(g.width == 51 && g.origin_x == 10 && g.height == 37 && g.origin_y == 6);
  g = w;
  CHECK(grow_window(&g, CellBox{-100000, -100000, 100000, 100000}) == -1);
  CHECK(g.width == 21);  // untouched
  std::mt19937 rng(7);
  for (int it = 0; it < 5000; ++it) {
    Window m{1 + (int)(rng() % 300), 1 + (int)(rng() % 300), (int)(rng() % 400) - 200, (int)(rng() % 400) - 200};
    const int lx = (int)(rng() % 600) - 300, ly = (int)(rng() % 600) - 300;
    const CellBox bb{lx, ly, lx + (int)(rng() % 200), ly + (int)(rng() % 200)};
    const KeyWindow kw = key_window(m, bb);
    CHECK(kw.n_bins == (long long)kw.w * kw.h);
    if (kw.n_bins) CHECK(kw.x0 >= 0 && kw.y0 >= 0 && kw.x0 + kw.w <= m.width && kw.y0 + kw.h <= m.height);
    Window grown = m;
    const int rc = grow_window(&grown, bb);
    CHECK(rc == 0 || rc == 1);
    // the grown window holds the whole box, and every old cell keeps its external coordinate
    CHECK(bb.lo_x + grown.origin_x >= 0 && bb.hi_x + grown.origin_x < grown.width);
    CHECK(bb.lo_y + grown.origin_y >= 0 && bb.hi_y + grown.origin_y < grown.height);
    CHECK(grown.origin_x >= m.origin_x && grown.width - grown.origin_x >= m.width - m.origin_x);
    CHECK(grown.origin_y >= m.origin_y && grown.height - grown.origin_y >= m.height - m.origin_y);
    const KeyWindow kg = key_window(grown, bb);
    CHECK(kg.w == bb.hi_x - bb.lo_x + 1 && kg.h == bb.hi_y - bb.lo_y + 1);
  }
}

static void test_arena() {
  std::mt19937 rng(99);
  for (int it = 0; it < 500; ++it) {
    const int K = (int)(rng() % 20);
    std::vector<JobShape> sh;
    for (int k = 0; k < K; ++k)
      sh.push_back(JobShape{(int)(rng() % 4097), (unsigned)(rng() % 500000), (long long)(rng() % (1 << 20))});
    if (K > 2) sh[1] = JobShape{1, 1, 1};
    const size_t line = 64, beam = 48;
    const ArenaLayout L = plan_arena(sh, line, beam);
    CHECK(L.jobs.size() == (size_t)K);
    std::vector<std::pair<size_t, size_t>> iv;  // [begin, end) of every slice
    std::vector<std::pair<size_t, size_t>> irr;
    for (int k = 0; k < K; ++k) {
      const JobSlices &s = L.jobs[k];
      const size_t n = (size_t)sh[k].n;
      auto add = [&](size_t off, size_t bytes, bool upload) {
        CHECK(off % kAlign == 0);
        CHECK(off + bytes <= (upload ? L.upload_bytes : L.arena_bytes));
        if (!upload) CHECK(off >= L.upload_bytes);
        if (bytes) iv.push_back({off, off + bytes});
      };
      add(s.scan, 4 * n * 8, true);
      add(s.occ, n * 4, true);
      add(s.host_offsets, n * 4, true);
      add(s.lines, n * line, false);
      add(s.beam_end, 2 * n * 8, false);
      add(s.beam_inv, 2 * n * 8, false);
      add(s.beam_info, n * beam, false);
      add(s.counts, n * 4, false);
      add(s.offsets, (n + 1) * 4, false);
      add(s.keys, (size_t)sh[k].total * 4, false);
      add(s.bad, ((n + 7) & ~(size_t)7) + 8, false);
      irr.push_back({s.irr, s.irr + (size_t)sh[k].n_bins + 1});
      CHECK(s.irr + (size_t)sh[k].n_bins + 1 <= L.irr_words);
    }
    CHECK(L.upload_bytes % kAlign == 0 && L.upload_bytes <= L.arena_bytes);
    for (auto *v : {&iv, &irr}) {
      std::sort(v->begin(), v->end());
      for (size_t i = 1; i < v->size(); ++i) CHECK((*v)[i - 1].second <= (*v)[i].first);  // disjoint
    }
  }
  CHECK(plan_arena({}, 64, 48).arena_bytes == 0);
}

static void test_grids() {
  const JobGrid g = job_grid(37, 203, 131, 8);
  CHECK(g.line_blocks == 37u && g.near_blocks == (17u * 17u + 3u) / 4u && g.far_blocks == 13u * 9u);
  CHECK(job_grid(1, 1, 1, 2).far_blocks == 1u);
  std::mt19937 rng(5);
  for (int it = 0; it < 500; ++it) {
    const int K = 1 + (int)(rng() % 70);
    std::vector<JobGrid> jg;
    for (int k = 0; k < K; ++k) {
      const bool none = rng() % 5 == 0;  // (a job without workgroups)
      jg.push_back(none ? JobGrid{0, 0, 0} : job_grid(1 + (int)(rng() % 4096), 1 + (int)(rng() % 2048), 1 + (int)(rng() % 2048), 2 + (int)(rng() % 39)));
    }
    const GridPlan p = plan_grid(jg);
    CHECK(p.fits);
    CHECK(p.line_off.size() == (size_t)K + 1 && p.cell_off.size() == (size_t)K + 1);
    CHECK(p.line_off[0] == 0 && p.cell_off[0] == 0);
    unsigned long long ls = 0, cs = 0;
    for (int k = 0; k < K; ++k) {
      CHECK(p.line_off[k + 1] - p.line_off[k] == jg[k].line_blocks);
      CHECK(p.cell_off[k + 1] - p.cell_off[k] == jg[k].near_blocks + jg[k].far_blocks);
      ls += jg[k].line_blocks;
      cs += jg[k].near_blocks + jg[k].far_blocks;
    }
    CHECK(p.line_off[K] == ls && p.cell_off[K] == cs);
    // every workgroup finds the job whose stretch holds it: first, last and a random one of every job
    for (int k = 0; k < K; ++k) {
      const unsigned lo = p.cell_off[k], hi = p.cell_off[k + 1];
      if (lo == hi) continue;
      CHECK(find_job(p.cell_off.data(), K, lo) == k);
      CHECK(find_job(p.cell_off.data(), K, hi - 1) == k);
      CHECK(find_job(p.cell_off.data(), K, lo + rng() % (hi - lo)) == k);
      CHECK(find_job(p.line_off.data(), K, p.line_off[k]) == k);
    }
  }
  std::vector<JobGrid> huge(3, JobGrid{1u << 30, 0, 0});
  CHECK(!plan_grid(huge).fits);
}

static void test_capacities() {
  CHECK(grow_capacity(0, 1, 1 << 16) == (size_t)1 << 16);
  CHECK(grow_capacity(0, (1 << 16) + 1, 1 << 16) == (size_t)1 << 17);
  CHECK(grow_capacity(1 << 20, 5, 1 << 16) == (size_t)1 << 20);  // never shrinks
  CHECK(grow_capacity(0, 0, 0) == 1);
  size_t cap = 0;
  for (size_t need = 1; need < ((size_t)1 << 30); need = need * 3 + 1) {
    const size_t next = grow_capacity(cap, need, 4096);
    CHECK(next >= need && next >= cap && (next & (next - 1)) == 0);
    CHECK(next == cap || next < 2 * std::max(need, (size_t)4096));
    cap = next;
  }
  CHECK(align_up(0) == 0 && align_up(1) == 256 && align_up(256) == 256 && align_up(257) == 512);
}

int main() {
  test_rounds();
  test_windows();
  test_arena();
  test_grids();
  test_capacities();
  if (g_fail) {
    std::fprintf(stderr, "%d checks failed\n", g_fail);
    return 1;
  }
  std::puts("ok");
  return 0;
}
