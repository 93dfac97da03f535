// raw_batch_stage_test.cpp -- the host half of slamhip_matcher_process_raw_scan_batch (csrc/scan_filter.cpp:
// RawBatchStage -- per job the lone call's filter and rows, the scanners' tables, the layout of the one pinned arena)
// held to the library's public host functions: slamhip_filter_scan, slamhip_scan_weights, slamhip_beam_trig_raw /
// _cached.  scan_filter.cpp is compiled INTO this program (also under ASan / UBSan: the arena is a heap block of
// exactly arena_bytes); the yardsticks come from libslamhip.so.  Everything is compared as bytes.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "scan_filter.h"
#include "slamhip.h"

using namespace slamhip;

static int g_checks = 0;
#define REQUIRE(cond, ...)                      \
  do {                                          \
    ++g_checks;                                 \
    if (!(cond)) {                              \
      std::printf("mismatch: " __VA_ARGS__);    \
      std::printf(" [%s:%d]\n", __FILE__, __LINE__); \
      std::exit(1);                             \
    }                                           \
  } while (0)

static bool same_bytes(const void *a, const void *b, size_t n) { return n == 0 || std::memcmp(a, b, n) == 0; }

struct Scanner {
  std::vector<double> angle;
  int trig_mode;
  double a_min, a_max, a_inc;
};

static Scanner make_scanner(int n, int trig_mode, double a_min, double a_inc) {
  Scanner s;
  s.trig_mode = trig_mode;
  s.a_min = a_min;
  s.a_inc = a_inc;
  s.a_max = a_min + a_inc * n + a_inc;
  double a = a_min;  // the cached provider's own accumulating angles: every table index is exact
  for (int i = 0; i < n; ++i) {
    s.angle.push_back(a);
    a += a_inc;
  }
  return s;
}

struct Job {
  const Scanner *sc;
  std::vector<double> range, factor;
  std::vector<int> occ;
  bool has_occ, has_factor;
  unsigned skip_rate;
  double max_range;
  int bounded, weighting;
  double pose[3];
  ScanWindow win;
};

static RawBatchJob view(const Job &j) {
  RawBatchJob r{};
  r.n = (int)j.range.size();
  r.range = j.range.data();
  r.angle = j.sc->angle.data();
  r.is_occ = j.has_occ ? j.occ.data() : nullptr;
  r.factor = j.has_factor ? j.factor.data() : nullptr;
  r.trig_mode = j.sc->trig_mode;
  r.a_min = j.sc->a_min;
  r.a_max = j.sc->a_max;
  r.a_inc = j.sc->a_inc;
  r.skip_rate = j.skip_rate;
  r.max_range = j.max_range;
  r.bounded = j.bounded;
  r.weighting = j.weighting;
  for (int q = 0; q < 3; ++q) r.pose[q] = j.pose[q];
  r.win = j.win;
  return r;
}

constexpr size_t kEntry = sizeof(ScanAssembleArgs);

// one job of a prepared and filled stage against the public host functions
static void check_job(const RawBatchStage &st, int c, const Job &j, const unsigned char *arena,
                      std::vector<std::pair<size_t, size_t>> &spans) {
  const RawBatchPlan &p = st.plan[c];
  const int n = (int)j.range.size();
  const Scanner &sc = *j.sc;
  // the yardstick's beam trig and, for the cached provider, its table
  std::vector<double> cos_a(n), sin_a(n), tab_s, tab_c;
  if (sc.trig_mode == SLAMHIP_TRIG_CACHED) {
    REQUIRE(slamhip_beam_trig_cached(n, sc.angle.data(), sc.a_min, sc.a_max, sc.a_inc, cos_a.data(), sin_a.data()) == 0, "trig");
    for (double a = sc.a_min; a < sc.a_max; a += sc.a_inc) {
      double s_, c_;
      ::sincos(a, &s_, &c_);
      tab_s.push_back(s_);
      tab_c.push_back(c_);
    }
  } else {
    REQUIRE(slamhip_beam_trig_raw(n, sc.angle.data(), cos_a.data(), sin_a.data()) == 0, "trig");
  }
  const ScanTables &t = st.slots[p.table].t;
  REQUIRE((int)t.cos_a.size() == n && same_bytes(t.cos_a.data(), cos_a.data(), 8 * n), "job %d: cos table", c);
  REQUIRE(same_bytes(t.sin_a.data(), sin_a.data(), 8 * n), "job %d: sin table", c);
  std::vector<int> kept(n);
  int k = -1;
  REQUIRE(slamhip_filter_scan(n, j.range.data(), sc.angle.data(), j.has_occ ? j.occ.data() : nullptr, sc.trig_mode, sc.a_min,
                              sc.a_inc, (int)tab_s.size(), tab_s.data(), tab_c.data(), j.pose, j.skip_rate, j.max_range,
                              j.bounded, j.win.width, j.win.height, j.win.origin_x, j.win.origin_y, j.win.scale, kept.data(),
                              &k) == 0, "filter");
  REQUIRE(p.k == k, "job %d: kept %d, the filter keeps %d", c, p.k, k);
  REQUIRE(same_bytes(st.kept.data() + p.kept_at, kept.data(), 4 * (size_t)k), "job %d: kept list", c);
  if (k == 0) {
    REQUIRE(p.live < 0 && p.off_range == kNoRow && p.off_kept == kNoRow && p.off_factor == kNoRow && p.off_weight == kNoRow,
            "job %d keeps nothing but has rows", c);
    return;
  }
  REQUIRE(p.live >= 0 && p.live < st.n_live, "job %d: live place", c);
  std::vector<double> r(k), a(k), f(k), w(k);
  for (int q = 0; q < k; ++q) {
    r[q] = j.range[kept[q]];
    a[q] = sc.angle[kept[q]];
    if (j.has_factor) f[q] = j.factor[kept[q]];
  }
  auto span = [&](size_t off, size_t bytes, const char *what) {
    REQUIRE(off != kNoRow && off % 16 == 0 && off + bytes <= st.arena_bytes, "job %d: %s row at %zu (+%zu) of %zu", c, what, off,
            bytes, st.arena_bytes);
    spans.push_back({off, off + bytes});
  };
  span(p.off_range, 8 * (size_t)k, "range");
  REQUIRE(same_bytes(arena + p.off_range, r.data(), 8 * (size_t)k), "job %d: ranges", c);
  if (k < n) {
    span(p.off_kept, 4 * (size_t)k, "kept");
    REQUIRE(same_bytes(arena + p.off_kept, kept.data(), 4 * (size_t)k), "job %d: kept row", c);
  } else {
    REQUIRE(p.off_kept == kNoRow, "job %d keeps every beam but stages indices", c);
  }
  if (j.has_factor) {
    span(p.off_factor, 8 * (size_t)k, "factor");
    REQUIRE(same_bytes(arena + p.off_factor, f.data(), 8 * (size_t)k), "job %d: factors", c);
  } else {
    REQUIRE(p.off_factor == kNoRow, "job %d has no factors but stages some", c);
  }
  REQUIRE(slamhip_scan_weights(j.weighting, k, r.data(), a.data(), w.data()) == 0, "weights");
  double tot = 0;
  for (int q = 0; q < k; ++q) tot += w[q];
  REQUIRE(same_bytes(&p.tot_w, &tot, 8), "job %d (weighting %d): total weight %.17g, in index order %.17g", c, j.weighting, p.tot_w, tot);
  if (j.weighting == 0) {
    REQUIRE(same_bytes(&p.w_even, &w[0], 8), "job %d: even weight", c);
  } else if (j.weighting == 1) {
    // (the device makes tab_viny[i] * sqrt(range): the same product on the host must be the yardstick's weight)
    for (int q = 0; q < k; ++q) {
      const double v = t.viny_f[kept[q]] * std::sqrt(r[q]);
      REQUIRE(same_bytes(&v, &w[q], 8), "job %d: viny weight %d", c, q);
    }
  }
  if (j.weighting == 2) {
    span(p.off_weight, 8 * (size_t)k, "weight");
    REQUIRE(same_bytes(arena + p.off_weight, w.data(), 8 * (size_t)k), "job %d: ahr weights", c);
  } else {
    REQUIRE(p.off_weight == kNoRow, "job %d: weights staged that the device makes", c);
  }
  REQUIRE(p.stride >= (size_t)k && p.stride % 8 == 0 && p.stride < (size_t)k + 8, "job %d: stride", c);
}

static const ScanAssembleArgs &five_rows_of(const ScanAssembleArgs &e) { return e; }
static const ScanAssembleArgs &five_rows_of(const ScanAssembleEachArgs &e) { return e.a; }
static const double *angle_plane_of(const ScanAssembleArgs &) { return nullptr; }
static const double *angle_plane_of(const ScanAssembleEachArgs &e) { return e.tab_angle; }

// live job c's entry of the args table, as RawBatchStage::entry builds it over the filled arena, a scanner's table of
// four planes of `cap` doubles at `tab` and the arena in HBM at `dst_base`
template <class Entry>
static void check_entry(const RawBatchStage &st, int c, const Job &j, const unsigned char *arena, const double *tab, size_t cap,
                        double *dst_base, int rows, std::vector<std::pair<size_t, size_t>> &blocks) {
  const RawBatchPlan &p = st.plan[c];
  const size_t k = (size_t)p.k, n = j.range.size();
  Entry e;
  std::memset(&e, 0xa5, sizeof e);
  st.entry(c, arena, ScanTablePlanes{tab, tab + cap, tab + 2 * cap, tab + 3 * cap}, dst_base, &e);
  const ScanAssembleArgs &a = five_rows_of(e);
  const size_t table_end = sizeof(Entry) * (size_t)st.n_live;
  auto pinned = [&](const void *ptr, size_t elem, const char *what) {
    const unsigned char *b = static_cast<const unsigned char *>(ptr);
    REQUIRE((uintptr_t)b % 16 == 0, "job %d: %s row is not 16-byte aligned", c, what);
    REQUIRE(b >= arena + table_end && b + elem * k <= arena + st.arena_bytes, "job %d: %s row leaves the arena", c, what);
  };
  REQUIRE(a.h_range != nullptr, "job %d: no range row", c);
  pinned(a.h_range, 8, "range");
  for (size_t q = 0; q < k; ++q)
    REQUIRE(same_bytes(&a.h_range[q], &j.range[st.kept[p.kept_at + q]], 8), "job %d: h_range[%zu]", c, q);
  REQUIRE((a.h_kept == nullptr) == (k == n), "job %d: kept row of %zu of %zu beams", c, k, n);
  if (a.h_kept) pinned(a.h_kept, 4, "kept");
  REQUIRE((a.h_factor == nullptr) == !j.has_factor, "job %d: factor row", c);
  if (a.h_factor) pinned(a.h_factor, 8, "factor");
  REQUIRE((a.h_weight != nullptr) == (j.weighting == 2), "job %d: weight row under weighting %d", c, j.weighting);
  if (a.h_weight) pinned(a.h_weight, 8, "weight");
  REQUIRE(a.tab_viny == (j.weighting == 1 ? tab + 2 * cap : nullptr), "job %d: viny plane under weighting %d", c, j.weighting);
  REQUIRE(a.tab_cos == tab && a.tab_sin == tab + cap, "job %d: cos / sin planes", c);
  REQUIRE(angle_plane_of(e) == (rows == 6 ? tab + 3 * cap : nullptr), "job %d: angle plane", c);
  REQUIRE(a.n == p.k && a.stride == p.stride && same_bytes(&a.w_even, &p.w_even, 8), "job %d: n, stride, w_even", c);
  REQUIRE(a.dst >= dst_base && (size_t)(a.dst - dst_base) + (size_t)rows * a.stride <= st.dst_doubles, "job %d: block leaves the arena in HBM", c);
  blocks.push_back({(size_t)(a.dst - dst_base), (size_t)(a.dst - dst_base) + (size_t)rows * a.stride});
}

template <class Entry>
static void check_stage_rows(RawBatchStage &st, const std::vector<Job> &jobs) {
  constexpr int rows = sizeof(Entry) == sizeof(ScanAssembleEachArgs) ? 6 : 5;
  std::vector<RawBatchJob> in;
  for (const Job &j : jobs) in.push_back(view(j));
  REQUIRE(st.prepare((int)in.size(), in.data(), sizeof(Entry), rows) == kScanOk, "prepare");
  // exactly arena_bytes on the heap: the sanitizer sees a byte too many
  unsigned char *arena = static_cast<unsigned char *>(std::malloc(st.arena_bytes ? st.arena_bytes : 1));
  std::memset(arena, 0xa5, st.arena_bytes);
  REQUIRE(st.fill(in.data(), arena) == kScanOk, "fill");
  std::vector<std::pair<size_t, size_t>> spans, blocks;
  spans.push_back({0, sizeof(Entry) * (size_t)st.n_live});  // the args table
  const size_t cap = 512;
  std::vector<double> tab(4 * cap), hbm(st.dst_doubles ? st.dst_doubles : 1);
  size_t dst = 0;
  int live = 0;
  for (int c = 0; c < (int)jobs.size(); ++c) {
    check_job(st, c, jobs[c], arena, spans);
    REQUIRE(st.plan[c].weighting == jobs[c].weighting, "job %d: the plan's weighting", c);
    if (st.plan[c].k > 0) {
      REQUIRE(st.plan[c].live == live++, "live places in job order");
      REQUIRE(st.plan[c].dst_at == dst, "job %d: block at %zu, the blocks before end at %zu", c, st.plan[c].dst_at, dst);
      dst += (size_t)rows * st.plan[c].stride;
      check_entry<Entry>(st, c, jobs[c], arena, tab.data(), cap, hbm.data(), rows, blocks);
    }
  }
  REQUIRE(dst == st.dst_doubles && live == st.n_live, "arena in HBM: %zu doubles, the blocks need %zu", st.dst_doubles, dst);
  for (const auto *v : {&spans, &blocks})
    for (size_t x = 0; x < v->size(); ++x)
      for (size_t y = x + 1; y < v->size(); ++y)
        REQUIRE((*v)[x].second <= (*v)[y].first || (*v)[y].second <= (*v)[x].first, "rows / blocks %zu and %zu overlap", x, y);
  std::free(arena);
}

// (six rows first: the stage is left as a five-row call leaves it, which is what the callers look at)
static void check_stage(RawBatchStage &st, const std::vector<Job> &jobs) {
  check_stage_rows<ScanAssembleEachArgs>(st, jobs);
  check_stage_rows<ScanAssembleArgs>(st, jobs);
}

int main() {
  std::mt19937 rs(17);
  std::uniform_real_distribution<double> u(0.0, 1.0);
  const double inc = 270.0 / 180.0 * M_PI / 360;
  std::vector<Scanner> scanners;
  scanners.push_back(make_scanner(360, SLAMHIP_TRIG_RAW, -2.3, inc));
  scanners.push_back(make_scanner(360, SLAMHIP_TRIG_CACHED, -2.3, inc));
  scanners.push_back(make_scanner(257, SLAMHIP_TRIG_CACHED, -1.0, 0.01));
  scanners.push_back(make_scanner(1, SLAMHIP_TRIG_RAW, 0.3, 0.01));
  scanners.push_back(make_scanner(64, SLAMHIP_TRIG_RAW, -3.0, 0.09));
  auto random_job = [&](const Scanner *sc) {
    Job j{};
    j.sc = sc;
    const int n = (int)sc->angle.size();
    for (int i = 0; i < n; ++i) {
      j.range.push_back(0.2 + 9.0 * u(rs));
      j.factor.push_back(0.5 + u(rs));
      j.occ.push_back(u(rs) < 0.8 ? 1 : 0);
    }
    j.has_occ = u(rs) < 0.5;
    j.has_factor = u(rs) < 0.5;
    j.skip_rate = (unsigned)(u(rs) * 4);
    j.max_range = u(rs) < 0.5 ? -1.0 : 6.0;
    j.bounded = u(rs) < 0.6;
    j.weighting = (int)(u(rs) * 3) % 3;
    j.pose[0] = 4.0 * (u(rs) - 0.5);
    j.pose[1] = 4.0 * (u(rs) - 0.5);
    j.pose[2] = 6.0 * (u(rs) - 0.5);
    // a window of 100 x 80 cells of 0.1 m whose rim the longer beams cross
    j.win = ScanWindow{0.1, 50 + (int)(20 * (u(rs) - 0.5)), 40, 100, 80};
    return j;
  };
  int n_jobs = 0;
  {
    // ---- random batches through ONE stage (the scanners' tables stay between the calls)
    RawBatchStage st;
    for (int round = 0; round < 60; ++round) {
      std::vector<Job> jobs;
      const int K = 1 + (int)(u(rs) * 9);
      for (int c = 0; c < K; ++c) jobs.push_back(random_job(&scanners[(size_t)(u(rs) * scanners.size()) % scanners.size()]));
      check_stage(st, jobs);
      n_jobs += K;
    }
    REQUIRE(st.slots.size() == scanners.size(), "%zu tables for %zu scanners", st.slots.size(), scanners.size());
  }
  {
    // ---- the named cases
    RawBatchStage st;
    Job rim = random_job(&scanners[0]);  // a bounded map whose rim drops points, and nothing else does
    rim.has_occ = false;
    rim.skip_rate = 0;
    rim.max_range = -1.0;
    rim.bounded = 1;
    rim.pose[0] = 4.4;
    rim.pose[1] = 0.0;
    rim.win.origin_x = 50;  // (x up to 5.0 m: the beams towards +x end at 5.9)
    for (double &r : rim.range) r = 1.5;
    Job none = random_job(&scanners[0]);  // keeps nothing
    none.has_occ = true;
    for (int &o : none.occ) o = 0;
    Job all = random_job(&scanners[1]);  // keeps everything: no index row
    all.has_occ = false;
    all.skip_rate = 0;
    all.max_range = -1.0;
    all.bounded = 0;
    all.weighting = 2;
    Job one = random_job(&scanners[0]);  // one kept beam
    one.has_occ = true;
    one.skip_rate = 0;
    one.max_range = -1.0;
    one.bounded = 0;
    for (int &o : one.occ) o = 0;
    one.occ[123] = 1;
    check_stage(st, {rim, none, all, one});
    n_jobs += 4;
    REQUIRE(st.plan[0].k > 0 && st.plan[0].k < 360, "the rim drops %d of 360 points", 360 - st.plan[0].k);
    REQUIRE(st.plan[1].k == 0 && st.plan[2].k == 360 && st.plan[3].k == 1 && st.n_live == 3, "named cases: kept counts");
    // scanners: jobs 0, 1 and 3 share one table, job 2 (the cached provider) has its own; both were built by this call
    REQUIRE(st.slots.size() == 2 && st.plan[0].table == st.plan[1].table && st.plan[0].table == st.plan[3].table &&
                st.plan[2].table != st.plan[0].table, "scanner tables of the named cases");
    REQUIRE(st.slots[0].fresh && st.slots[1].fresh, "new tables are to be uploaded");
    for (auto &s : st.slots) s.fresh = false;  // (the caller, once it has uploaded them)
    check_stage(st, {one, all, rim});          // the same scanners, new ranges: nothing to upload
    n_jobs += 3;
    REQUIRE(st.slots.size() == 2 && !st.slots[0].fresh && !st.slots[1].fresh, "a later call with the same scanners builds no table");
    // a changed angle: a third table, the others stay
    Scanner moved = scanners[0];
    moved.angle[200] = std::nextafter(moved.angle[200], 10.0);
    Job m = rim;
    m.sc = &moved;
    check_stage(st, {rim, m});
    n_jobs += 2;
    REQUIRE(st.slots.size() == 3 && st.slots[2].fresh && !st.slots[0].fresh && st.plan[0].table != st.plan[1].table,
            "a changed angle is another scanner");
    // ... and a changed table setting with the same angles
    Scanner wider = scanners[1];
    wider.a_max += wider.a_inc;
    Job w2 = all;
    w2.sc = &wider;
    check_stage(st, {all, w2});
    n_jobs += 2;
    REQUIRE(st.slots.size() == 4 && st.plan[0].table != st.plan[1].table, "a changed a_max is another scanner");
  }
  {
    // ---- more scanners over time than are kept: the oldest go, the count stays bounded, results stay right
    RawBatchStage st;
    std::vector<Scanner> many;
    for (int q = 0; q < 80; ++q) many.push_back(make_scanner(40 + q, SLAMHIP_TRIG_RAW, -1.0 - 0.001 * q, 0.02));
    for (int q = 0; q < 80; ++q) {
      check_stage(st, {random_job(&many[q]), random_job(&many[q / 2])});
      n_jobs += 2;
    }
    REQUIRE((int)st.slots.size() <= RawBatchStage::kSlotsKept, "%zu tables kept", st.slots.size());
    // ... and a call that needs more than are kept at once gets them
    std::vector<Job> wide;
    for (int q = 0; q < 70; ++q) wide.push_back(random_job(&many[q]));
    check_stage(st, wide);
    n_jobs += 70;
  }
  {
    // ---- a job from the C-ABI's raw scan, a pose and a window: every field lands in its place
    Job j = random_job(&scanners[1]);
    j.has_occ = j.has_factor = true;
    j.skip_rate = 3;
    j.bounded = 7;  // (any non-zero value means bounded)
    const RawBatchJob want = view(j);
    const slamhip_raw_scan raw{want.n,     want.range, want.angle,     want.is_occ,    want.factor, want.trig_mode, want.a_min,
                               want.a_max, want.a_inc, want.skip_rate, want.max_range, j.bounded,   want.weighting};
    const RawBatchJob got = RawBatchStage::job_of(raw, j.pose, j.win);
    REQUIRE(got.n == want.n && got.range == want.range && got.angle == want.angle && got.is_occ == want.is_occ &&
                got.factor == want.factor && got.trig_mode == want.trig_mode && got.skip_rate == 3u && got.bounded == 1 &&
                got.weighting == want.weighting, "job_of: the scan's fields");
    REQUIRE(same_bytes(&got.a_min, &want.a_min, 8) && same_bytes(&got.a_max, &want.a_max, 8) && same_bytes(&got.a_inc, &want.a_inc, 8) &&
                same_bytes(&got.max_range, &want.max_range, 8) && same_bytes(got.pose, want.pose, 24), "job_of: the doubles");
    REQUIRE(got.win.scale == j.win.scale && got.win.origin_x == j.win.origin_x && got.win.origin_y == j.win.origin_y &&
                got.win.width == j.win.width && got.win.height == j.win.height, "job_of: the window");
  }
  {
    // ---- errors: found in pass 1, with the lone call's texts
    RawBatchStage st;
    Job ok = random_job(&scanners[0]);
    RawBatchJob bad = view(ok);
    bad.n = 0;
    RawBatchJob in[2] = {view(ok), bad};
    REQUIRE(st.prepare(2, in, kEntry) == kScanBadArgs, "n = 0");
    in[1] = view(ok);
    in[1].range = nullptr;
    REQUIRE(st.prepare(2, in, kEntry) == kScanBadArgs, "null ranges");
    in[1] = view(ok);
    in[1].angle = nullptr;
    REQUIRE(st.prepare(2, in, kEntry) == kScanBadArgs, "null angles");
    in[1] = view(ok);
    in[1].weighting = 3;
    REQUIRE(st.prepare(2, in, kEntry) == kScanBadWeighting, "weighting 3");
    Scanner outside = scanners[1];
    outside.a_max = outside.a_min + outside.a_inc * 100;  // a table shorter than the scan
    Job o = random_job(&outside);
    in[1] = view(o);
    REQUIRE(st.prepare(2, in, kEntry) == kScanAngleOutsideTable, "angle outside the table");
    in[1] = view(o);
    in[1].a_inc = 0.0;
    REQUIRE(st.prepare(2, in, kEntry) == kScanBadArgs, "a_inc = 0");
    // ... and the stage is usable afterwards
    check_stage(st, {ok, ok});
    n_jobs += 2;
    REQUIRE(st.plan[0].table == st.plan[1].table, "two jobs of one scanner share its table");
  }
  std::printf("ok %d jobs, %d checks\n", n_jobs, g_checks);
  return 0;
}
