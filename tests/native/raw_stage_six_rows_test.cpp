// Native test of RawBatchStage (csrc/scan_filter.cpp) with the SIX-row block layout slamhip_matcher_m3rsm_match_each_raw
// asks for (five rows and the kept points' angles): requests that keep 0, 1 and 257 points.  scan_filter.cpp is compiled
// into this program; tests/test_pyr_refresh_plan_host.py runs it plainly and under -fsanitize=address,undefined, where
// the pinned arena and the arena in HBM are heap blocks of exactly arena_bytes / dst_doubles, written the way the
// assembly kernel writes them.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "scan_filter.h"

using namespace slamhip;

static int g_failed = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);  \
      ++g_failed;                                                    \
    }                                                                \
  } while (0)

struct Request {
  std::vector<double> range, angle, factor;
  std::vector<int> occ;
  int weighting;
};

// n raw beams of which exactly k are kept (is_occ), spread over the scan
static Request make_request(int n, int k, int weighting, bool with_factor) {
  Request r;
  r.weighting = weighting;
  for (int i = 0; i < n; ++i) {
    r.angle.push_back(-2.0 + 4.0 * i / n);
    r.range.push_back(0.5 + 0.001 * i);
    if (with_factor) r.factor.push_back(0.5 + 0.0005 * i);
  }
  r.occ.assign(n, 0);
  for (int q = 0; q < k; ++q) r.occ[(size_t)((long long)q * n / (k ? k : 1))] = 1;
  return r;
}

static RawBatchJob view(const Request &r) {
  RawBatchJob j{};
  j.n = (int)r.range.size();
  j.range = r.range.data();
  j.angle = r.angle.data();
  j.is_occ = r.occ.data();
  j.factor = r.factor.empty() ? nullptr : r.factor.data();
  j.trig_mode = 0;  // SLAMHIP_TRIG_RAW
  j.a_inc = 1.0;
  j.skip_rate = 0;
  j.max_range = -1.0;
  j.bounded = 0;
  j.weighting = r.weighting;
  j.pose[0] = 0.1;
  j.pose[1] = -0.2;
  j.pose[2] = 0.3;
  return j;
}

constexpr size_t kEntry = 96;  // (the caller's args entry: any size)

static void run(int rows) {
  const Request reqs[4] = {make_request(300, 0, 0, false), make_request(300, 1, 1, true), make_request(600, 257, 2, false),
                           make_request(300, 300, 0, false)};
  const int want_k[4] = {0, 1, 257, 300};
  std::vector<RawBatchJob> jobs;
  for (const Request &r : reqs) jobs.push_back(view(r));
  RawBatchStage st;
  CHECK((rows == 5 ? st.prepare(4, jobs.data(), kEntry) : st.prepare(4, jobs.data(), kEntry, rows)) == kScanOk);
  CHECK(st.n_live == 3 && st.max_k == 300);
  CHECK(st.slots.size() == 2);  // the scanners of 300 and of 600 beams
  size_t want_dst = 0;
  int live = 0, max_stride = 0;
  for (int c = 0; c < 4; ++c) {
    const RawBatchPlan &p = st.plan[c];
    CHECK(p.k == want_k[c]);
    if (p.k == 0) {
      CHECK(p.live < 0 && p.off_range == kNoRow);
      continue;
    }
    CHECK(p.live == live++);
    CHECK(p.stride % 8 == 0 && p.stride >= (size_t)p.k && p.stride < (size_t)p.k + 8);
    CHECK(p.dst_at == want_dst);  // the blocks lie side by side, `rows` rows of the stride each
    want_dst += (size_t)rows * p.stride;
    max_stride = (int)p.stride > max_stride ? (int)p.stride : max_stride;
    CHECK((p.off_kept == kNoRow) == (p.k == jobs[c].n));
    CHECK((p.off_factor == kNoRow) == (jobs[c].factor == nullptr));
    CHECK((p.off_weight == kNoRow) == (jobs[c].weighting != 2));
    for (int q = 0; q < p.k; ++q) CHECK(reqs[c].occ[st.kept[p.kept_at + q]] == 1 && (q == 0 || st.kept[p.kept_at + q] > st.kept[p.kept_at + q - 1]));
  }
  CHECK(st.dst_doubles == want_dst && st.max_stride == max_stride);
  CHECK(st.arena_bytes >= kEntry * 3);
  // the pinned arena, filled; the arena in HBM, written as the assembly kernel writes a block: every row's stride
  std::vector<unsigned char> arena(st.arena_bytes, 0xee);
  CHECK(st.fill(jobs.data(), arena.data()) == kScanOk);
  std::vector<double> dst(st.dst_doubles, 0.0);
  std::vector<unsigned char> written(st.dst_doubles, 0);
  const size_t cap = 1024;
  std::vector<double> tab(4 * cap);
  const ScanTablePlanes planes{tab.data(), tab.data() + cap, tab.data() + 2 * cap, tab.data() + 3 * cap};
  for (int c = 0; c < 4; ++c) {
    const RawBatchPlan &p = st.plan[c];
    if (p.k == 0) continue;
    // the job's entry of the args table, as RawBatchStage::entry builds it: the kernel's view of the same rows and block
    ScanAssembleEachArgs e;
    std::memset(&e, 0xee, sizeof e);
    if (rows == 6) {
      st.entry(c, arena.data(), planes, dst.data(), &e);
      CHECK(e.tab_angle == planes.angle);
    } else {
      st.entry(c, arena.data(), planes, dst.data(), &e.a);
    }
    const ScanAssembleArgs &a = e.a;
    CHECK(a.h_range == reinterpret_cast<const double *>(arena.data() + p.off_range) && (uintptr_t)a.h_range % 16 == 0);
    CHECK((a.h_kept == nullptr) == (p.k == jobs[c].n) && (uintptr_t)a.h_kept % 16 == 0);
    CHECK((a.h_factor == nullptr) == (jobs[c].factor == nullptr) && (uintptr_t)a.h_factor % 16 == 0);
    CHECK((a.h_weight != nullptr) == (jobs[c].weighting == 2) && (uintptr_t)a.h_weight % 16 == 0);
    for (const void *row : {(const void *)a.h_kept, (const void *)a.h_factor, (const void *)a.h_weight}) {
      const unsigned char *b = static_cast<const unsigned char *>(row);
      const size_t elem = row == a.h_kept ? sizeof(int) : sizeof(double);
      if (b) CHECK(b >= arena.data() + kEntry * 3 && b + elem * p.k <= arena.data() + st.arena_bytes);
    }
    for (int q = 0; q < p.k; ++q) CHECK(std::memcmp(&a.h_range[q], &reqs[c].range[st.kept[p.kept_at + q]], 8) == 0);
    CHECK(a.tab_cos == planes.cos_a && a.tab_sin == planes.sin_a && a.tab_viny == (jobs[c].weighting == 1 ? planes.viny_f : nullptr));
    CHECK(a.dst == dst.data() + p.dst_at && a.stride == p.stride && a.n == p.k && a.w_even == p.w_even);
    CHECK(p.dst_at + (size_t)rows * a.stride <= st.dst_doubles);  // (disjoint: the `written` marks below)
    CHECK(p.weighting == jobs[c].weighting);
    CHECK(p.off_range >= kEntry * 3 && p.off_range % 16 == 0 && p.off_range + sizeof(double) * p.k <= st.arena_bytes);
    const double *h_range = reinterpret_cast<const double *>(arena.data() + p.off_range);
    const int *h_kept = p.off_kept == kNoRow ? nullptr : reinterpret_cast<const int *>(arena.data() + p.off_kept);
    const ScanTables &t = st.slots[p.table].t;
    CHECK((int)t.angle.size() == jobs[c].n && (int)t.cos_a.size() == jobs[c].n);
    for (size_t q = 0; q < p.stride; ++q) {
      const bool in = q < (size_t)p.k;
      const int i = in ? (h_kept ? h_kept[q] : (int)q) : 0;
      for (int row = 0; row < rows; ++row) {
        double &cell = dst[p.dst_at + (size_t)row * p.stride + q];
        CHECK(!written[p.dst_at + (size_t)row * p.stride + q]);  // nobody else's
        written[p.dst_at + (size_t)row * p.stride + q] = 1;
        cell = !in ? 0.0 : row == 0 ? h_range[q] : row == 1 ? t.cos_a[i] : row == 2 ? t.sin_a[i] : row == 5 ? t.angle[i] : 1.0;
      }
      if (in) {
        CHECK(h_range[q] == reqs[c].range[i]);
        if (rows == 6) CHECK(dst[p.dst_at + 5 * p.stride + q] == reqs[c].angle[i]);
      }
    }
    if (jobs[c].weighting == 0) CHECK(p.w_even == 1.0 / p.k);
    CHECK(p.tot_w > 0.0);
  }
  for (unsigned char v : written) CHECK(v == 1);  // the blocks tile the arena: no double is left over
  // a second call with the same scanners builds no table
  for (RawBatchStage::Slot &s : st.slots) s.fresh = false;
  CHECK(st.prepare(4, jobs.data(), kEntry, rows) == kScanOk);
  for (const RawBatchStage::Slot &s : st.slots) CHECK(!s.fresh);
  CHECK(st.slots.size() == 2 && st.dst_doubles == want_dst);
}

int main() {
  run(6);
  run(5);  // (the default: what slamhip_matcher_process_raw_scan_batch lays out)
  if (g_failed) {
    std::printf("%d checks failed\n", g_failed);
    return 1;
  }
  std::printf("ok raw stage six rows\n");
  return 0;
}
