// scan_filter.cpp -- the raw scan's filter in two passes (plain C++, no device code).
//
// filter_scan keeps point i iff (skip_rate == 0 or i % skip_rate == 0), the point is occupied, it is not beyond the
// usable range and -- on a bounded map -- its end point's cell is in the map (weighted_mean_point_probability_spe.h:
// 75-95,136-141).  As ONE loop that is a chain of early exits around two true divisions and two floors per point, with
// a push_back at its end: nothing a compiler vectorizes, 10 us at 1080 beams.  Here
//   pass 1 writes one byte per point, branch-free, from the same operations on the same operands in the same order
//          (-ffp-contract=off; the division stays a division) -- the bounds test on the floored doubles against
//          -origin and extent - origin, which is the integer test's decision for every finite value (NaN and +-inf
//          come out "dropped" either way);
//   pass 2 turns the bytes into the ascending index list and gathers the rows that go with it.
// Pass 1 is compiled twice, baseline x86-64 (floor is a libm call there: no faster than the loop it replaces) and AVX2
// (vdivpd / vroundpd, four points at a time), picked at run time as mt_block.cpp picks its clones.
// tests/native/scan_filter_test.cpp holds both to the one-loop form.
#include <cmath>
#include <cstring>
#include <limits>

#include "scan_filter.h"

namespace slamhip {
namespace {

template <bool OCC, bool CUT, bool GEOM, bool RAW>
static inline __attribute__((always_inline)) void mask_loop(const ScanFilterArgs &a, const double *__restrict tc,
                                                            const double *__restrict ts, double cb, double sb,
                                                            unsigned char *__restrict mask) {
  constexpr double eps = std::numeric_limits<double>::epsilon();
  const int n = a.n;
  const double *__restrict range = a.range;
  const int *__restrict occ = a.is_occ;
  const double *__restrict cos_a = RAW ? tc : a.cos_a, *__restrict sin_a = RAW ? ts : a.sin_a;
  const double max_range = a.max_range, px = a.pose[0], py = a.pose[1], scale = a.scale;
  // 0 <= (int)floor(v) + origin < extent, on the floored double
  const double x_lo = -(double)a.origin_x, x_hi = (double)a.width - (double)a.origin_x;
  const double y_lo = -(double)a.origin_y, y_hi = (double)a.height - (double)a.origin_y;
#ifdef SCAN_FILTER_TEST_MUTANT  // (tests/test_scan_filter_host.py: the test must tell this from a division)
  const double inv_scale = 1.0 / scale;
#endif
  for (int i = 0; i < n; ++i) {
    const double r = range[i];
    bool keep = true;
    if (OCC) keep &= occ[i] != 0;
    if (CUT) keep &= !(max_range < r + eps);
    if (GEOM) {
      double c, s;
      if (RAW) {
        c = cos_a[i];
        s = sin_a[i];
      } else {
        c = cb * cos_a[i] - sb * sin_a[i];
        s = sb * cos_a[i] + cb * sin_a[i];
      }
      const double wx = px + r * c, wy = py + r * s;
#ifdef SCAN_FILTER_TEST_MUTANT
      const double fx = std::floor(wx * inv_scale), fy = std::floor(wy * inv_scale);
#else
      const double fx = std::floor(wx / scale), fy = std::floor(wy / scale);
#endif
      keep &= (x_lo <= fx) & (fx < x_hi) & (y_lo <= fy) & (fy < y_hi);
    }
    mask[i] = keep ? 1 : 0;
  }
}

template <bool OCC, bool CUT>
static inline __attribute__((always_inline)) void mask_geom(const ScanFilterArgs &a, const double *tc, const double *ts,
                                                            double cb, double sb, unsigned char *mask) {
  if (!a.bounded) mask_loop<OCC, CUT, false, false>(a, tc, ts, cb, sb, mask);
  else if (a.trig_raw) mask_loop<OCC, CUT, true, true>(a, tc, ts, cb, sb, mask);
  else mask_loop<OCC, CUT, true, false>(a, tc, ts, cb, sb, mask);
}

static inline __attribute__((always_inline)) int mask_body(const ScanFilterArgs &a, const double *tc, const double *ts,
                                                           double cb, double sb, unsigned char *__restrict mask) {
  constexpr double eps = std::numeric_limits<double>::epsilon();
  const bool cut = 0.0 < a.max_range + eps;  // (a usable range is set at all)
  if (a.is_occ) {
    if (cut) mask_geom<true, true>(a, tc, ts, cb, sb, mask);
    else mask_geom<true, false>(a, tc, ts, cb, sb, mask);
  } else {
    if (cut) mask_geom<false, true>(a, tc, ts, cb, sb, mask);
    else mask_geom<false, false>(a, tc, ts, cb, sb, mask);
  }
  if (a.skip_rate > 1) {  // (no vector has a remainder: the rare setting gets a pass of its own)
    unsigned left = 0;    // = i % skip_rate
    for (int i = 0; i < a.n; ++i) {
      mask[i] &= left == 0 ? 1 : 0;
      left = left + 1 == a.skip_rate ? 0 : left + 1;
    }
  }
  int k = 0;
  for (int i = 0; i < a.n; ++i) k += mask[i];
  return k;
}

int mask_generic(const ScanFilterArgs &a, const double *tc, const double *ts, double cb, double sb, unsigned char *mask) {
  return mask_body(a, tc, ts, cb, sb, mask);
}
__attribute__((target("avx2"))) int mask_avx2(const ScanFilterArgs &a, const double *tc, const double *ts, double cb,
                                              double sb, unsigned char *mask) {
  return mask_body(a, tc, ts, cb, sb, mask);
}

static inline __attribute__((always_inline)) double fill_body(int k, const int *__restrict kept,
                                                              const double *__restrict range,
                                                              const double *__restrict factor,
                                                              const double *__restrict viny_f, double *__restrict r_out,
                                                              double *__restrict f_out, double *__restrict w_out) {
  double tot_w = 0;
  if (w_out) {
    // (the sum's k dependent additions run beside the gathers and the square roots instead of behind them)
    for (int q = 0; q < k; ++q) {
      const int i = kept[q];
      const double r = range[i];
      if (r_out) r_out[q] = r;
      if (f_out) f_out[q] = factor[i];
      const double w = viny_f[i] * std::sqrt(r);
      w_out[q] = w;
      tot_w += w;
    }
  } else if (f_out) {
    for (int q = 0; q < k; ++q) {
      const int i = kept[q];
      if (r_out) r_out[q] = range[i];
      f_out[q] = factor[i];
    }
  } else if (r_out) {
    for (int q = 0; q < k; ++q) r_out[q] = range[kept[q]];
  }
  return tot_w;
}

double fill_generic(int k, const int *kept, const double *range, const double *factor, const double *viny_f, double *r_out,
                    double *f_out, double *w_out) {
  return fill_body(k, kept, range, factor, viny_f, r_out, f_out, w_out);
}
__attribute__((target("avx2"))) double fill_avx2(int k, const int *kept, const double *range, const double *factor,
                                                 const double *viny_f, double *r_out, double *f_out, double *w_out) {
  return fill_body(k, kept, range, factor, viny_f, r_out, f_out, w_out);
}

bool use_avx2(int variant) { return variant < 0 ? scan_filter_has_avx2() : variant == 1; }

}  // namespace

bool scan_filter_has_avx2() {
  static const bool avx2 = __builtin_cpu_supports("avx2");
  return avx2;
}

int scan_filter_mask(const ScanFilterArgs &a, unsigned char *mask, double *tmp, int variant) {
  double sb = 0, cb = 1;
  const double *tc = nullptr, *ts = nullptr;
  if (a.bounded) {
    if (a.trig_raw) {
      // the per-beam sincos of the sum, as the one-loop form makes it (for every point: the loop made it for the
      // points its earlier tests let through -- the same value where it is used)
      double *c_ = tmp, *s_ = tmp + a.n;
      for (int i = 0; i < a.n; ++i) ::sincos(a.pose[2] + a.angle[i], &s_[i], &c_[i]);
      tc = c_;
      ts = s_;
    } else {
      ::sincos(a.pose[2], &sb, &cb);
    }
  }
  return use_avx2(variant) ? mask_avx2(a, tc, ts, cb, sb, mask) : mask_generic(a, tc, ts, cb, sb, mask);
}

int scan_filter_compact(const unsigned char *mask, int n, int *kept) {
  int k = 0, i = 0;
  // eight bytes at a time: a scan keeps and drops its points in long runs (k <= i: every store stays inside the n entries)
  for (; i + 8 <= n; i += 8) {
    unsigned long long m8;
    std::memcpy(&m8, mask + i, 8);
    if (m8 == 0x0101010101010101ull) {
      for (int q = 0; q < 8; ++q) kept[k + q] = i + q;
      k += 8;
    } else if (m8 != 0) {
      for (int q = 0; q < 8; ++q) {
        kept[k] = i + q;
        k += mask[i + q];
      }
    }
  }
  for (; i < n; ++i) {
    kept[k] = i;
    k += mask[i];
  }
  return k;
}

double scan_filter_fill(int k, const int *kept, const double *range, const double *factor, const double *viny_f,
                        double *r_out, double *f_out, double *w_out, int variant) {
  return use_avx2(variant) ? fill_avx2(k, kept, range, factor, viny_f, r_out, f_out, w_out)
                           : fill_generic(k, kept, range, factor, viny_f, r_out, f_out, w_out);
}

const char *scan_error_text(int code) {
  switch (code) {
    case kScanOk: return "ok";
    case kScanAngleOutsideTable: return "scan angle outside the trig table";
    case kScanAhrBin: return "angle histogram bin out of range (reference asserts here)";
    case kScanBadWeighting: return "unknown weighting kind";
    default: return "bad arguments";
  }
}

int beam_trig_raw(int n, const double *angle, double *cos_out, double *sin_out) {
  if (n < 0 || !angle || !cos_out || !sin_out) return kScanBadArgs;
  for (int i = 0; i < n; ++i) ::sincos(angle[i], &sin_out[i], &cos_out[i]);
  return kScanOk;
}

int beam_trig_cached(int n, const double *angle, double a_min, double a_max, double a_inc, double *cos_out, double *sin_out) {
  if (n < 0 || !angle || !cos_out || !sin_out || !(a_inc > 0)) return kScanBadArgs;
  // the table of the last (a_min, a_max, a_inc) is kept: a world loop asks for the same one twice per scan, and
  // building it is a libm sincos per entry
  struct Table {
    double a_min = 0, a_max = 0, a_inc = 0;
    std::vector<double> ts, tc;
  };
  static thread_local Table tab;
  if (tab.ts.empty() || tab.a_min != a_min || tab.a_max != a_max || tab.a_inc != a_inc) {
    tab.ts.clear();
    tab.tc.clear();
    for (double a = a_min; a < a_max; a += a_inc) {  // accumulating loop, as the provider builds it
      double sv, cv;
      ::sincos(a, &sv, &cv);  // fused pair, as in the reference build (see score_staged)
      tab.ts.push_back(sv);
      tab.tc.push_back(cv);
    }
    tab.a_min = a_min;
    tab.a_max = a_max;
    tab.a_inc = a_inc;
  }
  const std::vector<double> &ts = tab.ts, &tc = tab.tc;
  for (int i = 0; i < n; ++i) {
    const int idx = (int)std::round((angle[i] - a_min) / a_inc);
    if (idx < 0 || idx >= (int)ts.size()) return kScanAngleOutsideTable;
    cos_out[i] = tc[idx];
    sin_out[i] = ts[idx];
  }
  return kScanOk;
}

// VinySlamSPW's angular factor (weighted_mean_point_probability_spe.h:47-60): the weight is this times sqrt(range)
static inline double viny_factor(double angle) {
  double sv, cv;
  ::sincos(angle, &sv, &cv);
  const double ac = std::abs(cv);
  double w = std::abs(sv) + ac;
  if (0.9 < ac) w = 3;
  else if (0.8 < ac) w = 2;
  return w;
}

int scan_weights(int kind, int n, const double *range, const double *angle, double *out) {
  if (n < 0 || !range || !angle || !out) return kScanBadArgs;
  if (kind == 0) {
    const double w = 1.0 / n;
    for (int i = 0; i < n; ++i) out[i] = w;
    return kScanOk;
  }
  if (kind == 1) {
    for (int i = 0; i < n; ++i) out[i] = viny_factor(angle[i]) * std::sqrt(range[i]);
    return kScanOk;
  }
  if (kind == 2) {
    constexpr int NB = 20;
    unsigned hist[NB] = {0};
    std::vector<double> dirs(n > 0 ? n : 1, 0.0);
    const double step = (180 * M_PI / 180) / NB;
    for (int i = 1; i < n; ++i) {
      double s1, c1, s0, c0;
      ::sincos(angle[i], &s1, &c1);
      ::sincos(angle[i - 1], &s0, &c0);
      const double d_x = range[i] * c1 - range[i - 1] * c0;
      const double d_y = range[i] * s1 - range[i - 1] * s0;
      double a = 0;
      if (d_y != 0) {
        a = std::acos(d_x / std::sqrt(d_x * d_x + d_y * d_y));
        if (d_y < 0 && d_x != 0) a = M_PI - a;
      }
      const size_t bin = (size_t)std::floor(a / step);
      if (bin >= NB) return kScanAhrBin;
      hist[bin]++;
      dirs[i] = a;
    }
    for (int i = 0; i < n; ++i) {
      const unsigned v = i == 0 ? (unsigned)n : hist[(size_t)std::floor(dirs[i] / step)];
      out[i] = 1.0 / v;
    }
    return kScanOk;
  }
  return kScanBadWeighting;
}

// total_weight accumulates in beam order and does not depend on the pose
// (weighted_mean_point_probability_spe.h:125)
double scan_total_weight(const double *weight, int n) {
  double tot_w = 0;
  for (int i = 0; i < n; ++i) tot_w += weight[i];
  return tot_w;
}

// ... of EvenSPW's k weights 1.0 / k: the same k additions in the same order, made once per k -- the value depends on
// nothing else, and the chain of k dependent additions was the longest single item of the raw scan's host half (about
// 1.3 us at 1080 beams by the additions' latency).  Per thread, as beam_trig_cached keeps its table.
double scan_total_weight_even(int k, double w) {
  static thread_local std::vector<double> memo;  // [k] = the sum, 0.0 = not made yet (a sum of positive weights is not 0)
  if ((int)memo.size() <= k) memo.resize((size_t)k + 1, 0.0);
  if (memo[k] == 0.0) {
    double tot_w = 0;
    for (int i = 0; i < k; ++i) tot_w += w;
    memo[k] = tot_w;
  }
  return memo[k];
}

bool ScanTables::same(int n, const double *angle_, int trig_mode_, double a_min_, double a_max_, double a_inc_) const {
  return (int)angle.size() == n && trig_mode == trig_mode_ && a_min == a_min_ && a_max == a_max_ && a_inc == a_inc_ &&
         std::memcmp(angle.data(), angle_, sizeof(double) * n) == 0;
}

int scan_tables_build(ScanTables &t, int n, const double *angle, int trig_mode, double a_min, double a_max, double a_inc) {
  t.angle.assign(angle, angle + n);
  t.trig_mode = trig_mode;
  t.a_min = a_min;
  t.a_max = a_max;
  t.a_inc = a_inc;
  t.cos_a.resize(n);
  t.sin_a.resize(n);
  // (trig_mode 1 is SLAMHIP_TRIG_CACHED; everything else the raw provider, as the lone call has always read it)
  const int rc = trig_mode == 1 ? beam_trig_cached(n, angle, a_min, a_max, a_inc, t.cos_a.data(), t.sin_a.data())
                                : beam_trig_raw(n, angle, t.cos_a.data(), t.sin_a.data());
  if (rc) {
    t.angle.clear();
    return rc;
  }
  t.viny_f.resize(n);
  for (int i = 0; i < n; ++i) t.viny_f[i] = viny_factor(angle[i]);
  return kScanOk;
}

// ---- filter_scan: keeps point i iff (skip_rate == 0 or i % skip_rate == 0), occupied, its end point's cell in the
// map, and not beyond the usable range (Q8 - Q10)
int scan_filter_kept(const ScanTables &t, int n, const double *range, const double *angle, const int *is_occ,
                     unsigned skip_rate, double max_range, const ScanWindow *win, const double pose[3],
                     ScanFilterScratch &s, int *kept) {
  // (a branch-free pass that writes one byte per point, then the bytes compacted into the index list)
  ScanFilterArgs fa{};
  fa.n = n;
  fa.range = range;
  fa.angle = angle;
  fa.is_occ = is_occ;
  fa.skip_rate = skip_rate;
  fa.max_range = max_range;
  fa.bounded = win ? 1 : 0;
  if (win) {
    fa.trig_raw = t.trig_mode == 1 ? 0 : 1;
    fa.cos_a = t.cos_a.data();
    fa.sin_a = t.sin_a.data();
    for (int q = 0; q < 3; ++q) fa.pose[q] = pose[q];
    fa.scale = win->scale;
    fa.origin_x = win->origin_x;
    fa.origin_y = win->origin_y;
    fa.width = win->width;
    fa.height = win->height;
    if (fa.trig_raw) s.trig.resize(2 * (size_t)n);
  }
  s.mask.resize(n);
  scan_filter_mask(fa, s.mask.data(), s.trig.data());
  return scan_filter_compact(s.mask.data(), n, kept);
}

int scan_stage_rows(const ScanTables &t, int n, const double *range, const double *angle, const double *factor,
                    int weighting, int k, const int *kept, const ScanStageRows &rows, double *w_viny,
                    ScanStageScratch &s, double *w_even, double *tot_w) {
  // (the rows that are gathered through the kept list -- ranges, factors, the viny weights -- in ONE sweep over it:
  // scan_filter_fill)
  if (k == n) std::memcpy(rows.range, range, sizeof(double) * k);
  else std::memcpy(rows.kept, kept, sizeof(int) * k);
  const double tot_viny = scan_filter_fill(k, kept, range, factor, t.viny_f.data(), k == n ? nullptr : rows.range,
                                           factor ? rows.factor : nullptr, weighting == 1 ? w_viny : nullptr);
  *w_even = 0.0;
  if (weighting == 0) {
    *w_even = 1.0 / k;  // EvenSPW (:21-32)
    *tot_w = scan_total_weight_even(k, *w_even);
  } else if (weighting == 1) {
    *tot_w = tot_viny;  // (the same additions in the same order)
  } else {
    s.a.resize(k);
    s.r.resize(k);
    s.w.resize(k);
    for (int q = 0; q < k; ++q) {
      s.a[q] = angle[kept[q]];
      s.r[q] = range[kept[q]];
    }
    const int rc = scan_weights(2, k, s.r.data(), s.a.data(), s.w.data());
    if (rc) return rc;
    std::memcpy(rows.weight, s.w.data(), sizeof(double) * k);
    *tot_w = scan_total_weight(s.w.data(), k);
  }
  return kScanOk;
}

int RawBatchStage::prepare(int n_jobs, const RawBatchJob *jobs, size_t args_entry_bytes, int dst_rows) {
  for (int c = 0; c < n_jobs; ++c) {
    const RawBatchJob &j = jobs[c];
    if (j.n <= 0 || !j.range || !j.angle) return kScanBadArgs;
    if (j.weighting < 0 || j.weighting > 2) return kScanBadWeighting;
  }
  ++call;
  plan.assign(n_jobs, RawBatchPlan{});
  kept.clear();
  n_live = max_stride = max_k = 0;
  dst_doubles = 0;
  size_t total_n = 0;
  for (int c = 0; c < n_jobs; ++c) total_n += (size_t)jobs[c].n;
  kept.resize(total_n);
  size_t kept_at = 0;
  for (int c = 0; c < n_jobs; ++c) {
    const RawBatchJob &j = jobs[c];
    RawBatchPlan &p = plan[c];
    // the job's scanner: one that is known (jobs of one call with equal scanners share it, a later call finds it), else
    // built in the place of the one that has gone unused longest once kSlotsKept are held
    int at = -1;
    for (int q = 0; q < (int)slots.size() && at < 0; ++q)
      if (slots[q].t.same(j.n, j.angle, j.trig_mode, j.a_min, j.a_max, j.a_inc)) at = q;
    if (at < 0) {
      if ((int)slots.size() >= kSlotsKept) {
        for (int q = 0; q < (int)slots.size(); ++q)
          if (slots[q].used < call && (at < 0 || slots[q].used < slots[at].used)) at = q;
      }
      const bool added = at < 0;
      if (added) {
        slots.emplace_back();
        at = (int)slots.size() - 1;
      }
      slots[at].fresh = true;
      const int rc = scan_tables_build(slots[at].t, j.n, j.angle, j.trig_mode, j.a_min, j.a_max, j.a_inc);
      if (rc) {
        if (added) slots.pop_back();  // (a taken-over slot stays, empty: it matches no scanner)
        return rc;
      }
    }
    slots[at].used = call;
    p.table = at;
    p.weighting = j.weighting;
    p.kept_at = kept_at;
    p.k = scan_filter_kept(slots[at].t, j.n, j.range, j.angle, j.is_occ, j.skip_rate, j.max_range,
                           j.bounded ? &j.win : nullptr, j.pose, fs, kept.data() + kept_at);
    kept_at += (size_t)p.k;
    if (p.k > 0) p.live = n_live++;
    max_k = p.k > max_k ? p.k : max_k;
  }
  // the arena: the args table, then per live job its rows -- only what is new with each scan
  auto align16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
  size_t at = align16(args_entry_bytes * (size_t)n_live);
  for (int c = 0; c < n_jobs; ++c) {
    const RawBatchJob &j = jobs[c];
    RawBatchPlan &p = plan[c];
    if (p.k == 0) continue;
    const size_t k = (size_t)p.k;
    p.off_range = at;
    at = align16(at + sizeof(double) * k);
    if (p.k < j.n) {
      p.off_kept = at;
      at = align16(at + sizeof(int) * k);
    }
    if (j.factor) {
      p.off_factor = at;
      at = align16(at + sizeof(double) * k);
    }
    if (j.weighting == 2) {
      p.off_weight = at;
      at = align16(at + sizeof(double) * k);
    }
    p.stride = (k + 7) & ~(size_t)7;
    p.dst_at = dst_doubles;
    dst_doubles += (size_t)dst_rows * p.stride;
    max_stride = (int)p.stride > max_stride ? (int)p.stride : max_stride;
  }
  arena_bytes = at;
  return kScanOk;
}

int RawBatchStage::fill(const RawBatchJob *jobs, unsigned char *arena) {
  for (int c = 0; c < (int)plan.size(); ++c) {
    const RawBatchJob &j = jobs[c];
    RawBatchPlan &p = plan[c];
    if (p.k == 0) continue;
    ScanStageRows rows{};
    rows.range = reinterpret_cast<double *>(arena + p.off_range);
    if (p.off_kept != kNoRow) rows.kept = reinterpret_cast<int *>(arena + p.off_kept);
    if (p.off_factor != kNoRow) rows.factor = reinterpret_cast<double *>(arena + p.off_factor);
    if (p.off_weight != kNoRow) rows.weight = reinterpret_cast<double *>(arena + p.off_weight);
    if (j.weighting == 1) w_viny.resize(p.k);
    const int rc = scan_stage_rows(slots[p.table].t, j.n, j.range, j.angle, j.factor, j.weighting, p.k,
                                   kept.data() + p.kept_at, rows, w_viny.data(), ss, &p.w_even, &p.tot_w);
    if (rc) return rc;
  }
  return kScanOk;
}

void RawBatchStage::entry(int c, const unsigned char *arena, const ScanTablePlanes &tab, double *dst_base,
                          ScanAssembleArgs *out) const {
  const RawBatchPlan &p = plan[c];
  ScanAssembleArgs as{};
  as.h_range = reinterpret_cast<const double *>(arena + p.off_range);
  if (p.off_kept != kNoRow) as.h_kept = reinterpret_cast<const int *>(arena + p.off_kept);
  if (p.off_factor != kNoRow) as.h_factor = reinterpret_cast<const double *>(arena + p.off_factor);
  if (p.off_weight != kNoRow) as.h_weight = reinterpret_cast<const double *>(arena + p.off_weight);
  as.tab_cos = tab.cos_a;
  as.tab_sin = tab.sin_a;
  if (p.weighting == 1) as.tab_viny = tab.viny_f;
  as.dst = dst_base + p.dst_at;
  as.stride = p.stride;
  as.n = p.k;
  as.w_even = p.w_even;
  *out = as;
}

}  // namespace slamhip
