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

}  // namespace slamhip
