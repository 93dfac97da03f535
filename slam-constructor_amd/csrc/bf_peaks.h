// bf_peaks.h -- the local maxima of a brute-force sweep's score landscape: THE rule, one text for the host
// (slamhip_bf_peaks_host, matchers.cpp) and the device (bf_peaks.hip).  Plain C++: no HIP, no other header of the library;
// tests/native/bf_peaks_test.cpp compiles this file alone with g++.
//
// The volume is V[it][iy][ix] = scores[ix + nx (iy + ny it)], the enumerator's lattice (x fastest, then y, then theta);
// index j is 0-based: pose j of the lattice is call j + 1 of the sweep.
//   key order   a beats b  iff  s_a > s_b, or s_a == s_b and a < b -- the lower index is the pose the enumerator hands
//               out first, the matcher's own "first pose holding the maximum" (pose_enumeration_scan_matcher.h:56).  A NaN
//               score is absent: it beats nothing and is never a peak.
//   window      W(i): |dix| <= rx, |diy| <= ry, |dit| <= rt, clipped at the faces of the volume; theta does not wrap.
//   peak        s_i is not NaN and no j != i in W(i) beats i.  Radius (0, 0, 0): every non-NaN point ("N best poses").
//   floors      s_max = the largest non-NaN score of the lattice; a peak is kept iff
//               s_i >= min_score && s_i >= min_ratio * s_max  (literally: one multiplication, two comparisons).
//   result      kept peaks in descending score, ties by ascending index; n_found of them, the first max_peaks written.
//   bound       two peaks are never inside each other's window: at most one per block of the partition into
//               (rx + 1) x (ry + 1) x (rt + 1) boxes, B = ceil(nx / (rx + 1)) ceil(ny / (ry + 1)) ceil(nt / (rt + 1)).
// The window maximum of a box is the maximum of per-axis maxima and the key order is total on non-NaN points, so the rule
// is separable: x, then y, then theta over (score, index) pairs; i is a peak iff the box maximum's index is i.
#pragma once

#include <algorithm>
#include <vector>

#if defined(__HIPCC__)
#define SLAMHIP_BF_PEAKS_HD __host__ __device__
#else
#define SLAMHIP_BF_PEAKS_HD
#endif

namespace slamhip {

constexpr int kBfPeaksMaxRadius = 32;
constexpr long long kBfPeaksMaxSurvivors = 8192;  // B and max_peaks: 8192 records of 16 bytes

// a lattice point as the passes hand it on; index < 0: no (non-NaN) point
struct BfPeakKey {
  double score;
  long long index;
};

SLAMHIP_BF_PEAKS_HD inline bool bf_peak_isnan(double s) { return s != s; }

// a beats b (both present, neither score NaN)
SLAMHIP_BF_PEAKS_HD inline bool bf_peak_beats(double sa, long long a, double sb, long long b) {
  return sa > sb || (sa == sb && a < b);
}

// the better of two keys, absent ones (index < 0) losing to present ones
SLAMHIP_BF_PEAKS_HD inline BfPeakKey bf_peak_better(BfPeakKey a, BfPeakKey b) {
  if (b.index < 0) return a;
  if (a.index < 0) return b;
  return bf_peak_beats(b.score, b.index, a.score, a.index) ? b : a;
}

// the key of lattice point i
SLAMHIP_BF_PEAKS_HD inline BfPeakKey bf_peak_key_of(const double *scores, long long i) {
  const double s = scores[i];
  return BfPeakKey{s, bf_peak_isnan(s) ? -1ll : i};
}

// the floors, literally
SLAMHIP_BF_PEAKS_HD inline bool bf_peak_kept(double s, double s_max, double min_ratio, double min_score) {
  return s >= min_score && s >= min_ratio * s_max;
}

// B; 0 for an empty volume
SLAMHIP_BF_PEAKS_HD inline long long bf_peaks_bound(int nx, int ny, int nt, const int radius[3]) {
  const long long bx = (nx + radius[0]) / (radius[0] + 1), by = (ny + radius[1]) / (radius[1] + 1),
                  bt = (nt + radius[2]) / (radius[2] + 1);
  return bx * by * bt;
}

// whether (nx, ny, nt, radius) is a call the rule takes: a non-empty volume, 0 <= r <= 32
SLAMHIP_BF_PEAKS_HD inline bool bf_peaks_shape_ok(int nx, int ny, int nt, const int radius[3]) {
  if (nx <= 0 || ny <= 0 || nt <= 0) return false;
  for (int k = 0; k < 3; ++k)
    if (radius[k] < 0 || radius[k] > kBfPeaksMaxRadius) return false;
  return true;
}

// ---- host forms ----------------------------------------------------------------------------------------------------

// descending score, ties by ascending index
inline void bf_peaks_order(std::vector<BfPeakKey> &v) {
  std::sort(v.begin(), v.end(), [](const BfPeakKey &a, const BfPeakKey &b) { return bf_peak_beats(a.score, a.index, b.score, b.index); });
}

// s_max and whether there is one
inline bool bf_peaks_lattice_max(const double *scores, long long n, double *s_max) {
  bool any = false;
  double m = 0.0;
  for (long long i = 0; i < n; ++i) {
    const double s = scores[i];
    if (bf_peak_isnan(s)) continue;
    if (!any || s > m) m = s;
    any = true;
  }
  *s_max = m;
  return any;
}

// one axis of the separable form: out[p] = the best key of in[] over |d| <= r along an axis of `len` points `stride` apart
inline void bf_peaks_axis_pass(const std::vector<BfPeakKey> &in, std::vector<BfPeakKey> &out, long long n, int len, long long stride,
                               int r) {
  for (long long p = 0; p < n; ++p) {
    const int c = (int)((p / stride) % len);
    const int lo = std::max(0, c - r), hi = std::min(len - 1, c + r);
    BfPeakKey best{0.0, -1};
    for (int q = lo; q <= hi; ++q) best = bf_peak_better(best, in[p + (long long)(q - c) * stride]);
    out[p] = best;
  }
}

// THE host routine, in the separable form: every kept peak, ordered.  The caller has checked the shape.
inline void bf_peaks_separable(const double *scores, int nx, int ny, int nt, const int radius[3], double min_ratio,
                               double min_score, std::vector<BfPeakKey> *kept) {
  kept->clear();
  const long long n = (long long)nx * ny * nt;
  double s_max = 0.0;
  if (!bf_peaks_lattice_max(scores, n, &s_max)) return;
  std::vector<BfPeakKey> a((size_t)n), b((size_t)n);
  for (long long i = 0; i < n; ++i) a[(size_t)i] = bf_peak_key_of(scores, i);
  bf_peaks_axis_pass(a, b, n, nx, 1, radius[0]);
  bf_peaks_axis_pass(b, a, n, ny, nx, radius[1]);
  bf_peaks_axis_pass(a, b, n, nt, (long long)nx * ny, radius[2]);
  for (long long i = 0; i < n; ++i)
    if (b[(size_t)i].index == i && bf_peak_kept(scores[i], s_max, min_ratio, min_score)) kept->push_back(BfPeakKey{scores[i], i});
  bf_peaks_order(*kept);
}

// ... and the definition as it reads, a triple loop over the window of every point (the native test compares the two)
inline void bf_peaks_brute(const double *scores, int nx, int ny, int nt, const int radius[3], double min_ratio, double min_score,
                           std::vector<BfPeakKey> *kept) {
  kept->clear();
  const long long n = (long long)nx * ny * nt;
  double s_max = 0.0;
  if (!bf_peaks_lattice_max(scores, n, &s_max)) return;
  for (int it = 0; it < nt; ++it)
    for (int iy = 0; iy < ny; ++iy)
      for (int ix = 0; ix < nx; ++ix) {
        const long long i = ix + (long long)nx * (iy + (long long)ny * it);
        const double s = scores[i];
        if (bf_peak_isnan(s)) continue;
        bool peak = true;
        for (int jt = std::max(0, it - radius[2]); peak && jt <= std::min(nt - 1, it + radius[2]); ++jt)
          for (int jy = std::max(0, iy - radius[1]); peak && jy <= std::min(ny - 1, iy + radius[1]); ++jy)
            for (int jx = std::max(0, ix - radius[0]); jx <= std::min(nx - 1, ix + radius[0]); ++jx) {
              const long long j = jx + (long long)nx * (jy + (long long)ny * jt);
              if (j != i && !bf_peak_isnan(scores[j]) && bf_peak_beats(scores[j], j, s, i)) {
                peak = false;
                break;
              }
            }
        if (peak && bf_peak_kept(s, s_max, min_ratio, min_score)) kept->push_back(BfPeakKey{s, i});
      }
  bf_peaks_order(*kept);
}

}  // namespace slamhip
