// scan_filter.h -- the raw scan's filter (WeightedMeanPointProbabilitySPE::filter_scan) as a branch-free keep-mask
// pass and a compaction pass (plain C++, no device code; see scan_filter.cpp).
#pragma once

namespace slamhip {

struct ScanFilterArgs {
  int n;
  const double *range, *angle;
  const int *is_occ;    // null: every point counts as occupied
  unsigned skip_rate;   // 0 or 1: every point; else the points whose index is a multiple
  double max_range;     // <= -epsilon: no usable range set
  int bounded;          // 0: the map has no rim -- nothing below is read
  int trig_raw;         // 1 (SLAMHIP_TRIG_RAW): ::sincos(pose[2] + angle[i]) per beam; 0: the tabulated cos_a / sin_a
  const double *cos_a, *sin_a;
  double pose[3];
  double scale;
  int origin_x, origin_y, width, height;
};

// `variant` of every function: -1 = what the CPU has, 0 = the baseline x86-64 clone, 1 = the AVX2 clone (the caller
// has asked scan_filter_has_avx2).
bool scan_filter_has_avx2();

// Pass 1: mask[i] = 1 where filter_scan keeps point i, else 0, for all n points; returns how many are kept.
// tmp: room for 2 n doubles, touched only where trig_raw and bounded are both set.
int scan_filter_mask(const ScanFilterArgs &a, unsigned char *mask, double *tmp, int variant = -1);

// Pass 2: the kept indices, ascending (room for n of them); returns their number ...
int scan_filter_compact(const unsigned char *mask, int n, int *kept);
// ... and the rows that go with them, each where its destination is given: r_out[q] = range[kept[q]],
// f_out[q] = factor[kept[q]], w_out[q] = viny_f[kept[q]] * sqrt(range[kept[q]]).  Returns the sum of w_out in index
// order (0 without w_out).
double scan_filter_fill(int k, const int *kept, const double *range, const double *factor, const double *viny_f,
                        double *r_out, double *f_out, double *w_out, int variant = -1);

}  // namespace slamhip
