// scan_filter.h -- the raw scan's filter (WeightedMeanPointProbabilitySPE::filter_scan) as a branch-free keep-mask
// pass and a compaction pass, and the rest of a raw scan's host half -- per-beam tables, staged rows, weights -- for one
// scan or a batch of them (plain C++, no device code; see scan_filter.cpp).
#pragma once

#include <cstddef>
#include <vector>

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

// ---- the raw scan's host half, stated once for the lone call (scan_filter_stage, slamhip_api.cpp) and for a batch of
// raw scans (RawBatchStage below): per-beam tables of a scanner, the filter against a pose and a map window, the rows
// that go into pinned memory.  Error codes of everything below (scan_error_text gives the message):
enum { kScanOk = 0, kScanBadArgs = 1, kScanAngleOutsideTable = 2, kScanAhrBin = 3, kScanBadWeighting = 4 };
const char *scan_error_text(int code);

// RawTrigonometryProvider / CachedTrigonometryProvider (slamhip_beam_trig_raw / _cached are these two)
int beam_trig_raw(int n, const double *angle, double *cos_out, double *sin_out);
int beam_trig_cached(int n, const double *angle, double a_min, double a_max, double a_inc, double *cos_out, double *sin_out);
// ScanPointWeighting::weight of a FILTERED scan: kind 0 even, 1 viny, 2 ahr (slamhip_scan_weights is this)
int scan_weights(int kind, int n, const double *range, const double *angle, double *out);
// the total weight, in beam order; of k even weights w (the same k additions, kept per k)
double scan_total_weight(const double *weight, int n);
double scan_total_weight_even(int k, double w);

// What depends on the scanner alone: cos / sin per raw beam as the scan's trig provider tabulates them, the viny
// weighting's angular factor.
struct ScanTables {
  std::vector<double> angle, cos_a, sin_a, viny_f;
  int trig_mode = -1;
  double a_min = 0, a_max = 0, a_inc = 0;
  bool same(int n, const double *angle_, int trig_mode_, double a_min_, double a_max_, double a_inc_) const;
};
// (on an error the tables are left empty: they match no scanner)
int scan_tables_build(ScanTables &t, int n, const double *angle, int trig_mode, double a_min, double a_max, double a_inc);

struct ScanWindow {
  double scale;
  int origin_x, origin_y, width, height;
};
struct ScanFilterScratch {
  std::vector<unsigned char> mask;
  std::vector<double> trig;
};
// filter_scan of one raw scan of t's scanner at `pose`; win null: the map has no rim.  kept: room for n indices;
// returns how many were kept.
int scan_filter_kept(const ScanTables &t, int n, const double *range, const double *angle, const int *is_occ,
                     unsigned skip_rate, double max_range, const ScanWindow *win, const double pose[3],
                     ScanFilterScratch &s, int *kept);

// Where the rows of one filtered scan go (pinned memory): range always, kept where k < n, factor where the caller has
// factors, weight where the weighting makes its weights from the scan's shape (ahr).
struct ScanStageRows {
  double *range;
  int *kept;
  double *factor, *weight;
};
struct ScanStageScratch {
  std::vector<double> a, r, w;
};
// Fills them (k > 0 kept points of n raw ones).  w_viny: room for k doubles, written under weighting 1 (the host's copy
// of the weights the device makes from tab_viny), else not touched.  *w_even: 1.0 / k under weighting 0.  *tot_w: the
// scan's total weight in index order.
int scan_stage_rows(const ScanTables &t, int n, const double *range, const double *angle, const double *factor,
                    int weighting, int k, const int *kept, const ScanStageRows &rows, double *w_viny,
                    ScanStageScratch &s, double *w_even, double *tot_w);

// What the assembly kernels are launched with (score_kernels.hip, scan_assemble_device.h).  The scan block `dst` (five
// rows of `stride` doubles) from n kept points' ranges in pinned memory and the scanner's resident per-beam tables;
// h_kept (raw index per point) null = every beam kept, h_factor null = 1.0, h_weight null = tab_viny[i] * sqrt(range)
// where tab_viny is given, else w_even.
struct ScanAssembleArgs {
  const double *h_range;
  const int *h_kept;
  const double *h_factor, *h_weight;
  const double *tab_cos, *tab_sin, *tab_viny;
  double *dst;
  size_t stride;
  int n;
  double w_even;
};
// ... with a sixth row, angle[kept[q]] from the scanner's angle plane in HBM (six rows of `stride` doubles at a.dst)
struct ScanAssembleEachArgs {
  ScanAssembleArgs a;
  const double *tab_angle;
};
// the planes of a scanner's tables in HBM (ScanTablesDevice, scan_tables_device.h); angle null where nobody keeps that plane
struct ScanTablePlanes {
  const double *cos_a, *sin_a, *viny_f, *angle;
};

// ---- K raw scans of one call (slamhip_matcher_process_raw_scan_batch, slamhip_matcher_m3rsm_match_each_raw): the filter
// and the rows per job, the scanners' tables kept between calls, ONE arena in pinned memory laid out for one assembly
// launch.
struct RawBatchJob {
  int n;
  const double *range, *angle;
  const int *is_occ;
  const double *factor;
  int trig_mode;
  double a_min, a_max, a_inc;
  unsigned skip_rate;
  double max_range;
  int bounded, weighting;
  double pose[3];
  ScanWindow win;  // read where bounded
};
constexpr size_t kNoRow = ~(size_t)0;
struct RawBatchPlan {
  int k = 0;       // points kept; 0: the job takes no part in the launches (nothing of it is in the arena)
  int table = -1;  // its scanner's slot
  int live = -1;   // its place among the jobs that kept something (its entry of the args table)
  int weighting = 0;
  size_t kept_at = 0;                                                               // its kept list in RawBatchStage::kept
  size_t off_range = kNoRow, off_kept = kNoRow, off_factor = kNoRow, off_weight = kNoRow;  // bytes into the arena
  size_t dst_at = 0, stride = 0;  // its block of dst_rows rows, doubles into the batch's arena in HBM
  double w_even = 0, tot_w = 0;
};
struct RawBatchStage {
  struct Slot {
    ScanTables t;
    unsigned long long used = 0;  // the last call that asked for it
    bool fresh = false;           // built or rebuilt: its copy in HBM is still to be made (the caller clears this)
  };
  static constexpr int kSlotsKept = 64;  // scanners kept between calls (a call may use more)
  std::vector<Slot> slots;
  unsigned long long call = 0;
  std::vector<RawBatchPlan> plan;
  std::vector<int> kept;
  int n_live = 0, max_stride = 0, max_k = 0;
  size_t arena_bytes = 0, dst_doubles = 0;
  ScanFilterScratch fs;
  ScanStageScratch ss;
  std::vector<double> w_viny;
  // Pass 1: arguments checked, scanners found or built, every job filtered, the arena laid out -- the args table of
  // n_live entries of args_entry_bytes at offset 0, the rows behind it, every row 16-byte aligned.  dst_rows: the rows
  // of `stride` doubles a job's block in HBM has (five; six where the kept points' angles ride along as a sixth row).
  int prepare(int n_jobs, const RawBatchJob *jobs, size_t args_entry_bytes, int dst_rows = 5);
  // Pass 2: the rows of every live job written into `arena` (arena_bytes long), weights and their sums made.
  int fill(const RawBatchJob *jobs, unsigned char *arena);
  // Live job c's entry of the args table: its rows in `arena`, its scanner's planes, its block at dst_base + dst_at.
  void entry(int c, const unsigned char *arena, const ScanTablePlanes &tab, double *dst_base, ScanAssembleArgs *out) const;
  void entry(int c, const unsigned char *arena, const ScanTablePlanes &tab, double *dst_base, ScanAssembleEachArgs *out) const {
    entry(c, arena, tab, dst_base, &out->a);
    out->tab_angle = tab.angle;
  }
  // a raw scan as the C-ABI states it (slamhip_raw_scan), matched from `pose` on a map with window `win`
  template <class Scan>
  static RawBatchJob job_of(const Scan &s, const double pose[3], const ScanWindow &win) {
    return RawBatchJob{s.n,     s.range, s.angle,     s.is_occ,    s.factor,          s.trig_mode, s.a_min,
                       s.a_max, s.a_inc, s.skip_rate, s.max_range, s.bounded ? 1 : 0, s.weighting, {pose[0], pose[1], pose[2]},
                       win};
  }
};

}  // namespace slamhip
