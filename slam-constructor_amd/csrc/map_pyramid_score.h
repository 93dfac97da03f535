// map_pyramid_score.h -- what map_pyramid.hip (levels, k_pyr_score) and m3rsm.hip (k_m3rsm_expand) share: the pyramid
// object, the arguments of a bound-scoring launch and the per-candidate scoring body both kernels run.
#pragma once

#include <vector>

#include "map_pyramid_device.h"
#include "score_device.h"

struct slamhip_pyramid {
  slamhip_ctx *ctx = nullptr;  // null once the context has gone
  int fine_id = -1, first_id = -1, oie = 0;
  int cell_model = 0;
  // the fine map the levels were planned for: a re-bound (grown) fine map needs slamhip_pyramid_rebuild
  int fine_w = 0, fine_h = 0, fine_ox = 0, fine_oy = 0;
  const double *fine_payload = nullptr;
  slamhip::pyr::Plan plan{};
  std::vector<int *> d_coord;               // per level: the fine coordinate of every cell's winner (x, y)
  std::vector<const double *> lv_payload;   // per level: the payload the table below points at
  slamhip::MapView *d_views = nullptr;      // plan.n + 1 views, the fine map first
  // slamhip_pyramid_score_matches' staging in HBM: rotation | rect | sin, cos per candidate; scores; levels; terms
  double *d_in = nullptr, *d_scores = nullptr, *d_terms = nullptr;
  int *d_levels = nullptr;
  int in_cap = 0;
  size_t terms_cap = 0;
  // slamhip_pyramid_expand_matches' staging (m3rsm.hip): parents as above; per slot rect | score | level in one block;
  // h_x: the pinned host side of both
  double *d_x_in = nullptr, *d_x_out = nullptr, *h_x = nullptr;
  int x_parent_cap = 0;
  size_t x_slot_cap = 0;
};

namespace slamhip {

constexpr int kPyrThreads = 256;

struct MatchArgs {
  const MapView *levels;  // n_levels views, the fine map first
  int n_levels;
  ScanView scan;
  const double *rotation;  // n
  const double *rect;      // n x (bot, top, left, right)
  const double *pose_sc;   // optional n x (sin, cos) of rotation + heading from the host; null = device sincos
  double base[3];
  double *scores;
  int *level_out;
  double *terms;  // beam-order sum only: n x scan.n
  int n, oie, oope;
};

// map_pyramid.hip
int pyr_invalid(const char *msg);
int pyr_state(const char *msg);
int pyr_check_fresh(const slamhip_pyramid *p);
int pyr_check_score_cfg(const slamhip_pyramid *p, const slamhip_spe_cfg *cfg);
int pyr_fill_args(slamhip_pyramid *p, const slamhip_spe_cfg *cfg, const double base[3], size_t n_out, MatchArgs *a);
void pyr_free_staging(slamhip_pyramid *p);
// the reference's beam-order sum over the stored terms, for every output that has a level
int pyr_launch_sum_sequential(const MatchArgs &a, size_t n_out, hipStream_t stream);

#if defined(__HIPCC__)
// Match::prob_upper_bound of ONE candidate by the whole workgroup (kPyrThreads threads): rotation index `src` (into
// a.rotation / a.pose_sc), the rectangle in registers, the result at index `out` of a.scores / a.level_out / a.terms.
// Every thread of the workgroup calls it with the same arguments.
template <int MODEL>
__device__ __forceinline__ void pyr_score_one(const MatchArgs &a, size_t src, size_t out, double bot, double top, double left,
                                              double right, double *s_trig, double *s_part) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int n = a.scan.n;
  const double vside = top - bot, hside = right - left;
  // (a rectangle that is no rectangle -- NaN, infinite or reversed -- has no level and no window: NaN, level -1)
  if (!(vside >= 0.0 && hside >= 0.0 && vside < __builtin_inf() && hside < __builtin_inf())) {
    if (t == 0) {
      a.scores[out] = __builtin_nan("");
      a.level_out[out] = -1;
    }
    return;
  }
  // RescalableCachingGridMap::rescale(std::max(vside, hside)): the first level whose scale holds the target
  const double target = vside < hside ? hside : vside;
  int lv = 0;
  while (lv < a.n_levels - 1 && !(target <= a.levels[lv].scale)) ++lv;
  const MapView map = a.levels[lv];
  // LightWeightRectangle::center() added to the pose
  const double x = a.base[0] + (left + hside / 2), y = a.base[1] + (bot + vside / 2);
  if (t == 0) {
    double sn, cs;
    if (a.pose_sc) {
      sn = a.pose_sc[2 * src];
      cs = a.pose_sc[2 * src + 1];
    } else {
      sincos(a.rotation[src] + a.base[2], &sn, &cs);
    }
    s_trig[0] = sn;
    s_trig[1] = cs;
  }
  __syncthreads();
  const double sn = s_trig[0], cs = s_trig[1];
  const double half_v = (top - bot) / 2, half_h = (right - left) / 2;
  double acc = 0.0;
  for (int b = t; b < n; b += kPyrThreads) {
    const double ca = a.scan.cos_a[b], sa = a.scan.sin_a[b], r = a.scan.range[b];
    const double c = cs * ca - sn * sa;
    const double s = sn * ca + cs * sa;
    const double ox = x + r * c, oy = y + r * s;
    const double pr = window_probability<MODEL>(map, a.oie, a.oope, half_v, half_h, ox, oy);
    const double term = pr * a.scan.weight[b] * a.scan.factor[b];
    if (a.terms) a.terms[out * n + b] = term;
    acc = acc + term;
  }
  acc = wave_xor_sum(acc);
  if (lane == 0) s_part[wave] = acc;
  __syncthreads();
  if (t == 0) {
    const double total = (s_part[0] + s_part[1]) + (s_part[2] + s_part[3]);
    a.scores[out] = (a.scan.tot_w == 0.0) ? __builtin_nan("") : total / a.scan.tot_w;
    a.level_out[out] = lv;
  }
}
#endif

}  // namespace slamhip
