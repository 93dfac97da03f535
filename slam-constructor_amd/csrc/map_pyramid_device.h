// map_pyramid_device.h -- the max-impact levels over a grid map (include/slamhip.h "map pyramid"), stated once for the
// host (slamhip_pyramid_build_host) and the device (csrc/map_pyramid.hip).
//
// What it restates (paths relative to the reference root):
//   M3RSMRescalableGridMap                         src/core/scan_matchers/m3rsm_engine.h:17-131
//   RescalableCachingGridMap (the list of levels)  src/core/maps/rescalable_caching_grid_map.h:27-42,171-194
//   ObservationImpactEstimator::estimate_obstacle_impact over DiscrepancyOIE / OccupancyOIE
//                                                  src/core/scan_matchers/observation_impact_estimators.h:14-28
//
// A level cell is the copy of ONE fine cell: of the known fine cells of its block, the one of largest impact.  The
// order "better" below is total -- impact first (by pyr_key, which orders doubles as numbers, -0 below +0, and is
// defined on every bit pattern), then the smaller fine x, then the smaller fine y -- so the winner of a block does not
// depend on how the block is cut into pieces: a level made from the level below it (2 x 2 winners, each carrying the
// fine coordinate it came from) holds what a scan of the whole block would.
//
// Everything is FP64 in the reference's operation order; compile with -ffp-contract=off.
#pragma once

#include "slamhip_internal.h"

#if defined(__HIPCC__)
#define SLAMHIP_PYR_FN __host__ __device__ static inline
#else
#define SLAMHIP_PYR_FN static inline
#endif

namespace slamhip {
namespace pyr {

constexpr int kMaxLevels = 34;  // 2^31 cells a side at most: 31 doublings, the 1 x 1 level, the fine map

// estimate_obstacle_impact of a cell: cell_probability<MODEL>(oie, payload) of score_device.h, operation for operation
// (belief cells know the discrepancy OIE only: check_oie)
SLAMHIP_PYR_FN double impact(int model, int oie, const double *p) {
  if (cell_is_belief(model)) return belief_probability(model, p[0], p[1], p[2], p[3]);
  if (oie == SLAMHIP_OIE_OCCUPANCY) return p[0];
  return 1.0 - __builtin_fabs(p[0] - 1.0);
}

// a double as an integer that compares the way the number does
SLAMHIP_PYR_FN long long key(double v) {
  long long b;
  __builtin_memcpy(&b, &v, 8);
  return b ^ ((b >> 63) & 0x7fffffffffffffffll);
}

// "known": the payload is not bit-equal to the map's unknown payload (CD doubles)
template <int CD>
SLAMHIP_PYR_FN bool known(const double *p, const double *unknown) {
  for (int k = 0; k < CD; ++k) {
    long long a, b;
    __builtin_memcpy(&a, p + k, 8);
    __builtin_memcpy(&b, unknown + k, 8);
    if (a != b) return true;
  }
  return false;
}

SLAMHIP_PYR_FN bool better(long long k, int fx, int fy, long long bk, int bfx, int bfy) {
  if (k != bk) return k > bk;
  if (fx != bfx) return fx < bfx;
  return fy < bfy;
}

// One level as the kernels and the host see it: `cd` doubles per cell at `pitch` cells per row; coord = per cell the
// EXTERNAL fine coordinate (x, y) its payload was copied from (null for the fine map: a cell's own).
struct Level {
  double *payload;
  int *coord;
  int width, height, pitch;
  int origin_x, origin_y;
};

// Cell (ix, iy), internal, of `dst` from the 2 x 2 cells of `src` under it: src cells at internal
// (2 ix + bias_x + {0, 1}, 2 iy + bias_y + {0, 1}), those outside src's window being unknown.
// bias = src.origin - 2 dst.origin for a level that halves (floor(x / 2) of EXTERNAL coordinates: the origins are what
// makes it a floor for negative ones), 0 for the 1 x 1 level over a src of at most 2 x 2 cells.
template <int CD>
SLAMHIP_PYR_FN void reduce_cell(const Level &src, const Level &dst, int bias_x, int bias_y, int model, int oie,
                                const double *unknown, int ix, int iy) {
  long long bk = 0;
  int bfx = 0, bfy = 0;
  const double *best = nullptr;
  for (int dx = 0; dx < 2; ++dx)
    for (int dy = 0; dy < 2; ++dy) {
      const long long sx = 2ll * ix + bias_x + dx, sy = 2ll * iy + bias_y + dy;
      if (sx < 0 || sx >= src.width || sy < 0 || sy >= src.height) continue;
      const size_t at = (size_t)sy * src.pitch + (size_t)sx;
      const double *p = src.payload + at * CD;
      if (!known<CD>(p, unknown)) continue;
      const long long k = key(impact(model, oie, p));
      const int fx = src.coord ? src.coord[2 * at] : (int)sx - src.origin_x;
      const int fy = src.coord ? src.coord[2 * at + 1] : (int)sy - src.origin_y;
      if (!best || better(k, fx, fy, bk, bfx, bfy)) {
        best = p;
        bk = k;
        bfx = fx;
        bfy = fy;
      }
    }
  const size_t to = (size_t)iy * dst.pitch + (size_t)ix;
  for (int k = 0; k < CD; ++k) dst.payload[to * CD + k] = best ? best[k] : unknown[k];
  dst.coord[2 * to] = bfx;
  dst.coord[2 * to + 1] = bfy;
}

// floor(v / 2^k) for k < 31
inline int floor_shift(int v, int k) { return v >> k; }

// The list of levels over a fine window of w x h cells whose external cell (0, 0) sits at internal (ox, oy).
// RescalableCachingGridMap keeps adding levels between the finest map and the 1 x 1 one until the last of them is at
// most 2 x 2 cells (ensure_map_cache_is_continuous); a level's own window is centred -- external cell (0, 0) at
// (width / 2, height / 2) -- when it is made and grows around the cells that are written, so the 2 x 2 level holds the
// external coarse cells -1 and 0 and is left alone exactly when every fine cell lies in [-2^k, 2^k) in x and in y.  Hence:
//   the last halving level k_last = the smallest k >= 0 with 2^k >= max(ox, w - ox, oy, h - oy)   (0: none at all)
//   level k, 1 <= k <= k_last: the coarse cells floor(x / 2^k) of the fine cells, a tight window
//   level k_last + 1: one cell of infinite scale, external (0, 0) at internal (0, 0).
// n (out) = k_last + 1 levels above the fine map; arrays of kMaxLevels.
struct Plan {
  int n;
  int width[kMaxLevels], height[kMaxLevels], origin_x[kMaxLevels], origin_y[kMaxLevels];
  double scale[kMaxLevels];
};
inline bool plan_levels(int w, int h, int ox, int oy, double scale, Plan *pl) {
  if (w <= 0 || h <= 0) return false;
  const long long x_lo = -(long long)ox, x_hi = (long long)w - 1 - ox, y_lo = -(long long)oy, y_hi = (long long)h - 1 - oy;
  if (x_lo < -(1ll << 30) || x_hi >= (1ll << 30) || y_lo < -(1ll << 30) || y_hi >= (1ll << 30)) return false;
  int k_last = 0;
  while (x_lo < -(1ll << k_last) || x_hi >= (1ll << k_last) || y_lo < -(1ll << k_last) || y_hi >= (1ll << k_last)) ++k_last;
  double s = scale;
  for (int k = 1; k <= k_last; ++k) {
    s = s * 2;
    const int X0 = floor_shift((int)x_lo, k), X1 = floor_shift((int)x_hi, k);
    const int Y0 = floor_shift((int)y_lo, k), Y1 = floor_shift((int)y_hi, k);
    pl->width[k - 1] = X1 - X0 + 1;
    pl->height[k - 1] = Y1 - Y0 + 1;
    pl->origin_x[k - 1] = -X0;
    pl->origin_y[k - 1] = -Y0;
    pl->scale[k - 1] = s;
  }
  pl->width[k_last] = pl->height[k_last] = 1;
  pl->origin_x[k_last] = pl->origin_y[k_last] = 0;
  pl->scale[k_last] = __builtin_inf();
  pl->n = k_last + 1;
  return true;
}

// the cells of level `lv` (1-based; width x height, origin as planned) whose blocks meet the fine window
// [x0, x0 + w) x [y0, y0 + h) (internal fine coordinates, inside the fine map): internal [*cx0, *cx1] x [*cy0, *cy1]
inline void level_window(const Plan &pl, int fine_ox, int fine_oy, int lv, int x0, int y0, int w, int h, int *cx0, int *cy0,
                         int *cx1, int *cy1) {
  if (lv == pl.n) {
    *cx0 = *cy0 = *cx1 = *cy1 = 0;
    return;
  }
  *cx0 = floor_shift(x0 - fine_ox, lv) + pl.origin_x[lv - 1];
  *cx1 = floor_shift(x0 + w - 1 - fine_ox, lv) + pl.origin_x[lv - 1];
  *cy0 = floor_shift(y0 - fine_oy, lv) + pl.origin_y[lv - 1];
  *cy1 = floor_shift(y0 + h - 1 - fine_oy, lv) + pl.origin_y[lv - 1];
}

// belief cells are scored -- and bounded -- under the discrepancy OIE only (slamhip_score_poses)
inline bool check_oie(int model, int oie) {
  if (oie != SLAMHIP_OIE_DISCREPANCY && oie != SLAMHIP_OIE_OCCUPANCY) return false;
  return !(cell_is_belief(model) && oie != SLAMHIP_OIE_DISCREPANCY);
}

}  // namespace pyr
}  // namespace slamhip
