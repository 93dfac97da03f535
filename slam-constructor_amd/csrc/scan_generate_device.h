// scan_generate_device.h -- one beam of LaserScanGenerator::laser_scan_2D (src/utils/data_generation/
// laser_scan_generator.h:35-80), restated once for the host and the device.
//
//   beam_dir = max_dist * (cos, sin)(a + theta)                      laser_scan_generator.h:49-50 (the raw provider's libm:
//                                                                    csrc/libm_exact.h with an explicit variant)
//   cells    = world_to_cells({robot, robot + beam_dir})             regular_squares_grid.h:56-101: the 4-connected walk,
//                                                                    its tie rule, the Bresenham list when the walk has
//                                                                    not arrived within cells_nm cells
//   first cell with !(double(map[cell]) < occ_threshold) whose bounds the ray meets twice: the hit
//                                                                    :52-77, Rectangle::find_intersections(Ray) =
//                                                                    ae_rect_ray (area_estimator_device.h)
//
// The cell list is the COMPLETE list of the reference: a walk that goes astray is thrown away as a whole, so a hit
// found on it is no hit.  sg_beam_sequential therefore keeps walking (without reading the map) after its first hit until
// the walk has arrived or has run out of cells, and scans Bresenham's list from the start in the second case.
// The wave form of csrc/scan_generate.hip evaluates the same walk 64 steps at a time from the closed form below.
//
// Everything is FP64 in the reference's operation order; compile with -ffp-contract=off.
#pragma once
#include <math.h>

#include "slamhip_internal.h"  // (first: the HIP qualifiers the next header's functions carry)

#include "area_estimator_device.h"
#include "libm_exact.h"

#if defined(__HIPCC__)
#define SLAMHIP_SG_FN __host__ __device__ static inline
#else
#define SLAMHIP_SG_FN static inline
#endif

namespace slamhip {
namespace sg {

// per-beam results (the status byte of slamhip_map_generate_scans); SG_TOUCH never leaves this header
enum { SG_NONE = 0, SG_HIT = 1, SG_ASSERT = 2, SG_TOUCH = 3 };

// a dense window of cells: `stride` doubles per cell (HBM: 1 or 4; a host payload: 1, 3 or 4), `pitch` cells per row
struct SgMap {
  const double *payload;
  int width, height, pitch, stride;
  int origin_x, origin_y;
  int model, occ_kind;
  double scale;
  double unknown_occ;  // double(prototype cell): what a cell outside the window reads as
};

struct SgBeam {
  double rx, ry;      // robot_point
  double dirx, diry;  // beam_dir
  double d_x, d_y;    // (robot + beam_dir) - robot, as world_to_cells forms it
  double ca, sa;      // cos / sin(a + theta)
  double scale;
  int bx, by, ex, ey;  // first and last cell of the segment
};

// double(map[cell]) (GridCell::operator double, grid_cell.h:18)
SLAMHIP_SG_FN double sg_cell_occ(const SgMap &m, int cx, int cy) {
  const unsigned ix = (unsigned)cx + (unsigned)m.origin_x, iy = (unsigned)cy + (unsigned)m.origin_y;
  if (ix >= (unsigned)m.width || iy >= (unsigned)m.height) return m.unknown_occ;
  const double *c = m.payload + ((size_t)iy * (size_t)m.pitch + ix) * (size_t)m.stride;
  if (cell_is_belief(m.model)) return cell_occupancy(m.model, m.occ_kind, c[0], c[1], c[2]);
  return c[0];
}

// One slot of a tile pool (tile_pool.h): GMAPPING cells of 4 doubles in 128 x 128-cell tiles, `table` the slot's
// tiles_y x tiles_x tile ids (0 = the shared unknown tile, whose cells hold the unknown payload).  double(map[cell]) is
// prob_occ, the cell's first double.
struct SgTiledMap {
  const double *pool;
  const int *table;
  int tiles_x, tiles_y;
  int origin_x, origin_y;  // virtual cell = external cell + origin
  double scale;
  double unknown_occ;  // what a cell outside the extent reads as
};

// the renderer's read (render_tiled_cell, map_render.hip); the bounds test in 64 bits: no cell coordinate the callers'
// limits admit reaches the table from outside the extent
SLAMHIP_SG_FN double sg_cell_occ(const SgTiledMap &m, int cx, int cy) {
  const long long vx = (long long)cx + m.origin_x, vy = (long long)cy + m.origin_y;
  if (vx < 0 || vx >= (long long)m.tiles_x * kTileSide || vy < 0 || vy >= (long long)m.tiles_y * kTileSide) return m.unknown_occ;
  const int ix = (int)vx, iy = (int)vy;
  const int tile = m.table[(iy >> kTileShift) * m.tiles_x + (ix >> kTileShift)];
  return m.pool[((size_t)tile * kTileCells + ((size_t)(iy & kTileMask) << kTileShift) + (ix & kTileMask)) * 4];
}

template <bool FMA>
SLAMHIP_SG_FN SgBeam sg_beam_setup(double x, double y, double theta, double a, double max_dist, double scale) {
  SgBeam b;
  const double ang = a + theta;
  libm_exact::sincos_<FMA>(ang, &b.sa, &b.ca);
  b.rx = x;
  b.ry = y;
  b.dirx = max_dist * b.ca;
  b.diry = max_dist * b.sa;
  const double end_x = x + b.dirx, end_y = y + b.diry;
  b.d_x = end_x - x;
  b.d_y = end_y - y;
  b.scale = scale;
  b.bx = (int)floor(x / scale);
  b.by = (int)floor(y / scale);
  b.ex = (int)floor(end_x / scale);
  b.ey = (int)floor(end_y / scale);
  return b;
}

// The ray against world_cell_bounds(cell) (regular_squares_grid.h:108-118): one intersection is a touch, two a hit at
// their midpoint; any other number is one of the reference's assertions (geometry_primitives.h:392,
// laser_scan_generator.h:64), and so is a scan point that world_to_cell does not put back into the cell (:71-74).
SLAMHIP_SG_FN int sg_test_cell(const SgBeam &b, int cx, int cy, double *range) {
  const ae::ae_rect r{b.scale * cy, b.scale * (cy + 1), b.scale * cx, b.scale * (cx + 1)};
  ae::ae_hits h;
  ae::ae_rect_ray(r, ae::ae_pt{b.rx, b.ry}, ae::ae_pt{b.dirx, b.diry}, h);
  const int n = ae::ae_count(h);
  if (n == 1) return SG_TOUCH;
  if (n != 2) return SG_ASSERT;
  const ae::ae_two t = ae::ae_first_two(h);
  const double px = (t.p0.x + t.p1.x) / 2, py = (t.p0.y + t.p1.y) / 2;
  const double ddx = b.rx - px, ddy = b.ry - py;
  const double rg = sqrt(ddx * ddx + ddy * ddy);  // std::pow(v, 2) is v * v
  // ScanPoint2D::move_origin(x, y, theta) (sensor_data.h:96-101): range * cos(a + theta) + x
  const double wx = rg * b.ca + b.rx, wy = rg * b.sa + b.ry;
  if ((int)floor(wx / b.scale) != cx || (int)floor(wy / b.scale) != cy) return SG_ASSERT;
  *range = rg;
  return SG_HIT;
}

// one cell of the list: SG_NONE = the scan of the list goes on.  Map: SgMap or SgTiledMap (sg_cell_occ is the one read)
template <class Map>
SLAMHIP_SG_FN int sg_visit(const Map &m, const SgBeam &b, double thr, int cx, int cy, double *range) {
  if (sg_cell_occ(m, cx, cy) < thr) return SG_NONE;
  const int r = sg_test_cell(b, cx, cy, range);
  return r == SG_TOUCH ? SG_NONE : r;
}

// The beam as the reference runs it, one cell after the other.  Returns the status, *range set on SG_HIT.
template <class Map>
SLAMHIP_SG_FN int sg_beam_sequential(const Map &m, const SgBeam &b, double thr, double *range) {
  const double scale = b.scale;
  const int inc_x = 0 < b.d_x ? 1 : -1, inc_y = 0 < b.d_y ? 1 : -1;
  int px = b.bx, py = b.by;
  const long long cells_nm = (long long)abs(b.ex - px) + (long long)abs(b.ey - py) + 1;
  const double mid_x = (px + 0.5) * scale, mid_y = (py + 0.5) * scale;
  const double mid_cell_seg_y = b.d_x * b.ry + (mid_x - b.rx) * b.d_y;
  double e = mid_cell_seg_y - mid_y * b.d_x;
  const double e_x_inc = inc_x * scale * b.d_y;
  const double e_y_inc = -inc_y * scale * b.d_x;
  int status = SG_NONE;
  double rg = 0.0;
  bool arrived;
  for (long long n = 0;;) {
    ++n;  // cells.push_back(pnt)
    if (status == SG_NONE) status = sg_visit(m, b, thr, px, py, &rg);
    if (px == b.ex && py == b.ey) {
      arrived = true;
      break;
    }
    if (cells_nm < n) {
      arrived = false;
      break;
    }
    const double e_x = e + e_x_inc, e_y = e + e_y_inc;
    const double abs_err_diff = fabs(e_y) - fabs(e_x);
    if (ae::ae_equal(abs_err_diff, 0.0)) {
      if (px == b.ex) py += inc_y;
      else if (py == b.ey) px += inc_x;
      else {
        px += inc_x;
        py += inc_y;
      }
      e = 0.0;
    } else if (0 < abs_err_diff) {
      px += inc_x;
      e = e_x;
    } else {
      py += inc_y;
      e = e_y;
    }
  }
  if (!arrived) {
    // DiscreteSegment2D{beg, end} (geometry_primitives.h, Bresenham): the list the reference returns instead
    status = SG_NONE;
    rg = 0.0;
    const int dxx = b.ex - b.bx, dyy = b.ey - b.by;
    const bool y_is_primary = abs(dxx) < abs(dyy);
    const int limit = y_is_primary ? b.ey : b.ex;
    int primary = y_is_primary ? b.by : b.bx, secondary = y_is_primary ? b.bx : b.by;
    const int d_primary = y_is_primary ? dyy : dxx, d_secondary = y_is_primary ? dxx : dyy;
    const int inc_primary = 0 < d_primary ? 1 : -1, inc_secondary = 0 < d_secondary ? 1 : -1;
    int error = 0;
    while (true) {
      const int cx = y_is_primary ? secondary : primary, cy = y_is_primary ? primary : secondary;
      status = sg_visit(m, b, thr, cx, cy, &rg);
      if (status != SG_NONE || primary == limit) break;
      const int err_inc_primary = error + inc_primary * d_secondary;
      const int err_inc_both = err_inc_primary - inc_secondary * d_primary;
      primary += inc_primary;
      if (abs(err_inc_primary) < abs(err_inc_both)) {
        error = err_inc_primary;
      } else {
        secondary += inc_secondary;
        error = err_inc_both;
      }
    }
  }
  *range = status == SG_HIT ? rg : 0.0;
  return status;
}

// The closed form of the walk away from ties (derived at k_mu_emit, map_update_kernels.h): with A = e_x_inc,
// B = e_y_inc the number of y steps among the first k steps of a piece that starts with error term e0 is
// floor((q0 + k |A|) / (|A| + |B|)), q0 = sign(A) e0 - (|B| - |A|) / 2 + |B|.
struct SgWalkLine {
  double q0, absA, absB, inv_W, e0, A, B;
  int inc_x, inc_y;
};
SLAMHIP_SG_FN SgWalkLine sg_walk_line(const SgBeam &b) {
  SgWalkLine L;
  const double scale = b.scale;
  L.inc_x = 0 < b.d_x ? 1 : -1;
  L.inc_y = 0 < b.d_y ? 1 : -1;
  const double mid_x = (b.bx + 0.5) * scale, mid_y = (b.by + 0.5) * scale;
  const double mid_cell_seg_y = b.d_x * b.ry + (mid_x - b.rx) * b.d_y;
  L.e0 = mid_cell_seg_y - mid_y * b.d_x;
  L.A = L.inc_x * scale * b.d_y;
  L.B = -L.inc_y * scale * b.d_x;
  L.absA = fabs(L.A);
  L.absB = fabs(L.B);
  const double W = L.absA + L.absB;
  const double sgn = L.A < 0 ? -1.0 : 1.0;
  const double theta = (L.absB - L.absA) * 0.5;
  L.q0 = sgn * L.e0 - theta + L.absB;
  L.inv_W = 1.0 / W;
  return L;
}
SLAMHIP_SG_FN int sg_walk_j(double q0, double absA, double inv_W, unsigned k) {
  const double fj = floor((q0 + (double)k * absA) * inv_W);
  return (int)fmin(fmax(fj, 0.0), (double)k);
}

// ---- the wave form's arithmetic, one lane at a time (csrc/scan_generate.hip runs it on 64 lanes; tests/native/
// scan_generate_test.cpp runs the same functions lane after lane on the host) -----------------------------------------
// The piece of the walk being evaluated: first walk index, cell (in steps from the robot's) and error term there, the
// formula's offset.
struct SgPiece {
  unsigned k_base;
  int ci, cj;
  double e_base, q0s;
};
// The closed form is trusted only while the rounding of the rebuilt error term e_base + i A + j B -- and of the
// recurrence it stands for -- stays far below the 1e-9 margin kept around the tie tolerance: each is a few ulps of
// cap (|A| + |B|), so cap (|A| + |B|) <= 1e5 bounds it by about 8 * 2^-53 * 1e5 < 1e-10.  Longer beams go to the
// sequential routine.  (The evaluator's to_lsp(100, 270, 1000) at 0.1 m: 1416 cells x 14 = 2e4.)
SLAMHIP_SG_FN bool sg_wave_applies(const SgWalkLine &L, unsigned cap) {
  return L.absA + L.absB > 0.0 && (L.absA + L.absB) * (double)cap <= 1e5;
}
// walk index k: the cell (*i, *j) and its class -- 0 a plain step the formula reproduces, 1 the end cell, 2 a tie,
// 3 not classifiable, 4 beyond cells_nm
SLAMHIP_SG_FN int sg_wave_classify(const SgWalkLine &L, const SgPiece &pc, unsigned k, unsigned cap, int steps_x, int steps_y,
                                   int *i, int *j) {
  const unsigned mm = k - pc.k_base;
  const int jm = sg_walk_j(pc.q0s, L.absA, L.inv_W, mm), jn = sg_walk_j(pc.q0s, L.absA, L.inv_W, mm + 1u);
  const int im = (int)mm - jm;
  *i = pc.ci + im;
  *j = pc.cj + jm;
  const double e = pc.e_base + (double)im * L.A + (double)jm * L.B;
  const double d = fabs(e + L.B) - fabs(e + L.A), ad = fabs(d);
  if (k >= cap) return 4;
  if (*i == steps_x && *j == steps_y) return 1;
  if (*i > steps_x || *j > steps_y) return 3;
  if (ad < 1e-7 - 1e-9) return 2;
  if (ad > 1e-7 + 1e-9 && (0 < d) == (jn == jm) && jn - jm <= 1) return 0;
  return 3;
}
// the piece behind a tie decided on cell (ti, tj) at walk index k: the diagonal step, or the one open axis
SLAMHIP_SG_FN SgPiece sg_wave_after_tie(const SgWalkLine &L, int ti, int tj, unsigned k, int steps_x, int steps_y) {
  const bool at_x = ti == steps_x, at_y = tj == steps_y;
  SgPiece pc;
  pc.ci = ti + (at_x ? 0 : 1);
  pc.cj = tj + ((at_x || !at_y) ? 1 : 0);
  pc.k_base = k + 1u;
  pc.e_base = 0.0;
  pc.q0s = (0.0 - (L.absB - L.absA) * 0.5) + L.absB;
  return pc;
}
constexpr int kSgMaxTies = 8;

// LaserScanGenerator's opening assertion (laser_scan_generator.h:42-44): true = the pose is supported
SLAMHIP_SG_FN bool sg_pose_ok(double x, double y, double scale) {
  const int cx = (int)floor(x / scale), cy = (int)floor(y / scale);
  return !ae::ae_equal(x, cx * scale) && !ae::ae_equal(y, cy * scale);
}

// The whole call on the host: n_poses x n_angles beams over a host payload.
template <bool FMA, class Map>
static inline void sg_generate_host(const Map &m, int n_poses, const double *poses_xyt, int n_angles, const double *angles,
                                    double max_dist, double thr, double *range_out, unsigned char *status_out) {
  for (int p = 0; p < n_poses; ++p)
    for (int i = 0; i < n_angles; ++i) {
      const SgBeam b = sg_beam_setup<FMA>(poses_xyt[3 * p], poses_xyt[3 * p + 1], poses_xyt[3 * p + 2], angles[i], max_dist,
                                          m.scale);
      double rg = 0.0;
      status_out[(size_t)p * n_angles + i] = (unsigned char)sg_beam_sequential(m, b, thr, &rg);
      range_out[(size_t)p * n_angles + i] = rg;
    }
}

// The limits every entry point holds its arguments to, so that cell coordinates fit an int with room to spare and a
// walk is at most a few million cells long.  Returns a message, or null when the arguments are fine.
static inline const char *sg_check_beams(double scale, int n_poses, const double *poses_xyt, int n_angles, const double *angles,
                                         double max_dist) {
  if (!(scale > 0.0) || !(scale - scale == 0.0)) return "bad map scale";
  if (!(max_dist - max_dist == 0.0) || !(fabs(max_dist) / scale <= 1048576.0)) return "max_dist is not finite, or longer than 2^20 cells";
  for (int i = 0; i < n_angles; ++i)
    if (!(fabs(angles[i]) <= 1e6)) return "a beam angle is not finite or beyond 1e6 rad";
  for (int p = 0; p < n_poses; ++p) {
    const double *q = poses_xyt + 3 * p;
    if (!(fabs(q[0]) / scale <= 536870912.0) || !(fabs(q[1]) / scale <= 536870912.0) || !(fabs(q[2]) <= 1e6))
      return "a pose is not finite, or farther than 2^29 cells from the origin";
    if (!sg_pose_ok(q[0], q[1], scale)) return "LS Gen: robot at cell boundary is not supported";
  }
  return nullptr;
}

// the angle list of laser_scan_generator.h:47-48: accumulated, with the 2 pi break
static inline long long sg_angles(double half_sector, double angle_inc, long long cap, double *out) {
  long long n = 0;
  for (double a = -half_sector; a <= half_sector; a += angle_inc) {
    if (2 * M_PI <= half_sector + a) break;
    if (n < cap) out[n] = a;
    ++n;
  }
  return n;
}

}  // namespace sg
}  // namespace slamhip
