// score_device.h -- device functions shared by the scoring kernels (score_kernels.hip) and the
// device-resident hill-climbing chain (hc_chain.hip): one definition, so a pose scored by either
// kernel gets the same bits.
//   RegularSquaresGrid::world_to_cell      src/core/maps/regular_squares_grid.h:40-46
//   ObstacleBasedOccupancyObservationPE    src/core/scan_matchers/occupancy_observation_probability.h:12-27
//   DiscrepancyOIE / OccupancyOIE          src/core/scan_matchers/observation_impact_estimators.h:14-28
//   GridCell::discrepancy                  src/core/maps/grid_cell.h:33-35
//   TbmBaseCell::discrepancy + conjunctive src/core/maps/tbm_grid_cells.h:21-35,
//                                          src/core/maps/transferable_belief_model.h:102-143
//   CredibilistCell::discrepancy + disjunctive src/slams/credibilist/grid_cell.h:31-40,
//                                          src/core/maps/transferable_belief_model.h:145-162
#pragma once

#include "slamhip_internal.h"

namespace slamhip {

// ---- helpers ---------------------------------------------------------------------------------
// value of lane (lane ^ OFF) without a trip through the LDS crossbar: DPP row operations inside a row of 16 lanes,
// gfx950's permlane swaps between rows / halves (tools/scratch/dpp_probe.hip prints what each of them reads).
// ds_bpermute (what __shfl_xor compiles to) costs an address computation and ~100 cycles per 32-bit half and step;
// six dependent steps of it were a third of a microsecond at the end of every pose of the matcher chains.
template <int OFF>
__device__ __forceinline__ unsigned lane_xor_u32(unsigned v) {
  static_assert(OFF == 1 || OFF == 2 || OFF == 4 || OFF == 8 || OFF == 16 || OFF == 32, "butterfly offsets only");
  if (OFF == 1) return (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, 0xB1, 0xF, 0xF, false);  // quad_perm [1,0,3,2]
  if (OFF == 2) return (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x4E, 0xF, 0xF, false);  // quad_perm [2,3,0,1]
  if (OFF == 4) {  // row_ror:12 into banks 0 and 2 (lanes with bit 2 clear), row_ror:4 into banks 1 and 3
    const int a = __builtin_amdgcn_update_dpp((int)v, (int)v, 0x12C, 0xF, 0x5, false);
    return (unsigned)__builtin_amdgcn_update_dpp(a, (int)v, 0x124, 0xF, 0xA, false);
  }
  if (OFF == 8) return (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x128, 0xF, 0xF, false);  // row_ror:8
  const int lane = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
  if (OFF == 16) {
    const auto r = __builtin_amdgcn_permlane16_swap(v, v, false, false);  // [0]: odd rows <- even rows, [1]: even <- odd
    return (lane & 16) ? r[0] : r[1];
  }
  const auto r = __builtin_amdgcn_permlane32_swap(v, v, false, false);  // [0]: upper half <- lower, [1]: lower <- upper
  return (lane & 32) ? r[0] : r[1];
}
template <int OFF>
__device__ __forceinline__ double lane_xor_f64(double v) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  const unsigned lo = lane_xor_u32<OFF>((unsigned)b), hi = lane_xor_u32<OFF>((unsigned)(b >> 32));
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

__device__ __forceinline__ double wave_xor_sum(double v) {
  // fixed butterfly: every lane ends with the same bits (a+b == b+a in IEEE)
  v = v + lane_xor_f64<32>(v);
  v = v + lane_xor_f64<16>(v);
  v = v + lane_xor_f64<8>(v);
  v = v + lane_xor_f64<4>(v);
  v = v + lane_xor_f64<2>(v);
  v = v + lane_xor_f64<1>(v);
  return v;
}

// ---- term-vector fingerprints (the matchers' checked default mode) -------------------------------
// h = sum over beams of lo32(term) * k_lo(b) + hi32(term) * k_hi(b) mod 2^64 with odd per-beam multipliers
// k(b) = (2b + 1) * C mod 2^32: integer arithmetic, so every order of adding it up gives the same value; one
// differing term changes it for certain, terms exchanged between beams change it unless the multipliers conspire.
__device__ __forceinline__ unsigned long long term_fingerprint(double term, unsigned k_lo, unsigned k_hi) {
  const unsigned long long bits = (unsigned long long)__double_as_longlong(term);
  return (unsigned long long)(unsigned)bits * k_lo + (unsigned long long)(unsigned)(bits >> 32) * k_hi;
}
// (r01-r03 folded h to 32 bits; the chains and K1 now carry all 64 -- VERDICT r3 item 7 -- and the co-resident chain,
// whose granule has room for 48 next to the score and the tag, folds the top 16 into them)
__device__ __forceinline__ unsigned long long fold_fingerprint48(unsigned long long h) {
  return (h ^ (h >> 48)) & 0xffffffffffffull;
}
// wave_xor_sum's fixed butterfly with the fingerprint's exchanges riding along
template <int OFF>
__device__ __forceinline__ void wave_xor_step_with(double &v, unsigned long long &h) {
  const double o = lane_xor_f64<OFF>(v);
  const unsigned ol = lane_xor_u32<OFF>((unsigned)h), oh = lane_xor_u32<OFF>((unsigned)(h >> 32));
  v = v + o;
  h += ((unsigned long long)oh << 32) | ol;
}
__device__ __forceinline__ void wave_xor_sum_with(double &v, unsigned long long &h) {
  wave_xor_step_with<32>(v, h);
  wave_xor_step_with<16>(v, h);
  wave_xor_step_with<8>(v, h);
  wave_xor_step_with<4>(v, h);
  wave_xor_step_with<2>(v, h);
  wave_xor_step_with<1>(v, h);
}

// world_to_cell: int(floor(x / scale)) with a TRUE division (Q15: multiplying by 1/scale flips
// cells at boundaries).  The division is the most expensive thing in the per-beam body, so it is
// only executed when it can matter: with t = v/scale, RN(t) is within 2^-53 |t| of t and
// q = RN(v * RN(1/scale)) within 2^-52 |t|, hence no integer separates q from RN(t) unless q lies
// within 1.5 * 2^-52 |q| of one.  Outside a 2^-49 |q| band around integers floor(q) IS the
// reference's cell; inside it (endpoints exactly on cell boundaries do occur, e.g. the reference's
// HC smoke fixture) the true quotient is evaluated.  The absolute term sends underflowing products
// to the exact path as well.
__device__ __forceinline__ int to_cell(double v, double scale, double inv_scale) {
  const double q = v * inv_scale;
  const double f = floor(q);
  const double d = q - f;
  const double tol = fabs(q) * 0x1p-49 + 0x1p-1000;
  if (__builtin_expect(d < tol || (1.0 - d) < tol, 0)) return (int)floor(v / scale);
  return (int)f;
}

// payload of cell (cx, cy) -- or of the prototype cell outside the window (UnboundedPlainGridMap::operator[],
// plain_grid_map.h:69-73); OCC uses .x only.  Split from the probability so that a thread can have the
// gathers of several beams in flight before it needs the first value.
template <int MODEL>
__device__ __forceinline__ double4 load_cell(const MapView &m, int cx, int cy) {
  const int ix = cx + m.origin_x, iy = cy + m.origin_y;
  const bool inb = (unsigned)ix < (unsigned)m.width && (unsigned)iy < (unsigned)m.height;
  double4 v = make_double4(m.unknown[0], m.unknown[1], m.unknown[2], m.unknown[3]);
  if (MODEL == SLAMHIP_CELL_OCC) {
    if (inb) v.x = m.payload[(size_t)iy * m.pitch + ix];
  } else {
    if (inb) v = *(reinterpret_cast<const double4 *>(m.payload) + ((size_t)iy * m.pitch + ix));
  }
  return v;
}

template <int MODEL>
__device__ __forceinline__ double cell_probability(int oie, const double4 &v) {
  if (MODEL == SLAMHIP_CELL_OCC) {
    const double occ = v.x;
    if (oie == SLAMHIP_OIE_OCCUPANCY) return occ;
    return 1.0 - fabs(occ - 1.0);
  } else if (MODEL == SLAMHIP_CELL_CREDIBILIST) {
    return credibilist_probability(v.x, v.y, v.z, v.w);
  } else {
    return tbm_discrepancy_probability(v.x, v.y, v.z, v.w);
  }
}

template <int MODEL>
__device__ __forceinline__ double point_probability(const MapView &m, int oie, int cx, int cy) {
  return cell_probability<MODEL>(oie, load_cell<MODEL>(m, cx, cy));
}

// one beam of WeightedMeanPointProbabilitySPE::estimate_scan_probability
// (weighted_mean_point_probability_spe.h:108-124): scan point moved to the pose with the cached-provider
// angle addition (sensor_data.h:83-88, trigonometry_utils.h:45-55), its cell, the cell's probability,
// times weight times factor
template <int MODEL>
__device__ __forceinline__ double4 beam_cell(const MapView &m, double x, double y, double sn, double cs, double r,
                                             double ca, double sa) {
  const double c = cs * ca - sn * sa;
  const double s = sn * ca + cs * sa;
  const double wx = x + r * c;
  const double wy = y + r * s;
  return load_cell<MODEL>(m, to_cell(wx, m.scale, m.inv_scale), to_cell(wy, m.scale, m.inv_scale));
}
// ---- K2: window OOPEs (max / mean / overlap) ------------------------------------------------------
// MaxOccupancyObservationPE / MeanOccupancyObservationPE / OverlapWeightedOccupancyObservationPE
// (src/core/scan_matchers/occupancy_observation_probability.h:29-99) over GridRasterizedRectangle
// (src/core/maps/grid_rasterization.h:26-64: x outer, y inner) and LightWeightRectangle::overlap /
// intersect_internal (src/core/geometry_primitives.h:205-310) with the reference's fuzzy
// comparisons (src/core/math_utils.h:15-25,37-51).  Sums run in the reference's cell order, so
// per-beam values are bit-identical to the CPU path.
struct Lwr {
  double bot, top, left, right;
};
__device__ __forceinline__ bool fz_equal(double a, double b) {
  const double m = fmax(fabs(a), fabs(b));
  return fabs(a - b) <= 1e-7 * fmax(1.0, m);
}
__device__ __forceinline__ bool fz_less(double a, double b) { return a < b + 2.220446049250313e-16; }
__device__ __forceinline__ bool fz_le(double a, double b) { return fz_equal(a, b) || fz_less(a, b); }
__device__ __forceinline__ bool fz_ordered(double a, double b, double c) { return fz_le(a, b) && fz_le(b, c); }
__device__ __forceinline__ double lwr_area(const Lwr &r) { return (r.top - r.bot) * (r.right - r.left); }
__device__ __forceinline__ bool lwr_contains(const Lwr &r, double x, double y) {
  return fz_ordered(r.left, x, r.right) && fz_ordered(r.bot, y, r.top);
}
__device__ inline Lwr lwr_intersect(const Lwr &self, const Lwr &that, bool reversed) {
  unsigned nm = 0;
  double cl = self.left, cr = self.right, ct = self.top, cb = self.bot;
  if (lwr_contains(self, that.left, that.bot)) { ++nm; cl = that.left; cb = that.bot; }
  if (lwr_contains(self, that.right, that.bot)) { ++nm; cr = that.right; cb = that.bot; }
  if (lwr_contains(self, that.left, that.top)) { ++nm; cl = that.left; ct = that.top; }
  if (lwr_contains(self, that.right, that.top)) { ++nm; cr = that.right; ct = that.top; }
  if (nm == 0) {
    if (reversed) return Lwr{0, 0, 0, 0};
    return lwr_intersect(that, self, true);
  }
  return Lwr{cb, ct, cl, cr};
}
__device__ inline double lwr_overlap(const Lwr &self, const Lwr &that) {
  if (lwr_area(self) != 0) return lwr_area(lwr_intersect(self, that, false)) / lwr_area(self);
  if (lwr_area(that) != 0) return lwr_contains(that, self.left, self.bot) ? 1.0 : 0.0;
  return (fz_equal(self.top, that.top) && fz_equal(self.bot, that.bot) && fz_equal(self.left, that.left) &&
          fz_equal(self.right, that.right)) ? 1.0 : 0.0;
}

// per-beam value of the window OOPEs at the beam's end point (ox, oy); half_v / half_h: half the analysis area's
// extent (sp_analysis_area, grid_scan_matcher.h:87-91)
template <int MODEL>
__device__ __forceinline__ double window_probability(const MapView &map, int oie, int oope, double half_v, double half_h,
                                                     double ox, double oy) {
  const double scale = map.scale, inv_scale = map.inv_scale;
  const Lwr area{oy - half_v, oy + half_v, ox - half_h, ox + half_h};
  const double ar = lwr_area(area);
  int lbx, lby, rtx, rty;
  if (ar != 0 && ar != __builtin_inf()) {
    lbx = to_cell(area.left, scale, inv_scale);
    lby = to_cell(area.bot, scale, inv_scale);
    rtx = to_cell(area.right, scale, inv_scale);
    rty = to_cell(area.top, scale, inv_scale);
  } else if (ar == 0) {
    lbx = rtx = to_cell(area.left, scale, inv_scale);
    lby = rty = to_cell(area.bot, scale, inv_scale);
  } else {
    lbx = -map.origin_x;
    lby = -map.origin_y;
    rtx = map.width - 1 - map.origin_x;
    rty = map.height - 1 - map.origin_y;
  }
  double tot_p = 0, tot_w = 0, mx = 0;
  unsigned cnt = 0;
  for (int cx = lbx; cx <= rtx; ++cx)
    for (int cy = lby; cy <= rty; ++cy) {
      const double impact = point_probability<MODEL>(map, oie, cx, cy);
      if (oope == SLAMHIP_OOPE_MAX) {
        mx = impact < mx ? mx : impact;
      } else if (oope == SLAMHIP_OOPE_MEAN) {
        tot_p += impact;
        cnt += 1;
      } else {
        const Lwr cb{scale * cy, scale * (cy + 1), scale * cx, scale * (cx + 1)};
        const double w = lwr_overlap(area, cb);
        tot_p += impact * w;
        tot_w += w;
      }
    }
  if (oope == SLAMHIP_OOPE_MAX) return mx;
  if (oope == SLAMHIP_OOPE_MEAN) return cnt ? tot_p / cnt : 0.5;
  return tot_w != 0 ? tot_p / tot_w : 0.5;
}

template <int MODEL>
__device__ __forceinline__ double beam_term(const MapView &m, int oie, double x, double y, double sn, double cs,
                                            double r, double ca, double sa, double w, double f) {
  const double pr = cell_probability<MODEL>(oie, beam_cell<MODEL>(m, x, y, sn, cs, r, ca, sa));
  return pr * w * f;
}

// ---- K1's scoring body (k_score_point, score_kernels.hip; k_bf_score_batch, bf_batch.hip) -----------------------
// 256 threads per workgroup, thread t owns beams t, t + 256, ...; at most 16 poses per workgroup.
constexpr int kScoreBlock = 256;
constexpr int kScoreMaxPosesPerBlock = 16;

// the beam constants of thread t (KB > 0: n <= 256 KB, they live in VGPRs for every pose of the workgroup)
template <int KB>
__device__ __forceinline__ void score_point_load_beams(const ScanView &scan, int n, int t, double *br, double *bc, double *bs,
                                                       double *bw, double *bf) {
  if (KB > 0) {
#pragma unroll
    for (int k = 0; k < (KB > 0 ? KB : 1); ++k) {
      const int b = t + kScoreBlock * k;
      const bool ok = b < n;
      br[k] = ok ? scan.range[b] : 0.0;
      bc[k] = ok ? scan.cos_a[b] : 0.0;
      bs[k] = ok ? scan.sin_a[b] : 0.0;
      bw[k] = ok ? scan.weight[b] : 0.0;
      bf[k] = ok ? scan.factor[b] : 0.0;
    }
  }
}

// The npb poses staged in s_pose (x, y, sin, cos), scored in the canonical order: thread t adds its beams' terms in
// ascending order, a wave64 xor-butterfly, (g0 + g1) + (g2 + g3) across the four waves, total / tot_w (NaN where tot_w
// is 0); FPRINT: the term vector's fingerprint beside it.  Pose p0 + j goes to scores[p0 + j].  The caller has put a
// barrier behind its stores to s_pose.
template <int MODEL, int KB, bool WRITE_TERMS, bool FPRINT>
__device__ __forceinline__ void score_point_body(const MapView &map, const ScanView &scan, int oie, int n, int p0, int npb,
                                                 const double (*s_pose)[4], double (*s_part)[4], unsigned long long (*s_hpart)[4],
                                                 const double *br, const double *bc, const double *bs, const double *bw,
                                                 const double *bf, double *terms, double *scores, unsigned long long *fprints) {
  constexpr int kBlock = kScoreBlock;
  constexpr int KR = KB > 0 ? KB : 1;
  const int t = threadIdx.x;
  const int lane = t & 63, wave = t >> 6;
  const double scale = map.scale, inv_scale = map.inv_scale;
  // position-sensitive multilinear form of the terms' 32-bit halves, odd per-beam multipliers (hc_chain.hip's)
  const unsigned fk_lo = (2u * (unsigned)t + 1u) * 0x9E3779B1u, fk_hi = (2u * (unsigned)t + 1u) * 0x85EBCA6Bu;
  for (int j = 0; j < npb; ++j) {
    const double x = s_pose[j][0], y = s_pose[j][1], sn = s_pose[j][2], cs = s_pose[j][3];
    double acc = 0.0;
    unsigned long long h = 0ull;
    if (KB > 0) {
#pragma unroll
      for (int k = 0; k < KR; ++k) {
        const int b = t + kBlock * k;
        if (b < n) {
          const double c = cs * bc[k] - sn * bs[k];
          const double s = sn * bc[k] + cs * bs[k];
          const double wx = x + br[k] * c;
          const double wy = y + br[k] * s;
          const double pr = point_probability<MODEL>(map, oie, to_cell(wx, scale, inv_scale), to_cell(wy, scale, inv_scale));
          const double term = pr * bw[k] * bf[k];
          if (WRITE_TERMS) terms[(size_t)(p0 + j) * n + b] = term;
          acc = acc + term;
          if (FPRINT) h += term_fingerprint(term, fk_lo + (unsigned)k * (2u * kBlock * 0x9E3779B1u),
                                            fk_hi + (unsigned)k * (2u * kBlock * 0x85EBCA6Bu));
        }
      }
    } else {
      for (int b = t; b < n; b += kBlock) {
        const double ca = scan.cos_a[b], sa = scan.sin_a[b], r = scan.range[b];
        const double c = cs * ca - sn * sa;
        const double s = sn * ca + cs * sa;
        const double wx = x + r * c;
        const double wy = y + r * s;
        const double pr = point_probability<MODEL>(map, oie, to_cell(wx, scale, inv_scale), to_cell(wy, scale, inv_scale));
        const double term = pr * scan.weight[b] * scan.factor[b];
        if (WRITE_TERMS) terms[(size_t)(p0 + j) * n + b] = term;
        acc = acc + term;
        if (FPRINT) {
          const unsigned kq = (unsigned)(b / kBlock);
          h += term_fingerprint(term, fk_lo + kq * (2u * kBlock * 0x9E3779B1u), fk_hi + kq * (2u * kBlock * 0x85EBCA6Bu));
        }
      }
    }
    if (FPRINT) {
      wave_xor_sum_with(acc, h);
      if (lane == 0) s_hpart[j][wave] = h;
    } else {
      acc = wave_xor_sum(acc);
    }
    if (lane == 0) s_part[j][wave] = acc;
  }
  __syncthreads();
  if (t < npb) {
    const double total = (s_part[t][0] + s_part[t][1]) + (s_part[t][2] + s_part[t][3]);
    scores[p0 + t] = (scan.tot_w == 0.0) ? __builtin_nan("") : total / scan.tot_w;
    if (FPRINT) fprints[p0 + t] = s_hpart[t][0] + s_hpart[t][1] + s_hpart[t][2] + s_hpart[t][3];
  }
}

// ---- K2's scoring body (k_score_window, score_kernels.hip; k_score_window_batch, score_batch.hip) -----------------
// The npb poses staged in s_pose through a window OOPE: thread t walks its beams t, t + 256, ... in ascending order
// (constants re-read per pose: the per-beam window walk dwarfs them), the canonical sum and the fingerprint of
// score_point_body (same multipliers; fprints null: none).  terms (null: none) is pose-major, n per pose; pose p0 + j
// goes to scores[p0 + j].  The caller has put a barrier behind its stores to s_pose.
template <int MODEL>
__device__ __forceinline__ void score_window_body(const MapView &map, const ScanView &scan, int oie, int oope, double half_v,
                                                  double half_h, int n, int p0, int npb, const double (*s_pose)[4],
                                                  double (*s_part)[4], unsigned long long (*s_hpart)[4], double *terms,
                                                  double *scores, unsigned long long *fprints) {
  constexpr int kBlock = kScoreBlock;
  const int t = threadIdx.x;
  const int lane = t & 63, wave = t >> 6;
  // (the checked default mode over the window OOPEs, r05: K1's term-vector fingerprint, same multipliers)
  const bool fprint = fprints != nullptr;
  const unsigned fk_lo = (2u * (unsigned)t + 1u) * 0x9E3779B1u, fk_hi = (2u * (unsigned)t + 1u) * 0x85EBCA6Bu;
  for (int j = 0; j < npb; ++j) {
    const double x = s_pose[j][0], y = s_pose[j][1], sn = s_pose[j][2], cs = s_pose[j][3];
    double acc = 0.0;
    unsigned long long h = 0ull;
    for (int b = t; b < n; b += kBlock) {
      const double ca = scan.cos_a[b], sa = scan.sin_a[b], r = scan.range[b];
      const double c = cs * ca - sn * sa;
      const double s = sn * ca + cs * sa;
      const double ox = x + r * c, oy = y + r * s;
      const double pr = window_probability<MODEL>(map, oie, oope, half_v, half_h, ox, oy);
      const double term = pr * scan.weight[b] * scan.factor[b];
      if (terms) terms[(size_t)(p0 + j) * n + b] = term;
      acc = acc + term;
      if (fprint) {
        const unsigned kq = (unsigned)(b / kBlock);
        h += term_fingerprint(term, fk_lo + kq * (2u * kBlock * 0x9E3779B1u), fk_hi + kq * (2u * kBlock * 0x85EBCA6Bu));
      }
    }
    wave_xor_sum_with(acc, h);  // (the butterfly of wave_xor_sum with the fingerprint riding along: same sum bits)
    if (lane == 0) {
      s_part[j][wave] = acc;
      s_hpart[j][wave] = h;
    }
  }
  __syncthreads();
  if (t < npb) {
    const double total = (s_part[t][0] + s_part[t][1]) + (s_part[t][2] + s_part[t][3]);
    scores[p0 + t] = (scan.tot_w == 0.0) ? __builtin_nan("") : total / scan.tot_w;
    if (fprint) fprints[p0 + t] = s_hpart[t][0] + s_hpart[t][1] + s_hpart[t][2] + s_hpart[t][3];
  }
}

}  // namespace slamhip
