// Internal declarations shared by the HIP kernels (score_kernels.hip) and the host side
// of the C-ABI (slamhip_api.cpp, matchers.cpp).  Not installed; the public ABI is include/slamhip.h.
#pragma once

// Testing and debugging hooks (in-kernel wall-clock stamps, a workgroup that leaves at once, injected failures, a stalled
// stream, a pretend-small trace buffer) exist only in libslamhip_testing.so, which csrc/Makefile builds from the same
// sources with -DSLAMHIP_TESTING and which the tests that need a hook load; the shipped libslamhip.so exports none of
// them and its kernels carry no branch for them.
#ifdef SLAMHIP_TESTING
#define SLAMHIP_STAMPS_ON(expr) (expr)
#else
#define SLAMHIP_STAMPS_ON(expr) false
#endif


#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "gm_carry.h"
#include "scan_filter.h"
#include "slamhip.h"

namespace slamhip {

// ---- views passed to kernels by value -----------------------------------------------------
// Map window in HBM: row-major [height][pitch] cells, each cell CELL_DOUBLES(model) doubles
// (OCC 1, TBM 4, GMAPPING 4 = prob_occ, obst.x, obst.y, pad -> 32-byte aligned gathers).
// The pad of a GMAPPING cell of a DENSE window holds, in its low dword, the cell's NEIGHBOURHOOD MASK once a GMapping
// scorer has asked for it (nbr_ok): bit 3 (dx + 1) + (dy + 1) = "the cell at (+dx, +dy) is inside the window and full",
// full = !(prob_occ < fullness_th) -- the scorer's own test.  One 4-byte load then tells a beam which of the nine
// cells of its 3 x 3 window it has to look at (gm_score_device.h); writers keep the masks (mu_cell_store flips the
// nine neighbours' bits when a cell changes sides; uploads re-derive them) or drop them (DeviceMap::nbr_ok).
struct MapView {
  const double *payload;
  int width, height, pitch;
  int origin_x, origin_y;
  double scale, inv_scale;  // inv_scale = RN(1 / scale), see to_cell()
  double unknown[4];
  int nbr_ok;  // the neighbourhood masks of this (dense, GMAPPING) window are valid for the scorer's threshold
  int reserved_;
};

// TbmBaseCell::discrepancy of the scorer's fixed observation, 1 - it: the per-beam probability of a TBM cell under the
// discrepancy OIE (tbm_grid_cells.h:21-35, transferable_belief_model.h:102-143; SURVEY Q18: the observation is always
// (u, e, o, c) = (0, 0, 1, 0), so the value is a PURE FUNCTION OF THE CELL).  One definition for the scoring kernels
// (cell_probability<TBM>), the probability plane's writers and the host (the prototype cell's value): the same
// operations in the same order, hence the same bits wherever it is evaluated (-ffp-contract=off).
__host__ __device__ inline double tbm_discrepancy_probability(double U, double E, double O, double Cc) {
  // that = aoo2tbm(obstacle AOO) = (u,e,o,c) = (0,0,1,0); conjunctive(that, cell) before
  // normalisation = (0, 0, U+O, E+C); normalize() divides by the total mass.
  const double d_occ = __builtin_fabs(1.0 - O);
  const double t2 = U + O, t3 = E + Cc;
  const double tot = t2 + t3;
  const double conflict = (tot == 0.0) ? 0.0 : t3 / tot;
  const double unknown = U / 2.0;
  const double known = 1 - unknown;
  const double known_discrepancy = known * (conflict + d_occ) / 2.0;
  return 1.0 - (unknown / 2 + known_discrepancy);
}

// CredibilistCell::discrepancy of the same observation, 1 - it (slams/credibilist/grid_cell.h:31-40): the per-beam
// probability of a CREDIBILIST cell.  disjunctive((0,0,1,0), cell) before normalisation = (U+E, 0, O+C, 0)
// (transferable_belief_model.h:145-162: the products with the observation's zero masses add 0.0), normalize() divides by
// the total mass or resets a massless belief to (1,0,0,0), whose occupied() is 0.  The outer 1 - (1 - s) is the cell's
// `1.0 - score` under DiscrepancyOIE's `1.0 - discrepancy`: not s in floating point.
__host__ __device__ inline double credibilist_probability(double U, double E, double O, double Cc) {
  const double t0 = U + E, t2 = O + Cc;
  const double tot = ((t0 + 0.0) + t2) + 0.0;
  const double s = (tot == 0.0) ? 0.0 : t2 / tot;
  return 1.0 - (1.0 - s);
}
// whether a cell model's payload is a (u, e, o, c) belief; the probability of such a cell under the discrepancy OIE
__host__ __device__ inline bool cell_is_belief(int model) {
  return model == SLAMHIP_CELL_TBM || model == SLAMHIP_CELL_CREDIBILIST;
}
__host__ __device__ inline double belief_probability(int model, double U, double E, double O, double Cc) {
  return model == SLAMHIP_CELL_CREDIBILIST ? credibilist_probability(U, E, O, Cc) : tbm_discrepancy_probability(U, E, O, Cc);
}

// A cell's OCCUPANCY: what the reference's (double)map[c] / map.occupancy(c) -- GridCell::occupancy().prob_occ -- holds
// for the cell whose payload starts (p0, p1, p2).  One definition for the render kernels (map_render.hip) and the host
// (slamhip_render_cells), the reference's operations in its order:
//   OCC          p0
//   GMAPPING     p0 (a never-observed cell holds -1, gmapping_grid_cell.h:14)
//   TBM, kind 0  TbmOccConsistentCell::tbm2occ (tbm_grid_cells.h:89-93): o / (o + e)
//   TBM, kind 1  TbmUnknownEvenOccCell::tbm2occ (:104-106): o + 0.5 * u
//   CREDIBILIST  TBM_to_O (slams/credibilist/TBM_prob_conversion.h:8-10): o + 0.5 * u
// A TBM cell of kind 0 with the never-updated payload (u, e, o) == (1, 0, 0) reports 0.5: the reference's cell keeps
// its prototype's Occupancy{0.5, 1} until the first valid observation (tbm_grid_cells.h:10-19), the rule
// HipResidentMapView::set_cell uses.  The reference's cell holds the SAME payload after being updated only by
// observations of zero quality, and then reports 0 / 0 = NaN: there this value departs from the reference (the payload
// does not tell the two cells apart).  occ_kind is 0 for every model but TBM (the callers check).
__host__ __device__ inline double cell_occupancy(int model, int occ_kind, double p0, double p1, double p2) {
  if (model == SLAMHIP_CELL_TBM && occ_kind == SLAMHIP_OCC_TBM_CONSISTENT) {
    if (p0 == 1.0 && p1 == 0.0 && p2 == 0.0) return 0.5;
    const double qual = p2 + p1;
    return p2 / qual;
  }
  if (cell_is_belief(model)) return p2 + 0.5 * p0;
  return p0;
}
// occ_kind names a TBM cell class: 0 or 1 on a TBM map, 0 on every other
inline bool occ_kind_ok(int model, int occ_kind) {
  if (model == SLAMHIP_CELL_TBM) return occ_kind == SLAMHIP_OCC_TBM_CONSISTENT || occ_kind == SLAMHIP_OCC_TBM_UNKNOWN_EVEN;
  return occ_kind == 0;
}
// OccupancyGridPublisher::on_map_update's cell (src/ros/occupancy_grid_publisher.h:42-44): `int cell_value =
// value == -1 ? -1 : value * 100`, pushed into an int8 vector.  The reference's conversion is undefined for a value
// that is not finite or whose hundredfold leaves the range of int; here a non-finite occupancy writes -1 (unknown) and a
// finite one saturates at the ends of int before it is narrowed, the same on the host and the device.
__host__ __device__ inline signed char render_occgrid(double v) {
  if (v == -1) return (signed char)-1;
  const double t = v * 100;
  if (!(t - t == 0.0)) return (signed char)-1;  // NaN, +-inf
  const int c = t >= 2147483647.0 ? 2147483647 : (t <= -2147483648.0 ? (-2147483647 - 1) : (int)t);
  return (signed char)c;
}
// GridMapToPgmDumber::dump_map's pixel (src/utils/map_dumpers.h:80-82): bound_value is std::max(left, std::min(right,
// v)) (math_utils.h:33-35), i.e. the two compares below -- a NaN occupancy clamps to 1 and paints black, as there.
__host__ __device__ inline unsigned char render_pgm(double v) {
  double b = 0.5;
  if (!(v == -1)) {
    const double m = (v < 1.0) ? v : 1.0;  // std::min(1.0, v)
    b = (0.0 < m) ? m : 0.0;               // std::max(0.0, m)
  }
  const double value = 1.0 - b;
  return (unsigned char)(255 * value);
}
__host__ __device__ inline unsigned char render_byte(int format, double v) {
  return format == SLAMHIP_RENDER_PGM ? render_pgm(v) : (unsigned char)render_occgrid(v);
}

// Filtered scan, structure-of-arrays (coalesced per-beam loads), tot_w = sequential sum of
// weights in beam order computed once on the host (pose independent).
struct ScanView {
  const double *range, *cos_a, *sin_a, *weight, *factor;
  int n;
  double tot_w;
};

struct GmParams {
  double fullness_th;
  int window;
};

// (GmPoseInfo, the per-pose side outputs of the GMapping kernel for the carry-in fix-up: gm_carry.h, included above)

struct ScoreArgs {
  MapView map;
  ScanView scan;
  const double *poses;  // n_poses x 3 (x, y, theta)
  const double *pose_sc;  // optional n_poses x 2 (sin, cos) computed by the host; null = device
  double *scores;
  int n_poses;
  int poses_per_block;
  int oie;
  double area[4];
  GmParams gm;
  GmPoseInfo *gm_info;  // GMAPPING only
  double *terms;        // SEQUENTIAL order only: n_poses x scan.n scratch
  unsigned long long *fprints;  // K1, canonical sum only: per-pose term-vector fingerprints, 64 bits (null = none)
  // per-particle copy-on-write maps (K3 only, tile_pool.h): tile tables of all slots, the slot of
  // every pose; then map.payload = tile pool, map.pitch = tiles per table row, map.width/height =
  // the virtual extent in cells.  null = one dense window for all poses.
  const int *tables;
  const int *pose_slot;
  int table_stride;
  int xcd_blocks;  // set by launch_score: > 0 = the real block count of an XCD-chunked grid
  // fill_args: >= 0 = the model the kernels are instantiated for instead of the map's own -- a TBM map scored through
  // its probability plane looks like an OCC map under the occupancy OIE (DeviceMap::d_prob)
  int model_override;
};

// tiles of the copy-on-write maps: 128 x 128 cells like the reference's LazyTiledGridMap
// (src/core/maps/lazy_tiled_grid_map.h:24-26), row-major inside a tile
constexpr int kTileShift = 7;
constexpr int kTileSide = 1 << kTileShift;
constexpr int kTileMask = kTileSide - 1;
constexpr int kTileCells = kTileSide * kTileSide;
// the settle state of a pool cell (tile_pool.h TilePool::d_state): 1 = its mean is +0; 3 = a free observation leaves +0
// but has to WRITE it -- the never-observed value (a negative unknown[0], bit for bit), or -0; 0 = anything else
constexpr int kTileStateWords = kTileCells / 16;
__host__ __device__ inline unsigned mu_settle_class(double c0, long long unknown_bits, int fresh_ok) {
  long long bits;
  __builtin_memcpy(&bits, &c0, 8);
  return bits == 0ll ? 1u : ((c0 == 0.0 || (fresh_ok && bits == unknown_bits)) ? 3u : 0u);
}

inline int cell_doubles(int model) { return model == SLAMHIP_CELL_OCC ? 1 : 4; }
inline int cell_stride_host(int model) {
  return cell_is_belief(model) ? 4 : (model == SLAMHIP_CELL_GMAPPING ? 3 : 1);
}

// ---- launchers (score_kernels.hip) ---------------------------------------------------------
// ev_start / ev_stop (optional, single-kernel orders only): attached to the scoring dispatch
hipError_t launch_score(const ScoreArgs &a, int cell_model, int oope, int sum_order,
                        hipStream_t stream, hipEvent_t ev_start = nullptr,
                        hipEvent_t ev_stop = nullptr);
hipError_t launch_publish(unsigned *flag, unsigned seq, hipStream_t stream);
// ---- the libm-exact modes (exact_kernels.hip; csrc/libm_exact.h) ----
// cos / sin(theta_p + a_b) with the host glibc's bits for n_poses poses x n beams ([p * stride + b]) + (0, 1) per pose
hipError_t launch_exact_beam_trig(bool fma, const double *poses, int n_poses, const double *d_angle, int n, size_t stride,
                                  double *d_cos, double *d_sin, double *d_identity_sc, hipStream_t stream);
// the GMapping OOPE restated the plain way (exp per full cell, cache beam after beam and pose after pose, beam-order sum)
hipError_t launch_score_gmapping_exact(bool fma, const ScoreArgs &a, const double *d_angle, int raw_trig, void *d_cache,
                                       hipStream_t stream);
hipError_t launch_libm_eval(bool fma, int fn, const double *d_x, double *d_out, int n, hipStream_t stream);
// which build of sin / cos / exp the host's libm runs: 1 = glibc's FMA build, 0 = the plain one, -1 = neither matches
int libm_variant();
hipError_t launch_stall(int ms, hipStream_t stream);  // testing
// n_doubles (rounded up to two) from pinned host memory to HBM by a kernel; *h_flag = seq once the source has been read
// bytes rounded up to 16: both blocks must be that long
hipError_t launch_block_pull(const void *h_src, void *d_dst, size_t bytes, hipStream_t stream);
hipError_t launch_scan_pull(const double *h_src, double *d_dst, size_t n_doubles, unsigned *counter, unsigned *h_flag,
                            unsigned seq, hipStream_t stream);
// k_scan_assemble: one scan block from ScanAssembleArgs (scan_filter.h) and the context's resident per-beam tables.
// *h_flag = seq once the pinned arrays have been read.
hipError_t launch_scan_assemble(const ScanAssembleArgs &a, unsigned *counter, unsigned *h_flag, unsigned seq,
                                hipStream_t stream);
// k_scan_assemble_table: n_jobs scan blocks in one launch, job c from table[c] (a table in pinned memory; grid.y = job,
// max_stride = the widest block's stride).  Entry: ScanAssembleArgs (five rows) or ScanAssembleEachArgs (a sixth row,
// the kept points' angles).
template <class Entry>
hipError_t launch_scan_assemble_table(const Entry *table, int n_jobs, int max_stride, hipStream_t stream);
// (both uploads write the host's stride_host doubles of a cell and leave the rest of it alone -- a GMAPPING cell's pad)
hipError_t launch_scatter_cells(double *payload, int pitch, int cell_dbl, int stride_host, int n,
                                const int *d_coords, const double *d_vals, hipStream_t stream);
hipError_t launch_repack_window(double *dst, int dst_pitch, int cell_dbl, const double *src,
                                int stride_host, int x0, int y0, int w, int h, hipStream_t stream);
hipError_t launch_fill_cells(double *dst, size_t n_cells, int cell_dbl, const double *unknown4,
                             hipStream_t stream);

// ---- host state ------------------------------------------------------------------------------
struct DeviceMap {
  bool bound = false;
  int cell_model = 0;
  int width = 0, height = 0, pitch = 0;
  int origin_x = 0, origin_y = 0;
  double scale = 1.0;
  double unknown[4] = {0, 0, 0, 0};
  double *d_payload = nullptr;
  size_t bytes = 0;
  // update-only cell state, allocated by the first map update (map_update.hip):
  // MeanProbabilityCell::_n (1 double) or GmappingBaseCell::_hits/_tries (2 doubles) per cell
  double *d_aux = nullptr;
  int aux_stride = 0;
  // slamhip_map_set_auto_grow: an update that reaches beyond the window re-binds it first (the reference's
  // unbounded maps grow inside update(), plain_grid_map.h:133-173)
  bool auto_grow = false;
  long grown = 0;  // number of such re-binds
  // neighbourhood masks in the cells' pads (MapView): valid for threshold nbr_th; built by map_nbr_masks()
  bool nbr_ok = false;
  double nbr_th = 0.0;
  double nbr_other_th = 0.0;  // the last threshold a scorer asked for that was NOT the masks' (fill_args)
  // TBM / CREDIBILIST maps: the PROBABILITY PLANE -- one double per cell = belief_probability of the cell (r06, VERDICT r5
  // item 5).  The 1-cell scorers gather 8 bytes from it instead of the 32-byte cell and ~16 flops + a division per
  // (pose, beam); derived by the first scorer call that finds none (map_prob_plane), then kept by every writer: K6's
  // mu_cell_store (MuArgs::prob), uploads and the dirty log re-derive what they wrote; a re-bind drops it.
  double *d_prob = nullptr;
  bool prob_ok = false;
};
// the views the kernels take, every byte of them defined: a bound map's own window (no masks: nbr_ok = 0, the caller
// that has derived them says so), and a scan block of five rows of `stride` doubles at `d`
inline MapView view_of(const DeviceMap &m) {
  MapView v;
  std::memset(&v, 0, sizeof(v));
  v.payload = m.d_payload;
  v.width = m.width;
  v.height = m.height;
  v.pitch = m.pitch;
  v.origin_x = m.origin_x;
  v.origin_y = m.origin_y;
  v.scale = m.scale;
  v.inv_scale = 1.0 / m.scale;
  for (int k = 0; k < 4; ++k) v.unknown[k] = m.unknown[k];
  return v;
}
inline ScanView scan_view_of(const double *d, size_t stride, int n, double tot_w) {
  ScanView v;
  std::memset(&v, 0, sizeof(v));
  v.range = d;
  v.cos_a = d + stride;
  v.sin_a = d + 2 * stride;
  v.weight = d + 3 * stride;
  v.factor = d + 4 * stride;
  v.n = n;
  v.tot_w = tot_w;
  return v;
}
// (re)derives the plane over [x0, x0 + w) x [y0, y0 + h) (clipped) / over n listed cells (d_coords: x, y pairs);
// model: SLAMHIP_CELL_TBM / _CREDIBILIST = which of the two functions the map's plane holds (anything else is an error)
hipError_t launch_prob_build(int model, const double *payload, double *prob, int width, int height, int pitch, int x0, int y0, int w, int h,
                             hipStream_t stream);
hipError_t launch_prob_cells(int model, const double *payload, double *prob, int width, int height, int pitch, int n, const int *d_coords,
                             hipStream_t stream);
// cells whose stored value differs from the derived one (testing), added to *d_count
hipError_t launch_prob_check(int model, const double *payload, const double *prob, int width, int height, int pitch,
                             unsigned long long *d_count, hipStream_t stream);
// (re)derives the masks of the cells of [x0, x0 + w) x [y0, y0 + h) (clipped to the window) from the occupancies
hipError_t launch_nbr_build(double *payload, int width, int height, int pitch, double th, int x0, int y0, int w, int h,
                            hipStream_t stream);
// ... and of the 3 x 3 neighbourhoods of n listed cells (d_coords: x, y pairs)
hipError_t launch_nbr_cells(double *payload, int width, int height, int pitch, double th, int n, const int *d_coords,
                            hipStream_t stream);
// cells whose stored mask differs from the one their neighbours' occupancies give (testing), added to *d_count
hipError_t launch_nbr_check(const double *payload, int width, int height, int pitch, double th, unsigned long long *d_count,
                            hipStream_t stream);

void mu_allow_scan_reuse(slamhip_ctx *ctx, bool on);  // map_update.hip
bool mu_set_deferred(slamhip_ctx *ctx, bool on);      // map_update.hip: queue plain updates without waiting (returns the old setting)
int mu_drain(slamhip_ctx *ctx, long long *n_updates, int *err);
void mu_release(slamhip_ctx *ctx);                    // map_update.hip: frees the context's K6 scratch
void shard_release(slamhip_ctx *ctx);                 // shard.cpp: leaves the RCCL group, frees its staging
void pyramids_release(slamhip_ctx *ctx);              // map_pyramid.hip: frees what the context's pyramids hold in HBM
void score_batch_release(slamhip_ctx *ctx);           // slamhip_api.cpp: frees slamhip_score_poses_batch's staging
void set_error(const std::string &msg);
int hip_fail(hipError_t e, const char *what);
hipError_t refuse_launch(const char *why);  // hipErrorInvalidValue; hip_fail appends `why` to the failed call's text

}  // namespace slamhip

#define SLAMHIP_CHECK(expr)                                        \
  do {                                                             \
    hipError_t _e = (expr);                                        \
    if (_e != hipSuccess) return slamhip::hip_fail(_e, #expr);     \
  } while (0)

#include "hip_block.h"
#include "scan_tables_device.h"

struct slamhip_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  std::vector<slamhip::DeviceMap> maps;
  // scan
  slamhip::DeviceBuf<double> d_scan;  // 5 arrays of scan_cap doubles
  // slamhip_scan_upload: the five arrays packed in pinned memory (two buffers taking turns, an event each) and
  // sent with ONE asynchronous copy -- no wait for the stream, which may still be busy with a queued map update
  slamhip::PinnedBuf<double> h_scan_stage[2];
  hipEvent_t scan_stage_done[2] = {nullptr, nullptr};  // (recorded for the second launch lane only)
  int scan_stage_turn = 0;
  // ... pulled into HBM by a kernel (k_scan_pull): the sequence number of the pull that last read each buffer, what
  // the kernel reported back (pinned), its arrival counter
  unsigned scan_pull_seq[2] = {0, 0}, scan_pull_next = 0;
  slamhip::PinnedBuf<unsigned> h_scan_pulled;
  slamhip::DeviceBuf<unsigned> d_scan_pull_count;
  int scan_cap = 0, scan_n = 0;
  double scan_tot_w = 0.0;
  // the scan the kernels read: d_scan after slamhip_scan_upload, a stored scan after slamhip_scan_select
  const double *scan_ptr = nullptr;
  size_t scan_stride = 0;
  struct ScanSlot {  // slamhip_scan_store: a filtered scan kept resident in HBM (five arrays of `cap` doubles)
    slamhip::DeviceBuf<double> d;
    int cap = 0, n = 0;
    double tot_w = 0.0;
    std::vector<double> w, f;
    // slamhip_scan_store_angles: the points' angles (SLAMHIP_POSE_TRIG_RAW_EXACT), on the host and in HBM; empty after
    // a slamhip_scan_store into the slot
    std::vector<double> angle;
    slamhip::DeviceBuf<double> d_angle;
    int angle_cap = 0;
  };
  std::vector<ScanSlot> scan_slots;
  // slamhip_scan_filter_upload: what depends on the scanner's beam ANGLES only (cos / sin per raw beam as the scan's
  // trig provider tabulates them, the viny weighting's angular factor) is kept between scans -- a scanner's angles do
  // not change -- next to the buffers the filtered scan is assembled in
  struct ScanPrep : slamhip::ScanTables {  // (angle, cos_a, sin_a, viny_f and the scanner's settings: scan_filter.h)
    std::vector<double> r, a, c, s, w, f;
    std::vector<int> kept;       // raw indices of the CURRENT scan's points (of the last call that uploaded one)
    std::vector<int> kept_next;  // ... of the call under way: becomes `kept` once its scan is the current one
    slamhip::ScanFilterScratch filter;  // scan_filter.cpp: one byte per raw point and the per-beam cosines | sines of
                                        // SLAMHIP_TRIG_RAW on a bounded map
    slamhip::ScanStageScratch stage;    // ... the filtered scan's angles / ranges / weights where the weighting asks
  } scan_prep;
  // ... and the same three per-beam arrays resident in HBM (cos | sin | viny_f), where k_scan_assemble gathers them:
  // uploaded when scan_prep recomputes, never by a context that is not given raw scans
  slamhip::ScanTablesDevice scan_tab;
  long long scan_tab_uploads = 0;
  std::vector<double> h_weight, h_factor;  // host copies for GMapping carry-in fix-ups
  // The raw scan between its two halves (slamhip::scan_filter_stage / scan_assemble_now).  `active`: the current scan
  // is staged in pinned memory and recorded as the current one, but the scan block in HBM has not been written yet --
  // whoever reads the block launches nothing before scan_assemble_now; a lone co-resident hill-climbing chain takes
  // `as` into its own launch instead (HcChainArgs::raw) and ends the turn with scan_fused_done.  `record_due`: the host
  // copies of weights / factors are still to be made (scan_record_finish: behind the launch, while the GPU runs).
  struct ScanPending {
    bool active = false, record_due = false;
    slamhip::ScanAssembleArgs as{};
    int turn = 0, weighting = 0;
    unsigned seq = 0;
  } scan_pending;
  // the libm-exact modes (exact_kernels.hip): the beam ANGLES of the current scan (slamhip_scan_set_angles, or the kept
  // angles of slamhip_scan_filter_upload) -- on the host until an exact scoring call needs them in HBM --, the
  // per-pose trig tables, the reference's one GMapping cache object on the device
  std::vector<double> h_scan_angle;
  // after slamhip_scan_filter_upload they are scan_prep.angle[scan_prep.kept[q]] and are written out only when somebody
  // asks (slamhip::scan_angles_materialise): the default scoring modes never do
  bool scan_angle_lazy = false;
  slamhip::DeviceBuf<double> d_scan_angle;
  int scan_angle_cap = 0;
  bool scan_angle_on_device = false;
  slamhip::DeviceBuf<double> d_exact_trig;
  size_t exact_trig_cap = 0;
  slamhip::DeviceBuf<unsigned char> d_gm_exact_cache;
  bool gm_exact_last = false;  // the last scoring call applied the GMapping cache itself: no host fix-up after it
  // pose / score staging
  slamhip::DeviceBuf<double> d_poses, d_scores, d_pose_sc;
  slamhip::PinnedBuf<double> h_poses, h_scores, h_pose_sc;
  slamhip::DeviceBuf<slamhip::GmPoseInfo> d_gm_info;
  slamhip::PinnedBuf<slamhip::GmPoseInfo> h_gm_info;
  slamhip::PinnedBuf<unsigned long long> h_fprints;  // next to h_scores
  bool want_fprints = false;      // the next score_staged() asks K1 for fingerprints (matchers' checked mode)
  slamhip::PinnedBuf<int> h_pose_slot;  // map slot of every staged pose (per-particle maps only)
  int pose_cap = 0;
  slamhip::DeviceBuf<double> d_terms;
  size_t terms_cap = 0;
  void *score_batch = nullptr;  // ScoreBatchStage: slamhip_score_poses_batch's arena, results and last stats (slamhip_api.cpp)
  // dirty-cell staging
  slamhip::DeviceBuf<int> d_dirty_xy;
  slamhip::DeviceBuf<double> d_dirty_val;
  int dirty_cap = 0;
  // GMapping OOPE cache (gmapping_occupancy_observation_pe.h:43-44)
  int gm_cx = 0, gm_cy = 0;
  double gm_prob = -1.0;
  // low-latency completion flag (k_publish in score_kernels.hip)
  slamhip::PinnedBuf<unsigned> h_done_flag;  // coherent
  unsigned seq = 0;
  // second launch lane (stream + completion flag): the filter's two job groups score on one lane each,
  // so that one group's kernel can start while the other's is still draining / publishing
  hipStream_t stream_b = nullptr;
  slamhip::PinnedBuf<unsigned> h_done_flag_b;
  unsigned seq_b = 0;
  hipEvent_t ev_fork = nullptr;
  void *shard = nullptr;  // RCCL group of the context (shard.cpp), or null
  void *mu_scratch = nullptr, *mu_bscratch = nullptr;  // K6 work buffers (map_update.hip), owned by the context
  void *mu_kscratch = nullptr;  // ... of slamhip_map_append_scan_batch: the per-job arena, staging, direction tables
  slamhip::DeviceBuf<unsigned char> d_render;  // the render kernels' output (map_render.hip): grows on demand
  size_t render_cap = 0;
  slamhip::DeviceBuf<unsigned char> d_scan_gen;  // slamhip_map_generate_scans' block in HBM (scan_generate.hip): grows on demand
  size_t scan_gen_cap = 0;
  std::vector<double> scan_gen_stage;  // ... and its host side: what goes up and what comes back, one copy each
  std::vector<void *> pyramids;  // the slamhip_pyramid objects made over this context's maps (map_pyramid.hip)
  void *pyr_many = nullptr;      // PyrManyStage: the staging of the multi-request pyramid launches (map_pyramid.hip)
  void *pyr_refresh = nullptr;   // PyrRefreshStage: slamhip_pyramid_refresh_batch's job tables and last plan (map_pyramid.hip)
  bool low_latency = true;
  bool stage_poses = false;  // copy poses to HBM first instead of reading them over PCIe
  // slamhip_ctx_set_option: equivalent execution paths (defaults = what is measured)
  bool filter_chains = true, k6_batch_fast = true, k6_batch_key64 = false, resident_chains = true, tbm_plane = true;
  int inert_tail = 2;  // SLAMHIP_OPT_INERT_TAIL
  bool raw_prologue = true;  // SLAMHIP_OPT_RAW_PROLOGUE
  long long raw_prologue_matches = 0;  // SLAMHIP_OPT_RAW_PROLOGUE_MATCHES
  int k6_path = 0;
  // profiling: event pairs recorded around scoring launches, resolved lazily in profile_read
  bool profile = false;
  std::vector<hipEvent_t> ev_pool;
  size_t ev_used = 0;
  std::vector<char> ev_kind;  // per event pair: 0 scoring dispatch, 1 one map update (K6 pipeline)
  double prof_ms = 0.0;
  long long prof_launches = 0, prof_units = 0;
  double prof_k6_ms = 0.0;
  long long prof_k6_calls = 0, prof_k6_records = 0;
};

namespace slamhip {
// the context knows the angles of the current scan's points (what SLAMHIP_POSE_TRIG_RAW_EXACT needs) ...
inline bool scan_angles_known(const slamhip_ctx *ctx) {
  return ctx->scan_angle_lazy || (int)ctx->h_scan_angle.size() == ctx->scan_n;
}
// ... and has them in h_scan_angle (slamhip_api.cpp)
void scan_angles_materialise(slamhip_ctx *ctx);
// ... and in HBM (uploaded on first use); SLAMHIP_ERR_STATE where it does not know them
int scan_exact_angles(slamhip_ctx *ctx, const double **d_angle);
// The raw scan's upload in two halves (slamhip_api.cpp; slamhip_scan_filter_upload is the two in a row).
// scan_filter_stage: filter, weights, the staging buffer filled, the new scan recorded as the current one --
// ctx->scan_pending.active unless the filter kept nothing.  scan_assemble_now: k_scan_assemble on the context's stream
// and the second lane's wait, if the scan is still pending (else nothing): THE way the scan block gets written when no
// chain does it -- the plain path and every fail-over call this one function.  scan_fused_done: a chain launched with
// HcChainArgs::raw has reported its result -- every workgroup has read the staging buffer, the bookkeeping one has
// written the block.  scan_record_finish: the host's copies of the scan's weights / factors, made behind the launch.
int scan_filter_stage(slamhip_ctx *ctx, int map_id, int n, const double *range, const double *angle, const int *is_occ,
                      const double *factor, int trig_mode, double a_min, double a_max, double a_inc, const double pose[3],
                      unsigned skip_rate, double max_range, int bounded, int weighting, int *kept_n, int *kept_idx);
int scan_assemble_now(slamhip_ctx *ctx);
int scan_fused_done(slamhip_ctx *ctx);
void scan_record_finish(slamhip_ctx *ctx);
// scoring target made of per-slot copy-on-write maps (tile_pool.h) instead of a bound dense window;
// pose p reads the map of slot ctx->h_pose_slot[p]
struct TiledTarget {
  const double *pool;
  const int *tables;
  int table_stride, tiles_x, width, height, origin_x, origin_y;
  double scale;
  double unknown[4];
  int nbr_ok;  // the tiles' in-tile neighbourhood masks are valid for threshold nbr_th (tile_pool.h)
  double nbr_th;
};
int ensure_pose_capacity(slamhip_ctx *ctx, int n);
// scores n poses whose (x,y,theta) sit in ctx->h_poses; results land in ctx->h_scores (synchronous)
// `off`: window of the staging buffers (poses at h_poses + 3 off, results at h_scores + off, ...);
// `async_seq` != null: return right after the launch with the number score_wait() takes (0 = the
// call was synchronous after all, nothing to wait for)
// `lane` 1: launch on the context's second stream / completion flag (zero-copy path only)
int score_staged(slamhip_ctx *ctx, int map_id, const slamhip_spe_cfg *cfg, int n_poses,
                 const TiledTarget *tiled = nullptr, int off = 0, unsigned *async_seq = nullptr, int lane = 0);
int score_wait(slamhip_ctx *ctx, unsigned seq, int lane = 0);
// orders the second lane behind everything queued on the first so far (scan upload, map updates)
int lane_fork(slamhip_ctx *ctx);
// (oie_eff, optional: a caller that passes it takes the map through its probability plane where there is one -- the
// view is then an OCC one and *oie_eff the occupancy OIE, see DeviceMap::d_prob; without it the view is the map's own)
int score_views(slamhip_ctx *ctx, int map_id, const slamhip_spe_cfg *cfg, MapView *map, ScanView *scan,
                int *cell_model, const TiledTarget *tiled = nullptr, int *oie_eff = nullptr);
// the map half of score_views (plane included) for a job whose scan is not the context's current one
int score_map_view(slamhip_ctx *ctx, int map_id, const slamhip_spe_cfg *cfg, MapView *map, int *cell_model, int *oie_eff);
int profile_event_pair(slamhip_ctx *ctx, hipEvent_t *e0, hipEvent_t *e1, int kind = 0);
// An event pair recorded AROUND a pipeline (the map update): every exit between the first record and the second --
// an empty update, a failed grow, a HIP error -- would leave a pair whose end was never recorded (or holds a stale
// time from the pool's last use), and slamhip_profile_read would fail on it.  The guard records the end on the
// way out unless close() did.
struct ProfilePairGuard {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  hipStream_t stream = nullptr;
  bool closed = true;
  int open(slamhip_ctx *ctx, hipStream_t st, int kind);
  int close();  // records the end of the pair; SLAMHIP_OK when profiling is off
  bool on() const { return e1 != nullptr; }
  ~ProfilePairGuard() {
    if (!closed && e1) (void)hipEventRecord(e1, stream);
  }
};

// ---- many hill-climbing chains over the GMapping OOPE in shared launches (matchers.cpp; the filter's lock-step
// replacement: one chain per particle, same map, same scan, no carry-in -- DESIGN.md section 7)
struct GmChainResult {
  double pose[3];
  double prob;
  long long calls, evaluated;
  int steps;
  int cx, cy;    // the cache entry the chain ended with
  double cprob;
  GmPoseInfo first_info;  // side outputs and raw score of the initial pose
  double first_raw;
  int error;     // 3: a one-run scan sat on the path: the caller redoes this match on the host-driven path
};
struct GmMultiChain;
// tiled + slots: chain c reads the copy-on-write map in slot slots[c] of the tile pool instead of the dense map
int gm_multi_chain_run(slamhip_ctx *ctx, GmMultiChain **scratch, int map_id, const slamhip_spe_cfg *cfg,
                       unsigned max_failed, double dt, double dr, int n, const double *inits, GmChainResult *out,
                       long long *kernels_launched, const TiledTarget *tiled = nullptr, const int *slots = nullptr);
void gm_multi_chain_free(GmMultiChain *s);
// whether gm_multi_chain_run would take n chains as ONE co-resident launch (hc_resident_gm.hip) on this context
bool gm_multi_chain_fits_resident(slamhip_ctx *ctx, int n);
}  // namespace slamhip
