// map_pyramid_score.h -- what map_pyramid.hip (levels, k_pyr_score) and m3rsm.hip (k_m3rsm_expand) share: the pyramid
// object, the arguments of a bound-scoring launch and the per-candidate scoring body both kernels run.
#pragma once

#include <vector>

#include "map_pyramid_device.h"
#include "score_device.h"

// a pyramid's staging in HBM and pinned memory, apart from the levels: gone with the pyramid, or -- the object outlives
// its context -- when the context goes (pyr_free_staging assigns an empty one)
struct slamhip_pyramid_staging {
  // slamhip_pyramid_score_matches' staging in HBM: rotation | rect | sin, cos per candidate; scores; levels; terms
  slamhip::DeviceBuf<double> d_in, d_scores, d_terms;
  slamhip::DeviceBuf<int> d_levels;
  int in_cap = 0;
  size_t terms_cap = 0;
  // slamhip_pyramid_expand_matches' staging (m3rsm.hip): parents as above; per slot rect | score | level in one block;
  // h_x: the pinned host side of both
  slamhip::DeviceBuf<double> d_x_in, d_x_out;
  slamhip::PinnedBuf<double> h_x;
  int x_parent_cap = 0;
  size_t x_slot_cap = 0;
  // SLAMHIP_POSE_TRIG_RAW_EXACT: the table of exact beam directions of the launch under way (RawTrig), cos rows in front
  // of the sin rows
  slamhip::DeviceBuf<double> d_raw;
  size_t raw_cap = 0;
};

struct slamhip_pyramid : slamhip_pyramid_staging {
  slamhip_ctx *ctx = nullptr;  // null once the context has gone
  int fine_id = -1, first_id = -1, oie = 0;
  int cell_model = 0;
  // the fine map the levels were planned for: a re-bound (grown) fine map needs slamhip_pyramid_rebuild
  int fine_w = 0, fine_h = 0, fine_ox = 0, fine_oy = 0;
  const double *fine_payload = nullptr;
  slamhip::pyr::Plan plan{};
  std::vector<slamhip::DeviceBuf<int>> d_coord;  // per level: the fine coordinate of every cell's winner (x, y)
  std::vector<const double *> lv_payload;        // per level: the payload the table below points at
  slamhip::DeviceBuf<slamhip::MapView> d_views;  // plan.n + 1 views, the fine map first
};

namespace slamhip {

constexpr int kPyrThreads = 256;

// What a candidate is scored against: a pyramid's level table, a scan and the pose the drifts are added to.  One per
// launch in the single-request kernels (MatchArgs is one); one per REQUEST, in a table in HBM, in the multi-request ones.
struct PyrSource {
  const MapView *levels;  // n_levels views, the fine map first
  int n_levels;
  ScanView scan;
  double base[3];
  const double *angle;  // the scan's point angles in HBM: SLAMHIP_POSE_TRIG_RAW_EXACT's tabulation reads them, else null
};

// SLAMHIP_POSE_TRIG_RAW_EXACT, the reference's default provider (RawTrigonometryProvider under
// LaserScan2D::to_cartesian(rot + pose.theta), m3rsm_engine.h:300-314): a beam's direction is libm's
// cos / sin((rotation + base heading) + angle[b]) -- a function of (request, rotation, beam) alone, whatever the
// rectangle.  The distinct (request, rotation) pairs of a call are the ROWS of a table filled by one launch in front of
// the scoring one (k_pyr_raw_table, map_pyramid.hip); candidate / parent i takes its beams' directions from row row[i]
// (null: row i) as they stand.  Null cos: the launch is not a RAW one.
struct RawTrig {
  const double *cos, *sin;  // n_rows x stride each
  const int *row;           // per candidate / parent
  size_t stride;
};

struct MatchArgs : PyrSource {
  const double *rotation;  // n
  const double *rect;      // n x (bot, top, left, right)
  const double *pose_sc;   // optional n x (sin, cos) of rotation + heading from the host; null = device sincos
  double *scores;
  int *level_out;
  double *terms;  // beam-order sum only: n x scan.n (multi-request: the rows lie where ManyArgs::terms_off says)
  int n, oie, oope;
  RawTrig raw;  // read by the RAW instantiations only
};

// The multi-request launches (k_pyr_score_many, k_m3rsm_expand_many): candidate / parent i belongs to request[i], whose
// scan, levels and base pose are table[request[i]].  m's own PyrSource part is not read.  The requests' beam counts differ,
// so the per-beam terms of the beam-order sum have no common stride: parent i's rows start at terms + terms_off[i], one row
// of table[request[i]].scan.n doubles per output of that parent.
struct ManyArgs {
  MatchArgs m;
  const PyrSource *table;
  const int *request;          // n
  const long long *terms_off;  // n, beam-order sum only
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
// ... of a multi-request launch with `slots` outputs per parent (1: the bounds kernel)
int pyr_launch_sum_sequential_many(const ManyArgs &a, size_t n_out, int slots, hipStream_t stream);

// ---- SLAMHIP_POSE_TRIG_RAW_EXACT (map_pyramid.hip) ----
// which libm build the tables restate (SLAMHIP_ERR_UNSUPPORTED where neither matches) and the current scan's angles in
// HBM (SLAMHIP_ERR_STATE where the context has none); launches nothing
int pyr_raw_prepare(slamhip_ctx *ctx, bool *fma, const double **d_angle);
// the distinct rotations (bit patterns) of n candidates / parents of one request, in order of first appearance:
// row_out[i] = the row of candidate i, rot_rows = the rows' rotations
void pyr_raw_rows(int n, const double *rotation, int *row_out, std::vector<double> *rot_rows);
// queues the tabulation of n_rows rows -- row r = cos / sin((d_rot_rows[r] + base_theta) + d_angle[b]), b < n_beams -- into
// the pyramid's table (grown on demand) and fills *out but for `row`
int pyr_raw_queue_table(slamhip_pyramid *p, bool fma, const double *d_rot_rows, int n_rows, double base_theta,
                        const double *d_angle, int n_beams, RawTrig *out);

// The staging of the multi-request launches (slamhip_pyramid_score_requests / _expand_requests), kept by the context:
// one pinned block and one block in HBM, each the inputs (table | terms offsets | rotation | rect | sin, cos | request)
// in front of the outputs (rect | score | level per slot), and the terms.
struct PyrManyStage {
  PinnedBuf<char> h;
  DeviceBuf<char> d;
  size_t cap = 0, out_at = 0;  // out_at: where the outputs of the launch staged last begin
  DeviceBuf<double> d_terms;
  size_t terms_cap = 0;
  DeviceBuf<double> d_raw;  // SLAMHIP_POSE_TRIG_RAW_EXACT: the launch's table of beam directions (RawTrig)
  size_t raw_cap = 0;
};
void pyr_many_release(slamhip_ctx *ctx);
// checks a request table against the context and cfg and fills the sources the kernels read
// (under SLAMHIP_POSE_TRIG_RAW_EXACT also that every request's slot has angles and the host's libm is a known build)
int pyr_many_sources(slamhip_ctx *ctx, const slamhip_spe_cfg *cfg, int n_requests, const slamhip_m3rsm_request *req,
                     std::vector<PyrSource> *out);
// ... the parts of that, for a caller whose requests' scans are not in stored slots: the pyramid's checks (the first
// request's also check cfg) and the level table; the pose; the scan as a block of five rows at `stride` with n points and
// their total weight, and the row of the points' angles (SLAMHIP_POSE_TRIG_RAW_EXACT, else null)
int pyr_source_begin(slamhip_ctx *ctx, const slamhip_spe_cfg *cfg, slamhip_pyramid *p, const slamhip_pyramid **first, PyrSource *q);
int pyr_source_pose(const double pose[3], PyrSource *q);
void pyr_source_block(const double *d, size_t stride, int n, double tot_w, const double *d_angle, PyrSource *q);
// slamhip_pyramid_score_requests / slamhip_pyramid_expand_requests (m3rsm.hip) below the sources: the candidates' checks,
// the staging, the launch, the fetch (cell_model: the pyramids')
int pyr_score_sources(slamhip_ctx *ctx, const slamhip_spe_cfg *cfg, const std::vector<PyrSource> &src, int cell_model, int n,
                      const int *request, const double *rotation, const double *rect, double *score_out, int *level_out);
int pyr_expand_sources(slamhip_ctx *ctx, const slamhip_spe_cfg *cfg, const std::vector<PyrSource> &src, int cell_model, int n,
                       const int *request, const double *rotation, const double *rect, double translation_step, int depth,
                       double *rect_out, double *score_out, int *level_out);
// stages n candidates (request, rotation, rect) of the table, leaving room for n x slots outputs; fills a->m's inputs and
// outputs, a->table, a->request, a->terms_off.  After the launch: pyr_many_fetch.  Under SLAMHIP_POSE_TRIG_RAW_EXACT it
// also stages the rows of the distinct (request, rotation) pairs, queues their tabulation and fills a->m.raw
int pyr_many_stage(slamhip_ctx *ctx, const slamhip_spe_cfg *cfg, const std::vector<PyrSource> &src, int n, const int *request,
                   const double *rotation, const double *rect, int slots, ManyArgs *a, double **d_rect_out);
// request indices inside the table, finite rotations and rectangles (reversed ones only where the caller lets them through)
int pyr_many_check_batch(int n_requests, int n, const int *request, const double *rotation, const double *rect, bool reversed_ok);
int pyr_many_fetch(slamhip_ctx *ctx, size_t n_out, bool with_rect, double *rect_out, double *score_out, int *level_out);

#if defined(__HIPCC__)
// Match::prob_upper_bound of ONE candidate by the whole workgroup (kPyrThreads threads): levels, scan and base pose
// from `q` (the launch's own MatchArgs, or the candidate's entry of the request table, read once by its caller),
// rotation index `src` (into a.rotation / a.pose_sc), the rectangle in registers, the result at index `out` of a.scores /
// a.level_out, the per-beam terms (beam-order sum; else `terms` is null) from terms[terms_at] on.  Every thread of the
// workgroup calls it with the same arguments.  RAW: a beam's direction is read from row a.raw.row[src] of the table of
// exact cos / sin((rotation + heading) + angle) -- no pose rotation, no sincos, no barrier for it; everything behind the
// direction is the other modes' code.
template <int MODEL, bool RAW = false>
__device__ __forceinline__ void pyr_score_one(const PyrSource &q, const MatchArgs &a, size_t src, size_t out, double *terms,
                                              size_t terms_at, double bot, double top, double left, double right, double *s_trig,
                                              double *s_part) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int n = q.scan.n;
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
  while (lv < q.n_levels - 1 && !(target <= q.levels[lv].scale)) ++lv;
  const MapView map = q.levels[lv];
  // LightWeightRectangle::center() added to the pose
  const double x = q.base[0] + (left + hside / 2), y = q.base[1] + (bot + vside / 2);
  double sn = 0.0, cs = 1.0;
  const double *cos_a = q.scan.cos_a, *sin_a = q.scan.sin_a;
  if (RAW) {
    const size_t at = (size_t)(a.raw.row ? a.raw.row[src] : (int)src) * a.raw.stride;
    cos_a = a.raw.cos + at;
    sin_a = a.raw.sin + at;
  } else {
    if (t == 0) {
      if (a.pose_sc) {
        sn = a.pose_sc[2 * src];
        cs = a.pose_sc[2 * src + 1];
      } else {
        sincos(a.rotation[src] + q.base[2], &sn, &cs);
      }
      s_trig[0] = sn;
      s_trig[1] = cs;
    }
    __syncthreads();
    sn = s_trig[0];
    cs = s_trig[1];
  }
  const double half_v = (top - bot) / 2, half_h = (right - left) / 2;
  double acc = 0.0;
  for (int b = t; b < n; b += kPyrThreads) {
    const double ca = cos_a[b], sa = sin_a[b], r = q.scan.range[b];
    const double c = RAW ? ca : cs * ca - sn * sa;
    const double s = RAW ? sa : sn * ca + cs * sa;
    const double ox = x + r * c, oy = y + r * s;
    const double pr = window_probability<MODEL>(map, a.oie, a.oope, half_v, half_h, ox, oy);
    const double term = pr * q.scan.weight[b] * q.scan.factor[b];
    if (terms) terms[terms_at + b] = term;
    acc = acc + term;
  }
  acc = wave_xor_sum(acc);
  if (lane == 0) s_part[wave] = acc;
  __syncthreads();
  if (t == 0) {
    const double total = (s_part[0] + s_part[1]) + (s_part[2] + s_part[3]);
    a.scores[out] = (q.scan.tot_w == 0.0) ? __builtin_nan("") : total / q.scan.tot_w;
    a.level_out[out] = lv;
  }
}
#endif

}  // namespace slamhip
