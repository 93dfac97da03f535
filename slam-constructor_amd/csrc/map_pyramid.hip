// map_pyramid.hip -- max-impact levels over a resident map and the bound scorer that reads them
// (include/slamhip.h "map pyramid"; the level definition: map_pyramid_device.h).
//
// What it replaces (paths relative to the reference root):
//   M3RSMRescalableGridMap::update_coarser_maps   src/core/scan_matchers/m3rsm_engine.h:101-127 -- per updated fine
//                                                 cell a walk up the levels, inside GridMap::update
//   Match::Match (prob_upper_bound)               src/core/scan_matchers/m3rsm_engine.h:156-180 -- rescale() to the
//                                                 level of the translation rectangle, then one scorer call
//
// Build: level k is made from level k - 1 (level 1 from the fine map), one thread per coarse cell reading the 2 x 2
// cells under it and writing the winner's payload and the fine coordinate it came from (pyr::reduce_cell); the kernels
// of the levels follow each other on the context's stream.  A refresh runs the same kernel over the coarse cells whose
// blocks meet the changed fine window.  Bandwidth bound: the fine map is read once, level k written once and read once.
//
// Score: one workgroup of 256 threads per candidate.  It picks the candidate's level from its rectangle, takes that
// level's MapView from a table in HBM and runs k_score_window's body (score_kernels.hip) for one pose: thread t adds the
// beams t, t + 256, ... in ascending order, the wave butterfly, (g0 + g1) + (g2 + g3) -- the canonical sum, hence the
// bits slamhip_score_poses gives for that pose on that level's map with cfg.area = the rectangle.  k_pyr_score_many scores
// candidates of several requests in one launch: level table, scan and base pose per candidate from a request table in HBM
// (slamhip_pyramid_score_requests; the staging both multi-request launches share is in here too).
// SLAMHIP_POSE_TRIG_RAW_EXACT (the reference's default trig provider, bit for bit): k_pyr_raw_table(_many) tabulate
// glibc's cos / sin((rotation + heading) + angle) for the distinct rotations of a call in one launch in front of the
// scoring one, whose RAW instantiation reads its candidate's row (RawTrig, map_pyramid_score.h).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "kernel_pick.h"
#include "libm_exact.h"
#include "map_pyramid_device.h"
#include "map_pyramid_score.h"
#include "pyr_refresh_batch_plan.h"
#include "score_device.h"

namespace slamhip {

int pyr_invalid(const char *msg) {
  set_error(msg);
  return SLAMHIP_ERR_INVALID;
}
int pyr_state(const char *msg) {
  set_error(msg);
  return SLAMHIP_ERR_STATE;
}

namespace {

constexpr int kMaxGridY = 65535;

DeviceMap *bound_map(slamhip_ctx *ctx, int map_id) {
  if (!ctx || map_id < 0 || map_id >= (int)ctx->maps.size() || !ctx->maps[map_id].bound) return nullptr;
  return &ctx->maps[map_id];
}

// ---- build ---------------------------------------------------------------------------------------
// cells [cx0, cx0 + cw) x [cy0, cy0 + ch) of dst (inside its window: the launcher clips)
template <int CD>
__global__ __launch_bounds__(kPyrThreads) void k_pyr_reduce(pyr::Level src, pyr::Level dst, int bias_x, int bias_y, int model,
                                                            int oie, double u0, double u1, double u2, double u3, int cx0,
                                                            int cy0, int cw, int ch) {
  const int x = (int)(blockIdx.x * kPyrThreads + threadIdx.x);
  if (x >= cw) return;
  const double unknown[4] = {u0, u1, u2, u3};
  for (int y = (int)blockIdx.y; y < ch; y += (int)gridDim.y)
    pyr::reduce_cell<CD>(src, dst, bias_x, bias_y, model, oie, unknown, cx0 + x, cy0 + y);
}

// ---- refresh of several pyramids (slamhip_pyramid_refresh_batch; the planning: pyr_refresh_batch_plan.h) ----------
// One (job, level) of a call, read from the job table in HBM: k_pyr_reduce's arguments.  Cells
// [cx0, cx0 + cw) x [cy0, cy0 + ch) of dst lie inside dst's window (the plan clips), cd = doubles per cell (1 or 4).
static_assert(pyr_plan::kThreads == kPyrThreads, "the plan sizes the grids for the kernels' workgroup");
struct PyrReduceEntry {
  pyr::Level src, dst;
  int bias_x, bias_y;
  int cx0, cy0, cw, ch;
  int model, oie, cd, pad;
  double unknown[4];
};

// cell c (row-major) of the entry's window; c < cw * ch
__device__ __forceinline__ void reduce_entry_cell(const PyrReduceEntry &e, int c) {
  const int y = c / e.cw, x = c - y * e.cw;
  if (e.cd == 1) pyr::reduce_cell<1>(e.src, e.dst, e.bias_x, e.bias_y, e.model, e.oie, e.unknown, e.cx0 + x, e.cy0 + y);
  else pyr::reduce_cell<4>(e.src, e.dst, e.bias_x, e.bias_y, e.model, e.oie, e.unknown, e.cx0 + x, e.cy0 + y);
}

// One level of every job of a round whose window at that level is large: a flat grid, job after job, a thread per cell;
// workgroup b belongs to the job j with off[j] <= b < off[j + 1] (uniform per workgroup: entry and offsets go through
// the scalar cache).  The jobs' pyramids differ, so no cell is written twice and no cell read is written by this launch.
__global__ __launch_bounds__(kPyrThreads) void k_pyr_reduce_batch(const PyrReduceEntry *__restrict__ entries,
                                                                  const unsigned *__restrict__ off, int n_jobs) {
  const int j = pyr_plan::find_job(off, n_jobs, blockIdx.x);
  const PyrReduceEntry &e = entries[j];
  const long long c = (long long)(blockIdx.x - off[j]) * kPyrThreads + threadIdx.x;
  if (c >= (long long)e.cw * e.ch) return;
  reduce_entry_cell(e, (int)c);
}

// The upper levels of every job of a round: workgroup j walks the n entries of its run bottom-up, a workgroup barrier
// between levels.  Level lv + 1 reads payload and coordinates this same workgroup has just written for level lv (its
// other source cells were written by earlier kernels): the waves of a workgroup run on one CU and share its vector L1,
// which its own stores go through, so __syncthreads() -- a workgroup-scope release (the stores' vmcnt wait), the
// barrier, a workgroup-scope acquire -- is all the ordering this needs; nothing here is read by another workgroup.
// The loop bounds come from the table and are uniform, and every thread reaches every barrier (no early return).
__global__ __launch_bounds__(kPyrThreads) void k_pyr_reduce_tail(const PyrReduceEntry *entries, const int *__restrict__ runs) {
  const int first = runs[2 * blockIdx.x], n = runs[2 * blockIdx.x + 1];
  for (int k = 0; k < n; ++k) {
    const PyrReduceEntry &e = entries[first + k];
    const int cells = e.cw * e.ch;  // (at most kPyrThreads by the plan; walked all the same)
    for (int c = (int)threadIdx.x; c < cells; c += kPyrThreads) reduce_entry_cell(e, c);
    __syncthreads();
  }
}

pyr::Level level_of(const DeviceMap &m, int *coord) {
  return pyr::Level{m.d_payload, coord, m.width, m.height, m.pitch, m.origin_x, m.origin_y};
}

// the levels' kernels over the fine window [x0, x0 + w) x [y0, y0 + h), queued on the context's stream
int queue_levels(slamhip_pyramid *p, int x0, int y0, int w, int h) {
  slamhip_ctx *ctx = p->ctx;
  const pyr::Plan &pl = p->plan;
  ProfilePairGuard prof;  // (while profiling is on: the levels' kernels, first to last, in kernel_ms_total)
  int rc = prof.open(ctx, ctx->stream, 0);
  if (rc) return rc;
  for (int lv = 1; lv <= pl.n; ++lv) {
    const DeviceMap &src = ctx->maps[lv == 1 ? p->fine_id : p->first_id + lv - 2];
    DeviceMap &dst = ctx->maps[p->first_id + lv - 1];
    int cx0, cy0, cx1, cy1;
    pyr::level_window(pl, p->fine_ox, p->fine_oy, lv, x0, y0, w, h, &cx0, &cy0, &cx1, &cy1);
    cx0 = std::max(cx0, 0);
    cy0 = std::max(cy0, 0);
    cx1 = std::min(cx1, dst.width - 1);
    cy1 = std::min(cy1, dst.height - 1);
    if (cx1 < cx0 || cy1 < cy0) return pyr_invalid("internal: a level window outside its level");
    const int cw = cx1 - cx0 + 1, ch = cy1 - cy0 + 1;
    const bool top = lv == pl.n;
    const int bias_x = top ? 0 : src.origin_x - 2 * dst.origin_x, bias_y = top ? 0 : src.origin_y - 2 * dst.origin_y;
    const pyr::Level s = level_of(src, lv == 1 ? nullptr : p->d_coord[lv - 2].get()), d = level_of(dst, p->d_coord[lv - 1].get());
    const dim3 grid((cw + kPyrThreads - 1) / kPyrThreads, std::min(ch, kMaxGridY));
    const auto kernel = cell_doubles(p->cell_model) == 1 ? k_pyr_reduce<1> : k_pyr_reduce<4>;
    SLAMHIP_CHECK(launch_kernel(kernel, grid, dim3(kPyrThreads), 0, ctx->stream, nullptr, nullptr, s, d, bias_x, bias_y,
                                p->cell_model, p->oie, dst.unknown[0], dst.unknown[1], dst.unknown[2], dst.unknown[3], cx0, cy0,
                                cw, ch));
    if (dst.prob_ok)  // a level somebody has scored with the 1-cell OOPE: its probability plane follows its cells
      SLAMHIP_CHECK(launch_prob_build(dst.cell_model, dst.d_payload, dst.d_prob, dst.width, dst.height, dst.pitch, cx0, cy0, cw,
                                      ch, ctx->stream));
  }
  rc = prof.close();
  if (rc) return rc;
  if (ctx->profile) ctx->prof_launches += 1;
  return SLAMHIP_OK;
}

void free_levels(slamhip_pyramid *p, bool release_maps) {
  slamhip_ctx *ctx = p->ctx;
  if (ctx) {
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    if (release_maps)
      for (int lv = 1; lv <= (int)p->lv_payload.size() - 1; ++lv) {
        // (only what is still the map this pyramid bound: an id the caller has re-bound since is the caller's)
        DeviceMap *m = bound_map(ctx, p->first_id + lv - 1);
        if (m && m->d_payload == p->lv_payload[lv]) (void)slamhip_map_release(ctx, p->first_id + lv - 1);
      }
  }
  p->d_coord.clear();
  p->lv_payload.clear();
  p->d_views.reset();
  p->plan.n = 0;
}

// plans the levels over the fine map as it is bound now, binds them and queues the whole build
int make_levels(slamhip_pyramid *p) {
  slamhip_ctx *ctx = p->ctx;
  DeviceMap *fine = bound_map(ctx, p->fine_id);
  if (!fine) return pyr_invalid("the fine map is not bound");
  if (fine->bytes == 0 || fine->cell_model == SLAMHIP_CELL_GMAPPING)
    return pyr_invalid("a pyramid stands over a dense OCC, TBM or CREDIBILIST map");
  if (!pyr::check_oie(fine->cell_model, p->oie))
    return pyr_invalid("unknown OIE, or OccupancyOIE over belief cells (they are scored under the discrepancy OIE only)");
  pyr::Plan pl;
  if (!pyr::plan_levels(fine->width, fine->height, fine->origin_x, fine->origin_y, fine->scale, &pl))
    return pyr_invalid("the fine map reaches beyond 2^30 cells from its origin");
  if (p->first_id < 0 || p->first_id + pl.n - 1 > 4095) return pyr_invalid("level map ids out of range [0, 4095]");
  if (p->fine_id >= p->first_id && p->fine_id < p->first_id + pl.n) return pyr_invalid("the level ids include the fine map's");
  for (int lv = 1; lv <= pl.n; ++lv)
    if (bound_map(ctx, p->first_id + lv - 1)) return pyr_invalid("a level map id is already bound");
  const int model = fine->cell_model;
  double unknown[4];
  for (int k = 0; k < 4; ++k) unknown[k] = fine->unknown[k];
  p->cell_model = model;
  p->plan = pl;
  p->d_coord.clear();
  p->d_coord.resize(pl.n);
  p->lv_payload.assign(pl.n + 1, nullptr);
  for (int lv = 1; lv <= pl.n; ++lv) {
    const int rc = slamhip_map_bind(ctx, p->first_id + lv - 1, model, pl.width[lv - 1], pl.height[lv - 1], pl.origin_x[lv - 1],
                                    pl.origin_y[lv - 1], pl.scale[lv - 1], unknown);
    if (rc) return rc;
    const DeviceMap &m = ctx->maps[p->first_id + lv - 1];
    p->lv_payload[lv] = m.d_payload;
    SLAMHIP_CHECK(p->d_coord[lv - 1].alloc(2 * (size_t)m.pitch * m.height));
  }
  fine = bound_map(ctx, p->fine_id);  // (binding may have moved the context's map table)
  p->fine_w = fine->width;
  p->fine_h = fine->height;
  p->fine_ox = fine->origin_x;
  p->fine_oy = fine->origin_y;
  p->fine_payload = p->lv_payload[0] = fine->d_payload;
  std::vector<MapView> views(pl.n + 1);
  views[0] = view_of(*fine);
  for (int lv = 1; lv <= pl.n; ++lv) views[lv] = view_of(ctx->maps[p->first_id + lv - 1]);
  SLAMHIP_CHECK(p->d_views.alloc(views.size()));
  SLAMHIP_CHECK(hipMemcpy(p->d_views.get(), views.data(), sizeof(MapView) * views.size(), hipMemcpyHostToDevice));
  return queue_levels(p, 0, 0, p->fine_w, p->fine_h);
}

// the maps are still the ones the levels were made over and of
int check_fresh(const slamhip_pyramid *p) {
  if (!p || !p->ctx) return pyr_invalid("null pyramid, or one whose context has been destroyed");
  if (p->plan.n <= 0) return pyr_state("the pyramid has no levels (a failed rebuild): slamhip_pyramid_rebuild");
  const DeviceMap *fine = bound_map(p->ctx, p->fine_id);
  if (!fine || fine->d_payload != p->fine_payload || fine->width != p->fine_w || fine->height != p->fine_h ||
      fine->origin_x != p->fine_ox || fine->origin_y != p->fine_oy)
    return pyr_state("the fine map has been re-bound since the levels were made: slamhip_pyramid_rebuild");
  for (int lv = 1; lv <= p->plan.n; ++lv) {
    const DeviceMap *m = bound_map(p->ctx, p->first_id + lv - 1);
    if (!m || m->d_payload != p->lv_payload[lv]) return pyr_state("a level map has been released or re-bound by the caller");
  }
  return SLAMHIP_OK;
}

// ---- score ---------------------------------------------------------------------------------------
template <int MODEL, bool RAW>
__global__ __launch_bounds__(kPyrThreads) void k_pyr_score(MatchArgs a) {
  __shared__ double s_trig[2];
  __shared__ double s_part[4];
  const size_t i = blockIdx.x;
  pyr_score_one<MODEL, RAW>(a, a, i, i, a.terms, i * (size_t)a.scan.n, a.rect[4 * i], a.rect[4 * i + 1], a.rect[4 * i + 2],
                            a.rect[4 * i + 3], s_trig, s_part);
}

// the same for candidates of several requests: the workgroup's scan, levels and base pose are its request's entry of the
// table (one read per workgroup, uniform: it goes through the scalar cache), the rest is k_pyr_score
template <int MODEL, bool RAW>
__global__ __launch_bounds__(kPyrThreads) void k_pyr_score_many(ManyArgs a) {
  __shared__ double s_trig[2];
  __shared__ double s_part[4];
  const size_t i = blockIdx.x;
  const PyrSource q = a.table[a.request[i]];
  pyr_score_one<MODEL, RAW>(q, a.m, i, i, a.m.terms, a.m.terms ? (size_t)a.terms_off[i] : 0, a.m.rect[4 * i],
                            a.m.rect[4 * i + 1], a.m.rect[4 * i + 2], a.m.rect[4 * i + 3], s_trig, s_part);
}

// ---- SLAMHIP_POSE_TRIG_RAW_EXACT: the table of beam directions (RawTrig, map_pyramid_score.h) ------------------------
// Row r of a launch: glibc's cos / sin(t_r + angle[b]) for the row's scan, t_r = rotation + base heading formed as ONE
// double first (fscan->to_cartesian(rot + pose.theta), then RawTrigonometryProvider's _base_angle + angle_rad).  One
// thread per (row, beam); rows beyond the grid's y extent are walked.  Compute bound and tiny: a few dozen rows of a
// scan's beams per match.  Writes stay inside [r * stride, r * stride + n) with n <= stride, r < n_rows.
template <bool FMA>
__device__ __forceinline__ void raw_row_fill(double t, const double *__restrict__ angle, int n, double *__restrict__ out_cos,
                                             double *__restrict__ out_sin) {
  for (int b = (int)(blockIdx.x * 256 + threadIdx.x); b < n; b += (int)(gridDim.x * 256)) {
    const double x = t + angle[b];
    out_cos[b] = libm_exact::cos_<FMA>(x);
    out_sin[b] = libm_exact::sin_<FMA>(x);
  }
}

template <bool FMA>
__global__ __launch_bounds__(256) void k_pyr_raw_table(const double *__restrict__ rot_rows, int n_rows, double base_theta,
                                                      const double *__restrict__ angle, int n, size_t stride,
                                                      double *__restrict__ out_cos, double *__restrict__ out_sin) {
  for (int r = (int)blockIdx.y; r < n_rows; r += (int)gridDim.y)
    raw_row_fill<FMA>(rot_rows[r] + base_theta, angle, n, out_cos + (size_t)r * stride, out_sin + (size_t)r * stride);
}

// ... for rows of several requests: row r belongs to request row_request[r], whose angles, beam count and heading come
// from the request table (beam counts differ: a row fills its own request's n of the common stride)
template <bool FMA>
__global__ __launch_bounds__(256) void k_pyr_raw_table_many(const double *__restrict__ rot_rows, const int *__restrict__ row_request,
                                                           int n_rows, const PyrSource *__restrict__ table, size_t stride,
                                                           double *__restrict__ out_cos, double *__restrict__ out_sin) {
  for (int r = (int)blockIdx.y; r < n_rows; r += (int)gridDim.y) {
    const PyrSource &q = table[row_request[r]];
    raw_row_fill<FMA>(rot_rows[r] + q.base[2], q.angle, q.scan.n, out_cos + (size_t)r * stride, out_sin + (size_t)r * stride);
  }
}

dim3 raw_table_grid(int max_beams, int n_rows) { return dim3((max_beams + 255) / 256, std::min(n_rows, kMaxGridY)); }

__device__ __forceinline__ double sum_sequential_row(const double *row, int n, double tot_w) {
  double acc = 0.0;
  for (int b = 0; b < n; ++b) acc = acc + row[b];
  return (tot_w == 0.0) ? __builtin_nan("") : acc / tot_w;
}

// the reference's beam-order sum over the terms (k_sum_sequential's loop), one lane per candidate that has a level
__global__ __launch_bounds__(64) void k_pyr_sum_sequential(const double *terms, const int *level, int n_cand, int n, double tot_w,
                                                           double *scores) {
  const int p = blockIdx.x * 64 + threadIdx.x;
  if (p >= n_cand || level[p] < 0) return;
  scores[p] = sum_sequential_row(terms + (size_t)p * n, n, tot_w);
}

// ... over the rows of a multi-request launch: output p is slot p % slots of parent p / slots
__global__ __launch_bounds__(64) void k_pyr_sum_sequential_many(ManyArgs a, int n_out, int slots) {
  const int p = blockIdx.x * 64 + threadIdx.x;
  if (p >= n_out || a.m.level_out[p] < 0) return;
  const int parent = p / slots;
  const ScanView &scan = a.table[a.request[parent]].scan;
  a.m.scores[p] = sum_sequential_row(a.m.terms + a.terms_off[parent] + (size_t)(p - parent * slots) * scan.n, scan.n, scan.tot_w);
}

int check_score_cfg(const slamhip_pyramid *p, const slamhip_spe_cfg *cfg) {
  if (!cfg) return pyr_invalid("null spe cfg");
  if (cfg->oope != SLAMHIP_OOPE_MAX && cfg->oope != SLAMHIP_OOPE_MEAN && cfg->oope != SLAMHIP_OOPE_OVERLAP)
    return pyr_invalid("bounds are scored with a window OOPE (max / mean / overlap)");
  if (cfg->oie != p->oie) return pyr_invalid("the scorer's OIE is not the one the levels were built with");
  if (cfg->sum_order != SLAMHIP_SUM_TREE256 && cfg->sum_order != SLAMHIP_SUM_SEQUENTIAL) return pyr_invalid("unknown sum order");
  return SLAMHIP_OK;
}

// queues the scoring of n candidates whose arrays are in HBM (pose_sc may be null; raw: the table of beam directions
// queued in front of this launch, or null)
int queue_score(slamhip_pyramid *p, const slamhip_spe_cfg *cfg, const double base[3], int n, const double *d_rotation,
                const double *d_rect, const double *d_pose_sc, const RawTrig *raw, double *d_scores, int *d_levels) {
  slamhip_ctx *ctx = p->ctx;
  MatchArgs a;
  int rc = pyr_fill_args(p, cfg, base, (size_t)n, &a);
  if (rc) return rc;
  a.rotation = d_rotation;
  a.rect = d_rect;
  a.pose_sc = d_pose_sc;
  a.scores = d_scores;
  a.level_out = d_levels;
  a.n = n;
  if (raw) a.raw = *raw;
  ProfilePairGuard prof;
  rc = prof.open(ctx, ctx->stream, 0);
  if (rc) return rc;
  typedef void (*Kernel)(MatchArgs);
  const Kernel kernel = pick_cell_model(p->cell_model, [raw](auto m) -> Kernel {
    return raw ? k_pyr_score<decltype(m)::value, true> : k_pyr_score<decltype(m)::value, false>;
  });
  SLAMHIP_CHECK(launch_kernel(kernel, dim3(n), dim3(kPyrThreads), 0, ctx->stream, nullptr, nullptr, a));
  if (a.terms) {
    rc = pyr_launch_sum_sequential(a, (size_t)n, ctx->stream);
    if (rc) return rc;
  }
  rc = prof.close();
  if (rc) return rc;
  if (ctx->profile) {
    ctx->prof_launches += 1;
    ctx->prof_units += (long long)n * a.scan.n;
  }
  return SLAMHIP_OK;
}

}  // namespace

int pyr_check_fresh(const slamhip_pyramid *p) { return check_fresh(p); }
int pyr_check_score_cfg(const slamhip_pyramid *p, const slamhip_spe_cfg *cfg) { return check_score_cfg(p, cfg); }

static int raw_libm_build(bool *fma) {
  const int variant = libm_variant();
  if (variant < 0) {
    set_error("this host's libm matches neither build of glibc's sin / cos restated in csrc/libm_exact.h: "
              "SLAMHIP_POSE_TRIG_RAW_EXACT is not available here");
    return SLAMHIP_ERR_UNSUPPORTED;
  }
  *fma = variant == 1;
  return SLAMHIP_OK;
}

int pyr_raw_prepare(slamhip_ctx *ctx, bool *fma, const double **d_angle) {
  const int rc = raw_libm_build(fma);
  if (rc) return rc;
  if (ctx->scan_n <= 0) return pyr_state("no scan uploaded");
  return scan_exact_angles(ctx, d_angle);
}

void pyr_raw_rows(int n, const double *rotation, int *row_out, std::vector<double> *rot_rows) {
  rot_rows->clear();
  for (int i = 0; i < n; ++i) {
    // (a layer of matches holds few rotations, and neighbours mostly share one: the row before is tried first)
    int r = i ? row_out[i - 1] : 0;
    if (!i || std::memcmp(&(*rot_rows)[r], &rotation[i], sizeof(double)) != 0) {
      for (r = 0; r < (int)rot_rows->size(); ++r)
        if (std::memcmp(&(*rot_rows)[r], &rotation[i], sizeof(double)) == 0) break;
      if (r == (int)rot_rows->size()) rot_rows->push_back(rotation[i]);
    }
    row_out[i] = r;
  }
}

int pyr_raw_queue_table(slamhip_pyramid *p, bool fma, const double *d_rot_rows, int n_rows, double base_theta,
                        const double *d_angle, int n_beams, RawTrig *out) {
  slamhip_ctx *ctx = p->ctx;
  const size_t stride = (size_t)((n_beams + 7) & ~7);
  const int rc = grow_block(ctx->stream, p->d_raw, p->raw_cap, 2 * stride * (size_t)n_rows, 1 << 14);
  if (rc) return rc;
  double *d_cos = p->d_raw.get(), *d_sin = p->d_raw.get() + stride * (size_t)n_rows;
  const auto kernel = fma ? k_pyr_raw_table<true> : k_pyr_raw_table<false>;
  SLAMHIP_CHECK(launch_kernel(kernel, raw_table_grid(n_beams, n_rows), dim3(256), 0, ctx->stream, nullptr, nullptr, d_rot_rows,
                              n_rows, base_theta, d_angle, n_beams, stride, d_cos, d_sin));
  out->cos = d_cos;
  out->sin = d_sin;
  out->row = nullptr;
  out->stride = stride;
  return SLAMHIP_OK;
}

// what every bound-scoring launch shares: the level table, the context's current scan, the base pose, the OOPE / OIE and,
// for the beam-order sum, room for n_out x scan.n terms
int pyr_fill_args(slamhip_pyramid *p, const slamhip_spe_cfg *cfg, const double base[3], size_t n_out, MatchArgs *out) {
  slamhip_ctx *ctx = p->ctx;
  if (ctx->scan_n <= 0) return pyr_state("no scan uploaded");
  MatchArgs a;
  std::memset(&a, 0, sizeof(a));
  a.levels = p->d_views.get();
  a.n_levels = p->plan.n + 1;
  const size_t c = ctx->scan_stride;
  a.scan.range = ctx->scan_ptr;
  a.scan.cos_a = ctx->scan_ptr + c;
  a.scan.sin_a = ctx->scan_ptr + 2 * c;
  a.scan.weight = ctx->scan_ptr + 3 * c;
  a.scan.factor = ctx->scan_ptr + 4 * c;
  a.scan.n = ctx->scan_n;
  a.scan.tot_w = ctx->scan_tot_w;
  for (int k = 0; k < 3; ++k) a.base[k] = base[k];
  a.oie = cfg->oie;
  a.oope = cfg->oope;
  if (cfg->sum_order == SLAMHIP_SUM_SEQUENTIAL) {
    const size_t need = n_out * (size_t)ctx->scan_n;
    const int rc = grow_block(ctx->stream, p->d_terms, p->terms_cap, need, need);  // (exactly the terms of the call)
    if (rc) return rc;
    a.terms = p->d_terms.get();
  }
  *out = a;
  return SLAMHIP_OK;
}

int pyr_launch_sum_sequential(const MatchArgs &a, size_t n_out, hipStream_t stream) {
  SLAMHIP_CHECK(launch_kernel(k_pyr_sum_sequential, dim3((unsigned)((n_out + 63) / 64)), dim3(64), 0, stream, nullptr, nullptr,
                              (const double *)a.terms, (const int *)a.level_out, (int)n_out, a.scan.n, a.scan.tot_w, a.scores));
  return SLAMHIP_OK;
}

int pyr_launch_sum_sequential_many(const ManyArgs &a, size_t n_out, int slots, hipStream_t stream) {
  SLAMHIP_CHECK(launch_kernel(k_pyr_sum_sequential_many, dim3((unsigned)((n_out + 63) / 64)), dim3(64), 0, stream, nullptr, nullptr,
                              a, (int)n_out, slots));
  return SLAMHIP_OK;
}

// ---- several requests in one launch ----------------------------------------------------------------
void pyr_many_release(slamhip_ctx *ctx) {
  delete static_cast<PyrManyStage *>(ctx->pyr_many);
  ctx->pyr_many = nullptr;
}

int pyr_source_begin(slamhip_ctx *ctx, const slamhip_spe_cfg *cfg, slamhip_pyramid *p, const slamhip_pyramid **first,
                     PyrSource *q) {
  if (!p) return pyr_invalid("a request without a pyramid");
  // (a pyramid of another context, or one that has been destroyed, is not in this context's list: it is not read)
  if (std::find(ctx->pyramids.begin(), ctx->pyramids.end(), (void *)p) == ctx->pyramids.end())
    return pyr_invalid("a request's pyramid belongs to another context, or has been destroyed");
  int rc = check_fresh(p);
  if (rc) return rc;
  if (!*first) {
    *first = p;
    rc = check_score_cfg(p, cfg);
    if (rc) return rc;
    if (cfg->pose_trig != SLAMHIP_POSE_TRIG_DEVICE && cfg->pose_trig != SLAMHIP_POSE_TRIG_HOST &&
        cfg->pose_trig != SLAMHIP_POSE_TRIG_RAW_EXACT)
      return pyr_invalid("pose_trig: DEVICE, HOST or RAW_EXACT");
    if (cfg->pose_trig == SLAMHIP_POSE_TRIG_RAW_EXACT) {
      bool fma = false;
      rc = raw_libm_build(&fma);
      if (rc) return rc;
    }
  }
  if (p->cell_model != (*first)->cell_model || p->oie != (*first)->oie)
    return pyr_invalid("the pyramids of one call share the cell model and the OIE");
  std::memset(q, 0, sizeof(*q));
  q->levels = p->d_views.get();
  q->n_levels = p->plan.n + 1;
  return SLAMHIP_OK;
}

int pyr_source_pose(const double pose[3], PyrSource *q) {
  for (int k = 0; k < 3; ++k)
    if (!std::isfinite(pose[k])) return pyr_invalid("a request's pose is not finite");
  for (int k = 0; k < 3; ++k) q->base[k] = pose[k];
  return SLAMHIP_OK;
}

void pyr_source_block(const double *d, size_t stride, int n, double tot_w, const double *d_angle, PyrSource *q) {
  q->scan = scan_view_of(d, stride, n, tot_w);
  q->angle = d_angle;
}

int pyr_many_sources(slamhip_ctx *ctx, const slamhip_spe_cfg *cfg, int n_requests, const slamhip_m3rsm_request *req,
                     std::vector<PyrSource> *out) {
  if (!ctx) return pyr_invalid("null context");
  if (n_requests < 1 || !req) return pyr_invalid("at least one request");
  out->clear();
  const slamhip_pyramid *first = nullptr;
  for (int r = 0; r < n_requests; ++r) {
    PyrSource q;
    int rc = pyr_source_begin(ctx, cfg, req[r].pyramid, &first, &q);
    if (rc) return rc;
    const int slot = req[r].scan_slot;
    if (slot < 0 || slot >= (int)ctx->scan_slots.size() || !ctx->scan_slots[slot].d || ctx->scan_slots[slot].n <= 0)
      return pyr_invalid("a request's scan slot holds no scan (slamhip_scan_store)");
    rc = pyr_source_pose(req[r].init_pose, &q);
    if (rc) return rc;
    const slamhip_ctx::ScanSlot &sl = ctx->scan_slots[slot];
    if (cfg->pose_trig == SLAMHIP_POSE_TRIG_RAW_EXACT && ((int)sl.angle.size() != sl.n || !sl.d_angle))
      return pyr_state("SLAMHIP_POSE_TRIG_RAW_EXACT needs the angles of every request's stored scan: "
                       "slamhip_scan_store_angles after slamhip_scan_store");
    pyr_source_block(sl.d.get(), (size_t)sl.cap, sl.n, sl.tot_w, cfg->pose_trig == SLAMHIP_POSE_TRIG_RAW_EXACT ? sl.d_angle.get() : nullptr,
                     &q);
    out->push_back(q);
  }
  return SLAMHIP_OK;
}

namespace {
size_t up8(size_t v) { return (v + 7) & ~(size_t)7; }
size_t many_in_bytes(size_t n_src, size_t n) {
  return up8(sizeof(PyrSource) * n_src) + sizeof(long long) * n + sizeof(double) * 7 * n + up8(sizeof(int) * n);
}
size_t many_out_bytes(size_t n_out) { return sizeof(double) * 5 * n_out + up8(sizeof(int) * n_out); }
}  // namespace

int pyr_many_stage(slamhip_ctx *ctx, const slamhip_spe_cfg *cfg, const std::vector<PyrSource> &src, int n, const int *request,
                   const double *rotation, const double *rect, int slots, ManyArgs *out, double **d_rect_out) {
  const bool raw = cfg->pose_trig == SLAMHIP_POSE_TRIG_RAW_EXACT;
  bool fma = false;
  if (raw) {
    const int rc = raw_libm_build(&fma);
    if (rc) return rc;
  }
  const size_t n_src = src.size(), n_out = (size_t)n * slots;
  if (!ctx->pyr_many) ctx->pyr_many = new PyrManyStage;
  PyrManyStage *st = static_cast<PyrManyStage *>(ctx->pyr_many);
  const size_t in_bytes = many_in_bytes(n_src, n), need = in_bytes + many_out_bytes(n_out);
  {
    const int rc = grow_blocks({ctx->stream}, st->cap, need, 1 << 16, [&](size_t cap) -> int {
      SLAMHIP_CHECK(st->d.alloc(cap));
      SLAMHIP_CHECK(st->h.alloc(cap));
      return SLAMHIP_OK;
    });
    if (rc) return rc;
  }
  const bool host_trig = cfg->pose_trig == SLAMHIP_POSE_TRIG_HOST, terms = cfg->sum_order == SLAMHIP_SUM_SEQUENTIAL;
  // table | terms offsets | rotation | rect | sin, cos | request: every part starts on 8 bytes
  size_t at = 0;
  const size_t table_at = at;
  std::memcpy(st->h.get() + at, src.data(), sizeof(PyrSource) * n_src);
  at += up8(sizeof(PyrSource) * n_src);
  const size_t off_at = at;
  long long *h_off = reinterpret_cast<long long *>(st->h.get() + at);
  size_t total_terms = 0;
  for (int i = 0; i < n; ++i) {
    h_off[i] = (long long)total_terms;
    if (terms) total_terms += (size_t)slots * (size_t)src[request[i]].scan.n;
  }
  at += sizeof(long long) * n;
  const size_t rot_at = at;
  std::memcpy(st->h.get() + at, rotation, sizeof(double) * n);
  at += sizeof(double) * n;
  const size_t rect_at = at;
  std::memcpy(st->h.get() + at, rect, sizeof(double) * 4 * n);
  at += sizeof(double) * 4 * n;
  const size_t sc_at = at;
  double *h_sc = reinterpret_cast<double *>(st->h.get() + at);
  // RAW_EXACT: the part holds the rows instead -- the distinct (request, rotation bits) pairs in order of first
  // appearance: rotation per row (at most n doubles) | request per row | row per candidate (n ints each)
  int n_rows = 0, max_beams = 0;
  if (host_trig) {  // (one sincos call per candidate / parent, on its own request's heading)
    for (int i = 0; i < n; ++i) ::sincos(rotation[i] + src[request[i]].base[2], &h_sc[2 * i], &h_sc[2 * i + 1]);
  } else if (raw) {
    int *h_row_req = reinterpret_cast<int *>(h_sc + n), *h_row = h_row_req + n;
    for (int i = 0; i < n; ++i) {
      int r = i ? h_row[i - 1] : 0;  // (neighbours mostly share request and rotation: the row before is tried first)
      if (!i || h_row_req[r] != request[i] || std::memcmp(&h_sc[r], &rotation[i], sizeof(double)) != 0) {
        for (r = 0; r < n_rows; ++r)
          if (h_row_req[r] == request[i] && std::memcmp(&h_sc[r], &rotation[i], sizeof(double)) == 0) break;
        if (r == n_rows) {
          h_sc[r] = rotation[i];
          h_row_req[r] = request[i];
          ++n_rows;
        }
      }
      h_row[i] = r;
    }
    for (const PyrSource &q : src) max_beams = std::max(max_beams, q.scan.n);
  } else {
    std::memset(h_sc, 0, sizeof(double) * 2 * n);
  }
  at += sizeof(double) * 2 * n;
  const size_t req_at = at;
  std::memcpy(st->h.get() + at, request, sizeof(int) * n);
  if (terms) {  // (exactly the terms of the call)
    const int rc = grow_block(ctx->stream, st->d_terms, st->terms_cap, total_terms, total_terms);
    if (rc) return rc;
  }
  const size_t raw_stride = (size_t)((max_beams + 7) & ~7);
  if (raw) {
    const int rc = grow_block(ctx->stream, st->d_raw, st->raw_cap, 2 * raw_stride * (size_t)n_rows, 1 << 14);
    if (rc) return rc;
  }
  SLAMHIP_CHECK(hipMemcpyAsync(st->d.get(), st->h.get(), in_bytes, hipMemcpyHostToDevice, ctx->stream));
  ManyArgs a;
  std::memset(&a, 0, sizeof(a));
  a.table = reinterpret_cast<const PyrSource *>(st->d.get() + table_at);
  if (raw) {
    const double *d_rot_rows = reinterpret_cast<const double *>(st->d.get() + sc_at);
    const int *d_row_req = reinterpret_cast<const int *>(d_rot_rows + n);
    double *d_cos = st->d_raw.get(), *d_sin = st->d_raw.get() + raw_stride * (size_t)n_rows;
    const auto kernel = fma ? k_pyr_raw_table_many<true> : k_pyr_raw_table_many<false>;
    SLAMHIP_CHECK(launch_kernel(kernel, raw_table_grid(max_beams, n_rows), dim3(256), 0, ctx->stream, nullptr, nullptr, d_rot_rows,
                                d_row_req, n_rows, a.table, raw_stride, d_cos, d_sin));
    a.m.raw.cos = d_cos;
    a.m.raw.sin = d_sin;
    a.m.raw.row = d_row_req + n;
    a.m.raw.stride = raw_stride;
  }
  a.terms_off = reinterpret_cast<const long long *>(st->d.get() + off_at);
  a.request = reinterpret_cast<const int *>(st->d.get() + req_at);
  a.m.rotation = reinterpret_cast<const double *>(st->d.get() + rot_at);
  a.m.rect = reinterpret_cast<const double *>(st->d.get() + rect_at);
  a.m.pose_sc = host_trig ? reinterpret_cast<const double *>(st->d.get() + sc_at) : nullptr;
  st->out_at = in_bytes;
  double *d_out = reinterpret_cast<double *>(st->d.get() + in_bytes);
  *d_rect_out = d_out;
  a.m.scores = d_out + 4 * n_out;
  a.m.level_out = reinterpret_cast<int *>(d_out + 5 * n_out);
  a.m.terms = terms ? st->d_terms.get() : nullptr;
  a.m.n = n;
  a.m.oie = cfg->oie;
  a.m.oope = cfg->oope;
  *out = a;
  return SLAMHIP_OK;
}

int pyr_many_fetch(slamhip_ctx *ctx, size_t n_out, bool with_rect, double *rect_out, double *score_out, int *level_out) {
  PyrManyStage *st = static_cast<PyrManyStage *>(ctx->pyr_many);
  // rect | score | level per output, as the kernels wrote them; the rectangles are skipped where nobody wrote them
  const size_t skip = with_rect ? 0 : sizeof(double) * 4 * n_out;
  SLAMHIP_CHECK(hipMemcpyAsync(st->h.get() + st->out_at + skip, st->d.get() + st->out_at + skip, many_out_bytes(n_out) - skip,
                               hipMemcpyDeviceToHost, ctx->stream));
  SLAMHIP_CHECK(hipStreamSynchronize(ctx->stream));
  const double *h_out = reinterpret_cast<const double *>(st->h.get() + st->out_at);
  if (with_rect) std::memcpy(rect_out, h_out, sizeof(double) * 4 * n_out);
  std::memcpy(score_out, h_out + 4 * n_out, sizeof(double) * n_out);
  std::memcpy(level_out, h_out + 5 * n_out, sizeof(int) * n_out);
  return SLAMHIP_OK;
}

void pyr_free_staging(slamhip_pyramid *p) { static_cast<slamhip_pyramid_staging &>(*p) = slamhip_pyramid_staging(); }

// slamhip_pyramid_refresh_batch's job tables, kept by the context: one block in HBM and two pinned ones taking turns.
// The call does not wait, so the copy of a table may still be pending when the next call fills one: a pinned block is
// written only after the event behind its last copy has passed (the block in HBM is rewritten in stream order, behind
// the kernels that read it).
struct PyrRefreshStage {
  PinnedBuf<char> h[2];
  DeviceBuf<char> d;
  hipEvent_t copied[2] = {nullptr, nullptr};
  bool pending[2] = {false, false};
  size_t cap = 0;
  int turn = 0;
  pyr_plan::Plan plan;  // of the last call that was not refused
};

static void pyr_refresh_release(slamhip_ctx *ctx) {
  PyrRefreshStage *st = static_cast<PyrRefreshStage *>(ctx->pyr_refresh);
  if (!st) return;
  (void)hipStreamSynchronize(ctx->stream);
  for (int k = 0; k < 2; ++k)
    if (st->copied[k]) (void)hipEventDestroy(st->copied[k]);
  delete st;
  ctx->pyr_refresh = nullptr;
}

void pyramids_release(slamhip_ctx *ctx) {
  pyr_refresh_release(ctx);
  for (void *v : ctx->pyramids) {
    slamhip_pyramid *p = static_cast<slamhip_pyramid *>(v);
    free_levels(p, false);  // (the context frees its maps itself)
    pyr_free_staging(p);
    p->ctx = nullptr;
  }
  ctx->pyramids.clear();
  pyr_many_release(ctx);
}

}  // namespace slamhip

using namespace slamhip;

int slamhip_pyramid_create(slamhip_ctx *ctx, int fine_map_id, int oie, int first_level_map_id, slamhip_pyramid **out) {
  if (!ctx || !out) return pyr_invalid("null context or output");
  *out = nullptr;
  SLAMHIP_CHECK(hipSetDevice(ctx->device));
  slamhip_pyramid *p = new slamhip_pyramid;
  p->ctx = ctx;
  p->fine_id = fine_map_id;
  p->first_id = first_level_map_id;
  p->oie = oie;
  const int rc = make_levels(p);
  if (rc) {
    free_levels(p, true);
    delete p;
    return rc;
  }
  ctx->pyramids.push_back(p);
  *out = p;
  return SLAMHIP_OK;
}

int slamhip_pyramid_destroy(slamhip_pyramid *p) {
  if (!p) return SLAMHIP_OK;
  if (p->ctx) {
    slamhip_ctx *ctx = p->ctx;
    free_levels(p, true);
    pyr_free_staging(p);
    ctx->pyramids.erase(std::remove(ctx->pyramids.begin(), ctx->pyramids.end(), (void *)p), ctx->pyramids.end());
  }
  delete p;
  return SLAMHIP_OK;
}

int slamhip_pyramid_info(slamhip_pyramid *p, int *n_levels, int cap, int *map_id, int *width, int *height, int *origin_x,
                         int *origin_y, double *scale) {
  if (!p || !p->ctx) return pyr_invalid("null pyramid, or one whose context has been destroyed");
  if (cap < 0) return pyr_invalid("negative capacity");
  if (n_levels) *n_levels = p->plan.n;
  for (int k = 0; k < std::min(cap, p->plan.n); ++k) {
    if (map_id) map_id[k] = p->first_id + k;
    if (width) width[k] = p->plan.width[k];
    if (height) height[k] = p->plan.height[k];
    if (origin_x) origin_x[k] = p->plan.origin_x[k];
    if (origin_y) origin_y[k] = p->plan.origin_y[k];
    if (scale) scale[k] = p->plan.scale[k];
  }
  return SLAMHIP_OK;
}

int slamhip_pyramid_rebuild(slamhip_pyramid *p) {
  if (!p || !p->ctx) return pyr_invalid("null pyramid, or one whose context has been destroyed");
  SLAMHIP_CHECK(hipSetDevice(p->ctx->device));
  if (check_fresh(p) == SLAMHIP_OK) return queue_levels(p, 0, 0, p->fine_w, p->fine_h);
  // the fine map has moved or grown: the levels are planned and bound anew under the same ids
  free_levels(p, true);
  const int rc = make_levels(p);
  if (rc) free_levels(p, true);
  else set_error("");  // (check_fresh's finding has been dealt with)
  return rc;
}

int slamhip_pyramid_refresh(slamhip_pyramid *p, int x0, int y0, int w, int h) {
  int rc = check_fresh(p);
  if (rc) return rc;
  if (w <= 0 || h <= 0 || x0 < 0 || y0 < 0 || (long long)x0 + w > p->fine_w || (long long)y0 + h > p->fine_h)
    return pyr_invalid("window outside the fine map");
  SLAMHIP_CHECK(hipSetDevice(p->ctx->device));
  return queue_levels(p, x0, y0, w, h);
}

int slamhip_pyramid_refresh_batch(slamhip_ctx *ctx, int n_jobs, const slamhip_pyramid_refresh_job *jobs) {
  if (!ctx) return pyr_invalid("null context");
  if (n_jobs < 0) return pyr_invalid("negative job count");
  if (n_jobs == 0) return SLAMHIP_OK;
  if (!jobs) return pyr_invalid("null jobs");
  // every refusal first: nothing is queued and the last call's plan stays
  std::vector<pyr_plan::Job> pj(n_jobs);
  std::vector<std::vector<pyr_plan::LevelGeom>> geom(n_jobs);
  for (int k = 0; k < n_jobs; ++k) {
    slamhip_pyramid *p = jobs[k].pyramid;
    if (!p) return pyr_invalid("a job without a pyramid");
    const auto at = std::find(ctx->pyramids.begin(), ctx->pyramids.end(), (void *)p);
    if (at == ctx->pyramids.end()) return pyr_invalid("a job's pyramid belongs to another context, or has been destroyed");
    const int rc = check_fresh(p);
    if (rc) return rc;
    pyr_plan::Job &j = pj[k];
    j.pyramid = (int)(at - ctx->pyramids.begin());
    j.n_levels = p->plan.n;
    geom[k].resize(p->plan.n);
    j.lone = false;
    for (int lv = 1; lv <= p->plan.n; ++lv) {
      geom[k][lv - 1] = pyr_plan::LevelGeom{p->plan.width[lv - 1], p->plan.height[lv - 1], p->plan.origin_x[lv - 1],
                                            p->plan.origin_y[lv - 1]};
      if (ctx->maps[p->first_id + lv - 1].prob_ok) j.lone = true;  // (its probability plane follows its cells: queue_levels)
    }
    j.levels = geom[k].data();
    j.fine_w = p->fine_w;
    j.fine_h = p->fine_h;
    j.fine_ox = p->fine_ox;
    j.fine_oy = p->fine_oy;
    j.x0 = jobs[k].x0;
    j.y0 = jobs[k].y0;
    j.w = jobs[k].w;
    j.h = jobs[k].h;
    j.stale = false;
  }
  pyr_plan::Plan plan;
  switch (pyr_plan::plan_call(pj, sizeof(PyrReduceEntry), &plan)) {
    case pyr_plan::kOk: break;
    case pyr_plan::kWindow: return pyr_invalid("a job's window is outside its fine map");
    case pyr_plan::kTooLarge: return pyr_invalid("the batch needs more than 2^31 workgroups in one launch: split it");
    default: return pyr_state("a job's pyramid is stale: slamhip_pyramid_rebuild");
  }
  SLAMHIP_CHECK(hipSetDevice(ctx->device));
  if (!ctx->pyr_refresh) ctx->pyr_refresh = new PyrRefreshStage;
  PyrRefreshStage *st = static_cast<PyrRefreshStage *>(ctx->pyr_refresh);
  for (int k = 0; k < 2; ++k)
    if (!st->copied[k]) SLAMHIP_CHECK(hipEventCreateWithFlags(&st->copied[k], hipEventDisableTiming));
  {
    const int rc = grow_blocks({ctx->stream}, st->cap, plan.table_bytes, 1 << 14, [&](size_t cap) -> int {
      st->pending[0] = st->pending[1] = false;  // (the stream has been waited for)
      SLAMHIP_CHECK(st->d.alloc(cap));
      for (int k = 0; k < 2; ++k) SLAMHIP_CHECK(st->h[k].alloc(cap));
      return SLAMHIP_OK;
    });
    if (rc) return rc;
  }
  const PyrReduceEntry *d_entries = reinterpret_cast<const PyrReduceEntry *>(st->d.get());
  const unsigned *d_off = reinterpret_cast<const unsigned *>(st->d.get() + plan.off_bytes_at);
  const int *d_runs = reinterpret_cast<const int *>(st->d.get() + plan.run_bytes_at);
  if (plan.table_bytes) {
    const int turn = st->turn;
    st->turn ^= 1;
    if (st->pending[turn]) {
      SLAMHIP_CHECK(hipEventSynchronize(st->copied[turn]));
      st->pending[turn] = false;
    }
    char *h = st->h[turn].get();
    std::memset(h, 0, plan.table_bytes);
    PyrReduceEntry *h_entries = reinterpret_cast<PyrReduceEntry *>(h);
    for (size_t i = 0; i < plan.entries.size(); ++i) {
      const pyr_plan::EntryRef &r = plan.entries[i];
      const slamhip_pyramid *p = jobs[r.job].pyramid;
      const int lv = r.level;
      const DeviceMap &src = ctx->maps[lv == 1 ? p->fine_id : p->first_id + lv - 2];
      const DeviceMap &dst = ctx->maps[p->first_id + lv - 1];
      const bool top = lv == p->plan.n;
      PyrReduceEntry &e = h_entries[i];
      e.src = level_of(src, lv == 1 ? nullptr : p->d_coord[lv - 2].get());
      e.dst = level_of(dst, p->d_coord[lv - 1].get());
      e.bias_x = top ? 0 : src.origin_x - 2 * dst.origin_x;
      e.bias_y = top ? 0 : src.origin_y - 2 * dst.origin_y;
      e.cx0 = r.win.cx0;
      e.cy0 = r.win.cy0;
      e.cw = r.win.cw;
      e.ch = r.win.ch;
      e.model = p->cell_model;
      e.oie = p->oie;
      e.cd = cell_doubles(p->cell_model) == 1 ? 1 : 4;
      for (int k = 0; k < 4; ++k) e.unknown[k] = dst.unknown[k];
    }
    unsigned *h_off = reinterpret_cast<unsigned *>(h + plan.off_bytes_at);
    int *h_runs = reinterpret_cast<int *>(h + plan.run_bytes_at);
    for (const pyr_plan::Step &s : plan.steps) {
      for (const pyr_plan::FlatLaunch &f : s.flat) std::copy(f.block_off.begin(), f.block_off.end(), h_off + f.off_at);
      for (size_t k = 0; k < s.tail.size(); ++k) {
        h_runs[2 * (s.run_at + k)] = (int)s.tail[k].entry_at;
        h_runs[2 * (s.run_at + k) + 1] = s.tail[k].n_entries;
      }
    }
    SLAMHIP_CHECK(hipMemcpyAsync(st->d.get(), h, plan.table_bytes, hipMemcpyHostToDevice, ctx->stream));
    SLAMHIP_CHECK(hipEventRecord(st->copied[turn], ctx->stream));
    st->pending[turn] = true;
  }
  st->plan = plan;
  st->plan.stats.launches = 0;  // (counted as they are queued)
  for (const pyr_plan::Step &s : plan.steps) {
    if (s.lone) {
      const slamhip_pyramid_refresh_job &jb = jobs[s.jobs[0]];
      const int rc = queue_levels(jb.pyramid, jb.x0, jb.y0, jb.w, jb.h);
      if (rc) return rc;
      continue;
    }
    ProfilePairGuard prof;  // (while profiling is on: a round's kernels, first to last, in kernel_ms_total)
    int rc = prof.open(ctx, ctx->stream, 0);
    if (rc) return rc;
    for (const pyr_plan::FlatLaunch &f : s.flat) {
      SLAMHIP_CHECK(launch_kernel(k_pyr_reduce_batch, dim3(f.block_off.back()), dim3(kPyrThreads), 0, ctx->stream, nullptr, nullptr,
                                  d_entries + f.entry_at, d_off + f.off_at, (int)f.jobs.size()));
      st->plan.stats.launches += 1;
    }
    SLAMHIP_CHECK(launch_kernel(k_pyr_reduce_tail, dim3((unsigned)s.tail.size()), dim3(kPyrThreads), 0, ctx->stream, nullptr,
                                nullptr, d_entries, d_runs + 2 * s.run_at));
    st->plan.stats.launches += 1;
    rc = prof.close();
    if (rc) return rc;
    if (ctx->profile) ctx->prof_launches += 1;
  }
  return SLAMHIP_OK;
}

int slamhip_pyramid_refresh_batch_stats(slamhip_ctx *ctx, int *rounds, int *jobs_in_shared_launches, int *jobs_lone,
                                        int *launches) {
  if (!ctx) return pyr_invalid("null context");
  const PyrRefreshStage *st = static_cast<const PyrRefreshStage *>(ctx->pyr_refresh);
  const pyr_plan::Stats s = st ? st->plan.stats : pyr_plan::Stats{};
  if (rounds) *rounds = s.rounds;
  if (jobs_in_shared_launches) *jobs_in_shared_launches = s.jobs_shared;
  if (jobs_lone) *jobs_lone = s.jobs_lone;
  if (launches) *launches = s.launches;
  return SLAMHIP_OK;
}

int slamhip_pyramid_score_matches_device(slamhip_ctx *ctx, slamhip_pyramid *p, const slamhip_spe_cfg *cfg,
                                         const double base_pose[3], int n, const double *d_rotation, const double *d_rect,
                                         double *d_score_out, int *d_level_out) {
  int rc = check_fresh(p);
  if (rc) return rc;
  if (ctx != p->ctx) return pyr_invalid("the pyramid belongs to another context");
  rc = check_score_cfg(p, cfg);
  if (rc) return rc;
  if (n < 0 || !base_pose) return pyr_invalid("bad candidate batch");
  if (n == 0) return SLAMHIP_OK;
  if (!d_rotation || !d_rect || !d_score_out || !d_level_out) return pyr_invalid("null device buffers");
  const bool raw = cfg->pose_trig == SLAMHIP_POSE_TRIG_RAW_EXACT;
  if (cfg->pose_trig != SLAMHIP_POSE_TRIG_DEVICE && !raw)
    return pyr_invalid("device-resident candidates use device sincos (pose_trig = DEVICE) or RAW_EXACT: the host-trig mode "
                       "takes host arrays");
  for (int k = 0; k < 3; ++k)
    if (!std::isfinite(base_pose[k])) return pyr_invalid("the base pose is not finite");
  SLAMHIP_CHECK(hipSetDevice(ctx->device));
  RawTrig rt{};
  if (raw) {
    // (the host does not see the rotations: every candidate is a row of its own, row i for candidate i)
    bool fma = false;
    const double *d_angle = nullptr;
    rc = pyr_raw_prepare(ctx, &fma, &d_angle);
    if (rc) return rc;
    rc = pyr_raw_queue_table(p, fma, d_rotation, n, base_pose[2], d_angle, ctx->scan_n, &rt);
    if (rc) return rc;
  }
  return queue_score(p, cfg, base_pose, n, d_rotation, d_rect, nullptr, raw ? &rt : nullptr, d_score_out, d_level_out);
}

int slamhip_pyramid_score_matches(slamhip_ctx *ctx, slamhip_pyramid *p, const slamhip_spe_cfg *cfg, const double base_pose[3],
                                  int n, const double *rotation, const double *rect, double *score_out, int *level_out) {
  int rc = check_fresh(p);
  if (rc) return rc;
  if (ctx != p->ctx) return pyr_invalid("the pyramid belongs to another context");
  rc = check_score_cfg(p, cfg);
  if (rc) return rc;
  if (n < 0 || !base_pose) return pyr_invalid("bad candidate batch");
  if (n == 0) return SLAMHIP_OK;
  if (!rotation || !rect || !score_out || !level_out) return pyr_invalid("null candidate arrays");
  const bool raw = cfg->pose_trig == SLAMHIP_POSE_TRIG_RAW_EXACT;
  if (cfg->pose_trig != SLAMHIP_POSE_TRIG_DEVICE && cfg->pose_trig != SLAMHIP_POSE_TRIG_HOST && !raw)
    return pyr_invalid("pose_trig: DEVICE, HOST or RAW_EXACT");
  for (int k = 0; k < 3; ++k)
    if (!std::isfinite(base_pose[k])) return pyr_invalid("the base pose is not finite");
  for (int i = 0; i < n; ++i) {
    const double *r = rect + 4 * (size_t)i;
    if (!std::isfinite(rotation[i]) || !std::isfinite(r[0]) || !std::isfinite(r[1]) || !std::isfinite(r[2]) ||
        !std::isfinite(r[3]) || !(r[0] <= r[1] && r[2] <= r[3]))
      return pyr_invalid("a candidate's rotation or rectangle is not finite, or not bot <= top and left <= right");
    // (the rule of cfg->area -- at most 10^4 cells per beam -- holds by construction: the rectangle is at most one
    // cell of its level wide, so a beam's window is at most 3 x 3 cells)
  }
  SLAMHIP_CHECK(hipSetDevice(ctx->device));
  bool fma = false;
  const double *d_angle = nullptr;
  if (raw) {  // (before anything is queued)
    rc = pyr_raw_prepare(ctx, &fma, &d_angle);
    if (rc) return rc;
  }
  rc = grow_blocks({ctx->stream}, p->in_cap, (size_t)n, 256, [&](size_t cap) -> int {
    SLAMHIP_CHECK(p->d_in.alloc(7 * cap));
    SLAMHIP_CHECK(p->d_scores.alloc(cap));
    SLAMHIP_CHECK(p->d_levels.alloc(cap));
    return SLAMHIP_OK;
  });
  if (rc) return rc;
  const bool host_trig = cfg->pose_trig == SLAMHIP_POSE_TRIG_HOST;
  std::vector<double> stage((size_t)n * 7);
  std::memcpy(stage.data(), rotation, sizeof(double) * n);
  std::memcpy(stage.data() + n, rect, sizeof(double) * 4 * n);
  if (host_trig)  // (one sincos call per pose, as slamhip_score_poses' host mode makes it)
    for (int i = 0; i < n; ++i) ::sincos(rotation[i] + base_pose[2], &stage[5 * (size_t)n + 2 * i], &stage[5 * (size_t)n + 2 * i + 1]);
  // RAW_EXACT: the (sin, cos) part holds the rows' rotations (at most n doubles) and, behind them, a row per candidate
  std::vector<double> rot_rows;
  if (raw) {
    pyr_raw_rows(n, rotation, reinterpret_cast<int *>(stage.data() + 6 * (size_t)n), &rot_rows);
    std::memcpy(stage.data() + 5 * (size_t)n, rot_rows.data(), sizeof(double) * rot_rows.size());
  }
  SLAMHIP_CHECK(hipMemcpyAsync(p->d_in.get(), stage.data(), sizeof(double) * (host_trig || raw ? 7 : 5) * n, hipMemcpyHostToDevice,
                               ctx->stream));
  RawTrig rt{};
  if (raw) {
    rc = pyr_raw_queue_table(p, fma, p->d_in.get() + 5 * (size_t)n, (int)rot_rows.size(), base_pose[2], d_angle, ctx->scan_n, &rt);
    if (rc) return rc;
    rt.row = reinterpret_cast<const int *>(p->d_in.get() + 6 * (size_t)n);
  }
  rc = queue_score(p, cfg, base_pose, n, p->d_in.get(), p->d_in.get() + n, host_trig ? p->d_in.get() + 5 * (size_t)n : nullptr,
                   raw ? &rt : nullptr, p->d_scores.get(), p->d_levels.get());
  if (rc) return rc;
  SLAMHIP_CHECK(hipMemcpyAsync(score_out, p->d_scores.get(), sizeof(double) * n, hipMemcpyDeviceToHost, ctx->stream));
  SLAMHIP_CHECK(hipMemcpyAsync(level_out, p->d_levels.get(), sizeof(int) * n, hipMemcpyDeviceToHost, ctx->stream));
  SLAMHIP_CHECK(hipStreamSynchronize(ctx->stream));
  return SLAMHIP_OK;
}

namespace slamhip {
// what both multi-request entry points check of their candidates
int pyr_many_check_batch(int n_requests, int n, const int *request, const double *rotation, const double *rect, bool reversed_ok) {
  if (!request || !rotation || !rect) return pyr_invalid("null candidate arrays");
  for (int i = 0; i < n; ++i) {
    const double *r = rect + 4 * (size_t)i;
    if (request[i] < 0 || request[i] >= n_requests) return pyr_invalid("a candidate's request is not in the table");
    if (!std::isfinite(rotation[i]) || !std::isfinite(r[0]) || !std::isfinite(r[1]) || !std::isfinite(r[2]) || !std::isfinite(r[3]))
      return pyr_invalid("a candidate's rotation or rectangle is not finite");
    if (!reversed_ok && !(r[0] <= r[1] && r[2] <= r[3])) return pyr_invalid("a candidate's rectangle: not bot <= top and left <= right");
  }
  return SLAMHIP_OK;
}
}  // namespace slamhip

int slamhip_pyramid_score_requests(slamhip_ctx *ctx, const slamhip_spe_cfg *cfg, int n_requests,
                                   const slamhip_m3rsm_request *table, int n, const int *request, const double *rotation,
                                   const double *rect, double *score_out, int *level_out) {
  std::vector<PyrSource> src;
  const int rc = pyr_many_sources(ctx, cfg, n_requests, table, &src);
  if (rc) return rc;
  return pyr_score_sources(ctx, cfg, src, table[0].pyramid->cell_model, n, request, rotation, rect, score_out, level_out);
}

int slamhip::pyr_score_sources(slamhip_ctx *ctx, const slamhip_spe_cfg *cfg, const std::vector<PyrSource> &src, int cell_model,
                               int n, const int *request, const double *rotation, const double *rect, double *score_out,
                               int *level_out) {
  const int n_requests = (int)src.size();
  int rc = SLAMHIP_OK;
  if (n < 0) return pyr_invalid("bad candidate batch");
  if (n == 0) return SLAMHIP_OK;
  if (!score_out || !level_out) return pyr_invalid("null output arrays");
  rc = pyr_many_check_batch(n_requests, n, request, rotation, rect, false);
  if (rc) return rc;
  SLAMHIP_CHECK(hipSetDevice(ctx->device));
  ManyArgs a;
  double *d_rect_out = nullptr;
  rc = pyr_many_stage(ctx, cfg, src, n, request, rotation, rect, 1, &a, &d_rect_out);
  if (rc) return rc;
  ProfilePairGuard prof;
  rc = prof.open(ctx, ctx->stream, 0);
  if (rc) return rc;
  typedef void (*Kernel)(ManyArgs);
  const bool raw = a.m.raw.cos != nullptr;
  const Kernel kernel = pick_cell_model(cell_model, [raw](auto m) -> Kernel {
    return raw ? k_pyr_score_many<decltype(m)::value, true> : k_pyr_score_many<decltype(m)::value, false>;
  });
  SLAMHIP_CHECK(launch_kernel(kernel, dim3(n), dim3(kPyrThreads), 0, ctx->stream, nullptr, nullptr, a));
  if (a.m.terms) {
    rc = pyr_launch_sum_sequential_many(a, (size_t)n, 1, ctx->stream);
    if (rc) return rc;
  }
  rc = prof.close();
  if (rc) return rc;
  if (ctx->profile) {
    ctx->prof_launches += 1;
    for (int i = 0; i < n; ++i) ctx->prof_units += src[request[i]].scan.n;
  }
  return pyr_many_fetch(ctx, (size_t)n, false, nullptr, score_out, level_out);
}

int slamhip_pyramid_build_host(int cell_model, int oie, int width, int height, int origin_x, int origin_y, double scale,
                               const double *unknown_payload, const double *payload, int level_cap, int *n_levels,
                               int *level_width, int *level_height, int *level_origin_x, int *level_origin_y,
                               double *level_scale, size_t payload_cap, double *payload_out, size_t *payload_need) {
  if (cell_model != SLAMHIP_CELL_OCC && !cell_is_belief(cell_model))
    return pyr_invalid("a pyramid stands over OCC, TBM or CREDIBILIST cells");
  if (!pyr::check_oie(cell_model, oie))
    return pyr_invalid("unknown OIE, or OccupancyOIE over belief cells (they are scored under the discrepancy OIE only)");
  if (!(scale > 0) || !unknown_payload || !payload || level_cap < 0 || !n_levels) return pyr_invalid("bad arguments");
  pyr::Plan pl;
  if (!pyr::plan_levels(width, height, origin_x, origin_y, scale, &pl)) return pyr_invalid("bad map geometry");
  const int cd = cell_stride_host(cell_model);  // (OCC 1, beliefs 4: the stride in HBM too)
  *n_levels = pl.n;
  size_t need = 0;
  for (int k = 0; k < pl.n; ++k) need += (size_t)pl.width[k] * pl.height[k] * cd;
  if (payload_need) *payload_need = need;
  for (int k = 0; k < std::min(level_cap, pl.n); ++k) {
    if (level_width) level_width[k] = pl.width[k];
    if (level_height) level_height[k] = pl.height[k];
    if (level_origin_x) level_origin_x[k] = pl.origin_x[k];
    if (level_origin_y) level_origin_y[k] = pl.origin_y[k];
    if (level_scale) level_scale[k] = pl.scale[k];
  }
  if (!payload_out) return SLAMHIP_OK;  // geometry only
  if (payload_cap < need) return pyr_invalid("payload_out is too small (payload_need says how many doubles)");
  double unknown[4] = {0, 0, 0, 0};
  for (int k = 0; k < cd; ++k) unknown[k] = unknown_payload[k];
  std::vector<std::vector<int>> coord(pl.n);
  pyr::Level src{const_cast<double *>(payload), nullptr, width, height, width, origin_x, origin_y};
  double *at = payload_out;
  for (int lv = 1; lv <= pl.n; ++lv) {
    const int w = pl.width[lv - 1], h = pl.height[lv - 1];
    coord[lv - 1].assign((size_t)2 * w * h, 0);
    pyr::Level dst{at, coord[lv - 1].data(), w, h, w, pl.origin_x[lv - 1], pl.origin_y[lv - 1]};
    const bool top = lv == pl.n;
    const int bias_x = top ? 0 : src.origin_x - 2 * dst.origin_x, bias_y = top ? 0 : src.origin_y - 2 * dst.origin_y;
    for (int iy = 0; iy < h; ++iy)
      for (int ix = 0; ix < w; ++ix) {
        if (cd == 1) pyr::reduce_cell<1>(src, dst, bias_x, bias_y, cell_model, oie, unknown, ix, iy);
        else pyr::reduce_cell<4>(src, dst, bias_x, bias_y, cell_model, oie, unknown, ix, iy);
      }
    src = dst;
    at += (size_t)w * h * cd;
  }
  return SLAMHIP_OK;
}
