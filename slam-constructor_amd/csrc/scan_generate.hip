// scan_generate.hip -- laser scans ray-cast from a resident map (include/slamhip.h "scan generation").
//
// LaserScanGenerator::laser_scan_2D (src/utils/data_generation/laser_scan_generator.h:35-80) walks every beam's cells
// through a std::vector, a virtual operator[] and a heap-allocated intersection list -- up to ~1400 cells per beam for
// the evaluator's to_lsp(100, 270, 1000) at 0.1 m.  Here K poses x B angles are one launch over the map where it lives;
// the per-beam routine is scan_generate_device.h, shared with the host entry at the bottom.
//
// Wave form (k_scan_generate_wave), one wave per beam, one lane per walk step, 64 steps a round: lane k evaluates its
// cell from the closed form of the walk and checks the step the recurrence would take from it, exactly as
// mu_walk_beam_wave does (map_update_kernels.h) -- pieces between ties, a step classified only when it is clear of the
// tie tolerance.  While no hit has been accepted, each lane that stands on a cell of the walk loads that cell's occupancy
// (8 bytes; 32-byte cells: the 24 bytes of u, e, o), a ballot finds the first cell that is not below the threshold, that
// lane intersects the ray with the cell, and a touch clears its bit.  After the accepted hit nothing is loaded any more,
// but the rounds go on until a lane stands on the END CELL: only then is the walk known to be the reference's list and
// the hit written.  Whatever the closed form does not settle -- an unclassifiable step, more than eight ties, a walk
// that does not arrive within cells_nm cells (the reference's Bresenham list) -- is redone by lane 0 with the
// sequential routine, hit included: nothing of an unproven walk is kept.
// Sequential form (k_scan_generate_seq): one thread per beam runs sg_beam_sequential; SLAMHIP_SCAN_GEN_SEQUENTIAL
// forces it for every beam.
// Per-particle maps (k_scan_generate_tiled_wave / _seq, slamhip_gmapping_particle_generate_scans): the same two kernels
// over the slots of a tile pool -- the per-beam routines take the map as a template parameter and read it through
// sg_cell_occ alone, which for an SgTiledMap is the renderer's read (table entry, then the cell's prob_occ); job = (slot,
// pose), all jobs in one launch.
// No LDS, no atomics; results leave as one block (ranges, then status bytes) in one copy.
#include <algorithm>
#include <cstring>
#include <vector>

#include "scan_generate_device.h"
#include "tile_pool.h"

namespace slamhip {
namespace {

using namespace sg;

constexpr int kSgThreads = 256;

__device__ __forceinline__ double sg_readlane(double v, int lane) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane), hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
}

// false: nothing is decided, the caller runs the sequential routine
template <class Map>
__device__ bool sg_beam_wave(const Map &m, const SgBeam &b, double thr, int lane, int *status_out, double *range_out) {
  const SgWalkLine L = sg_walk_line(b);
  const int steps_x = abs(b.ex - b.bx), steps_y = abs(b.ey - b.by);
  const unsigned cap = (unsigned)steps_x + (unsigned)steps_y + 1u;
  if (!sg_wave_applies(L, cap)) return false;  // (a beam that ends where it starts; one too long for the margin)
  SgPiece pc{0u, 0, 0, L.e0, L.q0};
  int ties = 0;
  bool found = false;
  int status = SG_NONE;
  double range = 0.0;
  for (unsigned k0 = 0u;;) {
    int i, j;
    const int cls = sg_wave_classify(L, pc, k0 + (unsigned)lane, cap, steps_x, steps_y, &i, &j);
    const unsigned long long ev = __ballot(cls != 0);
    const int first = ev ? __ffsll((long long)ev) - 1 : 64;
    const int fcls = first < 64 ? __builtin_amdgcn_readlane(cls, first) : 0;
    if (fcls == 3 || fcls == 4) return false;
    if (!found) {
      // (lane `first` stands on the end cell or on the cell the tie is decided from: a cell of the walk)
      const int cx = b.bx + L.inc_x * i, cy = b.by + L.inc_y * j;
      bool cand = false;
      if (lane <= first) cand = !(sg_cell_occ(m, cx, cy) < thr);
      unsigned long long mask = __ballot(cand);
      while (mask) {
        const int f = __ffsll((long long)mask) - 1;
        int r = SG_NONE;
        double rg = 0.0;
        if (lane == f) r = sg_test_cell(b, cx, cy, &rg);
        r = __builtin_amdgcn_readlane(r, f);
        if (r == SG_TOUCH) {
          mask &= mask - 1ull;
          continue;
        }
        found = true;
        status = r;
        range = r == SG_HIT ? sg_readlane(rg, f) : 0.0;
        break;
      }
    }
    if (first == 64) {
      k0 += 64u;
      continue;
    }
    if (fcls == 1) break;  // arrived: the cells seen so far are the reference's list
    // a tie at walk index k0 + first
    if (++ties > kSgMaxTies) return false;
    pc = sg_wave_after_tie(L, __builtin_amdgcn_readlane(i, first), __builtin_amdgcn_readlane(j, first), k0 + (unsigned)first,
                           steps_x, steps_y);
    k0 = pc.k_base;
  }
  *status_out = status;
  *range_out = range;
  return true;
}

template <bool FMA>
__global__ __launch_bounds__(kSgThreads) void k_scan_generate_wave(SgMap m, const double *__restrict__ poses, int n_angles,
                                                                   const double *__restrict__ angles, int n_beams,
                                                                   double max_dist, double thr, double *__restrict__ range_out,
                                                                   unsigned char *__restrict__ status_out) {
  const int g = blockIdx.x * (kSgThreads / 64) + (threadIdx.x >> 6);
  if (g >= n_beams) return;  // (the same for the whole wave)
  const int lane = threadIdx.x & 63;
  const int p = g / n_angles, ai = g - p * n_angles;
  const SgBeam b = sg_beam_setup<FMA>(poses[3 * p], poses[3 * p + 1], poses[3 * p + 2], angles[ai], max_dist, m.scale);
  int status = SG_NONE;
  double range = 0.0;
  if (!sg_beam_wave(m, b, thr, lane, &status, &range)) {
    if (lane == 0) status = sg_beam_sequential(m, b, thr, &range);
  }
  if (lane == 0) {
    range_out[g] = range;
    status_out[g] = (unsigned char)status;
  }
}

template <bool FMA>
__global__ __launch_bounds__(kSgThreads) void k_scan_generate_seq(SgMap m, const double *__restrict__ poses, int n_angles,
                                                                  const double *__restrict__ angles, int n_beams,
                                                                  double max_dist, double thr, double *__restrict__ range_out,
                                                                  unsigned char *__restrict__ status_out) {
  const int g = blockIdx.x * kSgThreads + threadIdx.x;
  if (g >= n_beams) return;
  const int p = g / n_angles, ai = g - p * n_angles;
  const SgBeam b = sg_beam_setup<FMA>(poses[3 * p], poses[3 * p + 1], poses[3 * p + 2], angles[ai], max_dist, m.scale);
  double range = 0.0;
  const int status = sg_beam_sequential(m, b, thr, &range);
  range_out[g] = range;
  status_out[g] = (unsigned char)status;
}

// The same two kernels over the slots of a tile pool (tile_pool.h): job p = beam g / n_angles reads pose p through the
// table of slot slots[p].  m.table is the pool's table block here, table_stride ints per slot.
template <bool FMA>
__global__ __launch_bounds__(kSgThreads) void k_scan_generate_tiled_wave(SgTiledMap m, int table_stride,
                                                                         const int *__restrict__ slots,
                                                                         const double *__restrict__ poses, int n_angles,
                                                                         const double *__restrict__ angles, int n_beams,
                                                                         double max_dist, double thr,
                                                                         double *__restrict__ range_out,
                                                                         unsigned char *__restrict__ status_out) {
  const int g = blockIdx.x * (kSgThreads / 64) + (threadIdx.x >> 6);
  if (g >= n_beams) return;  // (the same for the whole wave)
  const int lane = threadIdx.x & 63;
  const int p = g / n_angles, ai = g - p * n_angles;
  m.table += (size_t)slots[p] * table_stride;
  const SgBeam b = sg_beam_setup<FMA>(poses[3 * p], poses[3 * p + 1], poses[3 * p + 2], angles[ai], max_dist, m.scale);
  int status = SG_NONE;
  double range = 0.0;
  if (!sg_beam_wave(m, b, thr, lane, &status, &range)) {
    if (lane == 0) status = sg_beam_sequential(m, b, thr, &range);
  }
  if (lane == 0) {
    range_out[g] = range;
    status_out[g] = (unsigned char)status;
  }
}

template <bool FMA>
__global__ __launch_bounds__(kSgThreads) void k_scan_generate_tiled_seq(SgTiledMap m, int table_stride,
                                                                        const int *__restrict__ slots,
                                                                        const double *__restrict__ poses, int n_angles,
                                                                        const double *__restrict__ angles, int n_beams,
                                                                        double max_dist, double thr,
                                                                        double *__restrict__ range_out,
                                                                        unsigned char *__restrict__ status_out) {
  const int g = blockIdx.x * kSgThreads + threadIdx.x;
  if (g >= n_beams) return;
  const int p = g / n_angles, ai = g - p * n_angles;
  m.table += (size_t)slots[p] * table_stride;
  const SgBeam b = sg_beam_setup<FMA>(poses[3 * p], poses[3 * p + 1], poses[3 * p + 2], angles[ai], max_dist, m.scale);
  double range = 0.0;
  const int status = sg_beam_sequential(m, b, thr, &range);
  range_out[g] = range;
  status_out[g] = (unsigned char)status;
}

int sg_invalid(const char *msg) {
  set_error(msg);
  return SLAMHIP_ERR_INVALID;
}

constexpr int kSgMaxBeams = 1 << 26;

// the checks the device entry and the host entry share; null = fine
const char *sg_check_call(int model, int occ_kind, int variant, int n_poses, const double *poses_xyt, int n_angles,
                          const double *angles, const double *range_out, const unsigned char *status_out) {
  if (!occ_kind_ok(model, occ_kind)) return "occ_kind names a TBM cell class: 0 or 1 on a TBM map, 0 on every other";
  if (variant != 0 && variant != 1) return "variant: 0 = glibc's plain build of sin / cos, 1 = its FMA build";
  if (n_poses < 0 || n_angles < 0) return "negative count";
  if ((long long)n_poses * n_angles > kSgMaxBeams) return "more than 2^26 beams in one call";
  if (n_poses > 0 && !poses_xyt) return "null poses";
  if (n_angles > 0 && !angles) return "null angles";
  if (n_poses > 0 && n_angles > 0 && (!range_out || !status_out)) return "null output";
  return nullptr;
}

// room for `bytes` in the context's scan-generation buffer (kept between calls; a larger request replaces it)
int sg_reserve(slamhip_ctx *ctx, size_t bytes) {
  // (whole 64 KiB: the floor is the rounded size itself)
  return grow_block(ctx->stream, ctx->d_scan_gen, ctx->scan_gen_cap, bytes, (bytes + 65535) & ~(size_t)65535);
}

size_t round8(size_t v) { return (v + 7) & ~(size_t)7; }

}  // namespace

// n_jobs x n_angles beams, job k over slot slots[k] from pose k: slamhip_gmapping_particle_generate_scans behind its
// particle checks.  Nothing is queued before every argument has passed.
int tile_pool_generate_scans(TilePool *tp, int variant, int flags, int n_jobs, const int *slots, const double *poses_xyt,
                             int n_angles, const double *angles, double max_dist, double occ_threshold, double *range_out,
                             unsigned char *status_out) {
  if (flags & ~SLAMHIP_SCAN_GEN_SEQUENTIAL) return sg_invalid("unknown flags");
  const char *why = sg_check_call(SLAMHIP_CELL_GMAPPING, 0, variant, n_jobs, poses_xyt, n_angles, angles, range_out, status_out);
  if (!why && n_jobs > 0 && !slots) why = "null particles";
  if (!why) why = sg_check_beams(tp->scale, n_jobs, poses_xyt, n_angles, angles, max_dist);
  if (why) return sg_invalid(why);
  for (int k = 0; k < n_jobs; ++k)
    if (slots[k] < 0 || slots[k] >= tp->n_slots) return sg_invalid("bad slot");
  const int n_beams = n_jobs * n_angles;
  if (n_beams == 0) return SLAMHIP_OK;
  slamhip_ctx *ctx = tp->ctx;
  SLAMHIP_CHECK(hipSetDevice(ctx->device));
  // one block: poses | angles | slots | ranges | status bytes; in and out are one copy each
  const size_t in_doubles = 3 * (size_t)n_jobs + (size_t)n_angles + ((size_t)n_jobs + 1) / 2;
  const size_t in_bytes = in_doubles * sizeof(double);
  const size_t out_bytes = (size_t)n_beams * sizeof(double) + round8((size_t)n_beams);
  int rc = sg_reserve(ctx, in_bytes + out_bytes);
  if (rc) return rc;
  // behind the queued copy-on-write clones and table patches; the tables are the current generation's from here on
  rc = tile_pool_flush(tp);
  if (rc) return rc;
  std::vector<double> &stage = ctx->scan_gen_stage;
  stage.resize(std::max(in_doubles, out_bytes / sizeof(double)));
  std::memcpy(stage.data(), poses_xyt, sizeof(double) * 3 * (size_t)n_jobs);
  std::memcpy(stage.data() + 3 * (size_t)n_jobs, angles, sizeof(double) * (size_t)n_angles);
  stage[in_doubles - 1] = 0.0;  // (the pad behind an odd number of slots)
  std::memcpy(stage.data() + 3 * (size_t)n_jobs + (size_t)n_angles, slots, sizeof(int) * (size_t)n_jobs);
  double *d_in = reinterpret_cast<double *>(ctx->d_scan_gen.get());
  double *d_range = d_in + in_doubles;
  unsigned char *d_status = reinterpret_cast<unsigned char *>(d_range + n_beams);
  SLAMHIP_CHECK(hipMemcpyAsync(d_in, stage.data(), in_bytes, hipMemcpyHostToDevice, ctx->stream));
  SgTiledMap m;
  m.pool = tp->d_pool;
  m.table = tp->d_table();
  m.tiles_x = tp->tiles_x;
  m.tiles_y = tp->tiles_y;
  m.origin_x = tp->origin_x;
  m.origin_y = tp->origin_y;
  m.scale = tp->scale;
  m.unknown_occ = tp->unknown[0];
  const int stride = tp->table_stride();
  hipEvent_t e0 = nullptr, e1 = nullptr;
  rc = profile_event_pair(ctx, &e0, &e1);
  if (rc) return rc;
  if (e0) SLAMHIP_CHECK(hipEventRecord(e0, ctx->stream));
  const double *d_poses = d_in, *d_angles = d_in + 3 * (size_t)n_jobs;
  const int *d_slots = reinterpret_cast<const int *>(d_angles + n_angles);
  const bool fma = variant == 1;
  if (flags & SLAMHIP_SCAN_GEN_SEQUENTIAL) {
    const dim3 grid((n_beams + kSgThreads - 1) / kSgThreads);
    if (fma)
      hipLaunchKernelGGL(k_scan_generate_tiled_seq<true>, grid, dim3(kSgThreads), 0, ctx->stream, m, stride, d_slots, d_poses,
                         n_angles, d_angles, n_beams, max_dist, occ_threshold, d_range, d_status);
    else
      hipLaunchKernelGGL(k_scan_generate_tiled_seq<false>, grid, dim3(kSgThreads), 0, ctx->stream, m, stride, d_slots, d_poses,
                         n_angles, d_angles, n_beams, max_dist, occ_threshold, d_range, d_status);
  } else {
    constexpr int per_block = kSgThreads / 64;
    const dim3 grid((n_beams + per_block - 1) / per_block);
    if (fma)
      hipLaunchKernelGGL(k_scan_generate_tiled_wave<true>, grid, dim3(kSgThreads), 0, ctx->stream, m, stride, d_slots, d_poses,
                         n_angles, d_angles, n_beams, max_dist, occ_threshold, d_range, d_status);
    else
      hipLaunchKernelGGL(k_scan_generate_tiled_wave<false>, grid, dim3(kSgThreads), 0, ctx->stream, m, stride, d_slots, d_poses,
                         n_angles, d_angles, n_beams, max_dist, occ_threshold, d_range, d_status);
  }
  SLAMHIP_CHECK(hipGetLastError());
  if (e1) SLAMHIP_CHECK(hipEventRecord(e1, ctx->stream));
  SLAMHIP_CHECK(hipMemcpyAsync(stage.data(), d_range, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
  SLAMHIP_CHECK(hipStreamSynchronize(ctx->stream));
  std::memcpy(range_out, stage.data(), sizeof(double) * (size_t)n_beams);
  std::memcpy(status_out, stage.data() + n_beams, (size_t)n_beams);
  return SLAMHIP_OK;
}

}  // namespace slamhip

using namespace slamhip;

// Which build of glibc's sincos this host's libm runs, found as libm_variant() finds it for sin / cos / exp: by calling it
// on arguments where the two restated builds differ.
int slamhip_scan_gen_libm_variant(int *variant) {
  if (!variant) return sg_invalid("null variant");
  static const int found = [] {
    void (*volatile p_sincos)(double, double *, double *) = ::sincos;
    unsigned long long st = 0x243f6a8885a308d3ull;
    int votes_fma = 0, votes_plain = 0, probes = 0;
    for (long it = 0; it < 4000000 && probes < 24; ++it) {
      st += 0x9e3779b97f4a7c15ull;
      unsigned long long z = st;
      z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
      z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
      const double x = 0.2 + 6.0 * ((double)((z ^ (z >> 31)) >> 11) * 0x1p-53);
      double s1, c1, s0, c0, s, c;
      libm_exact::sincos_<true>(x, &s1, &c1);
      libm_exact::sincos_<false>(x, &s0, &c0);
      if (s1 == s0 && c1 == c0) continue;
      p_sincos(x, &s, &c);
      ++probes;
      votes_fma += s == s1 && c == c1;
      votes_plain += s == s0 && c == c0;
    }
    if (probes < 24) return -1;
    return votes_fma == probes ? 1 : (votes_plain == probes ? 0 : -1);
  }();
  *variant = found;
  return SLAMHIP_OK;
}

int slamhip_scan_gen_angles(double half_sector, double angle_inc, int cap, double *angles, int *n) {
  if (!n || cap < 0 || (cap > 0 && !angles)) return sg_invalid("bad arguments");
  if (!(half_sector - half_sector == 0.0) || !(angle_inc > 0.0) || !(angle_inc - angle_inc == 0.0))
    return sg_invalid("half_sector must be finite and angle_inc positive and finite");
  // (the list ends at half_sector or 2 pi - half_sector, whichever comes first: at most 2 pi / angle_inc + 1 angles)
  if (!(2 * M_PI / angle_inc <= (double)kSgMaxBeams)) return sg_invalid("more than 2^26 angles");
  *n = (int)sg::sg_angles(half_sector, angle_inc, cap, angles);
  return SLAMHIP_OK;
}

int slamhip_map_generate_scans(slamhip_ctx *ctx, int map_id, int occ_kind, int variant, int flags, int n_poses,
                               const double *poses_xyt, int n_angles, const double *angles, double max_dist,
                               double occ_threshold, double *range_out, unsigned char *status_out) {
  if (!ctx || map_id < 0 || map_id >= (int)ctx->maps.size() || !ctx->maps[map_id].bound) return sg_invalid("unknown map id");
  const DeviceMap &dm = ctx->maps[map_id];
  if (flags & ~SLAMHIP_SCAN_GEN_SEQUENTIAL) return sg_invalid("unknown flags");
  const char *why = sg_check_call(dm.cell_model, occ_kind, variant, n_poses, poses_xyt, n_angles, angles, range_out, status_out);
  if (!why) why = sg_check_beams(dm.scale, n_poses, poses_xyt, n_angles, angles, max_dist);
  if (why) return sg_invalid(why);
  const int n_beams = n_poses * n_angles;
  if (n_beams == 0) return SLAMHIP_OK;
  SLAMHIP_CHECK(hipSetDevice(ctx->device));
  // one block: poses | angles | ranges | status bytes; in and out are one copy each
  const size_t in_doubles = 3 * (size_t)n_poses + (size_t)n_angles;
  const size_t in_bytes = in_doubles * sizeof(double);
  const size_t out_bytes = (size_t)n_beams * sizeof(double) + round8((size_t)n_beams);
  int rc = sg_reserve(ctx, in_bytes + out_bytes);
  if (rc) return rc;
  std::vector<double> &stage = ctx->scan_gen_stage;
  stage.resize(std::max(in_doubles, out_bytes / sizeof(double)));
  std::memcpy(stage.data(), poses_xyt, sizeof(double) * 3 * (size_t)n_poses);
  std::memcpy(stage.data() + 3 * (size_t)n_poses, angles, sizeof(double) * (size_t)n_angles);
  double *d_in = reinterpret_cast<double *>(ctx->d_scan_gen.get());
  double *d_range = d_in + in_doubles;
  unsigned char *d_status = reinterpret_cast<unsigned char *>(d_range + n_beams);
  SLAMHIP_CHECK(hipMemcpyAsync(d_in, stage.data(), in_bytes, hipMemcpyHostToDevice, ctx->stream));
  SgMap m;
  m.payload = dm.d_payload;
  m.width = dm.width;
  m.height = dm.height;
  m.pitch = dm.pitch;
  m.stride = cell_doubles(dm.cell_model);
  m.origin_x = dm.origin_x;
  m.origin_y = dm.origin_y;
  m.model = dm.cell_model;
  m.occ_kind = occ_kind;
  m.scale = dm.scale;
  m.unknown_occ = cell_occupancy(dm.cell_model, occ_kind, dm.unknown[0], dm.unknown[1], dm.unknown[2]);
  hipEvent_t e0 = nullptr, e1 = nullptr;
  rc = profile_event_pair(ctx, &e0, &e1);
  if (rc) return rc;
  if (e0) SLAMHIP_CHECK(hipEventRecord(e0, ctx->stream));
  const double *d_poses = d_in, *d_angles = d_in + 3 * (size_t)n_poses;
  const bool fma = variant == 1;
  if (flags & SLAMHIP_SCAN_GEN_SEQUENTIAL) {
    const dim3 grid((n_beams + kSgThreads - 1) / kSgThreads);
    if (fma)
      hipLaunchKernelGGL(k_scan_generate_seq<true>, grid, dim3(kSgThreads), 0, ctx->stream, m, d_poses, n_angles, d_angles,
                         n_beams, max_dist, occ_threshold, d_range, d_status);
    else
      hipLaunchKernelGGL(k_scan_generate_seq<false>, grid, dim3(kSgThreads), 0, ctx->stream, m, d_poses, n_angles, d_angles,
                         n_beams, max_dist, occ_threshold, d_range, d_status);
  } else {
    constexpr int per_block = kSgThreads / 64;
    const dim3 grid((n_beams + per_block - 1) / per_block);
    if (fma)
      hipLaunchKernelGGL(k_scan_generate_wave<true>, grid, dim3(kSgThreads), 0, ctx->stream, m, d_poses, n_angles, d_angles,
                         n_beams, max_dist, occ_threshold, d_range, d_status);
    else
      hipLaunchKernelGGL(k_scan_generate_wave<false>, grid, dim3(kSgThreads), 0, ctx->stream, m, d_poses, n_angles, d_angles,
                         n_beams, max_dist, occ_threshold, d_range, d_status);
  }
  SLAMHIP_CHECK(hipGetLastError());
  if (e1) SLAMHIP_CHECK(hipEventRecord(e1, ctx->stream));
  SLAMHIP_CHECK(hipMemcpyAsync(stage.data(), d_range, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
  SLAMHIP_CHECK(hipStreamSynchronize(ctx->stream));
  std::memcpy(range_out, stage.data(), sizeof(double) * (size_t)n_beams);
  std::memcpy(status_out, stage.data() + n_beams, (size_t)n_beams);
  return SLAMHIP_OK;
}

int slamhip_scan_generate_host(int cell_model, int occ_kind, int variant, int width, int height, int origin_x, int origin_y,
                               double scale, const double *unknown_payload, const double *payload, int n_poses,
                               const double *poses_xyt, int n_angles, const double *angles, double max_dist,
                               double occ_threshold, double *range_out, unsigned char *status_out) {
  if (cell_model < SLAMHIP_CELL_OCC || cell_model > SLAMHIP_CELL_CREDIBILIST) return sg_invalid("unknown cell model");
  if (width < 0 || height < 0 || !unknown_payload || ((size_t)width * height > 0 && !payload)) return sg_invalid("bad map");
  const char *why = sg_check_call(cell_model, occ_kind, variant, n_poses, poses_xyt, n_angles, angles, range_out, status_out);
  if (!why) why = sg_check_beams(scale, n_poses, poses_xyt, n_angles, angles, max_dist);
  if (why) return sg_invalid(why);
  const int sh = cell_stride_host(cell_model);
  SgMap m;
  m.payload = payload;
  m.width = width;
  m.height = height;
  m.pitch = width;
  m.stride = sh;
  m.origin_x = origin_x;
  m.origin_y = origin_y;
  m.model = cell_model;
  m.occ_kind = occ_kind;
  m.scale = scale;
  m.unknown_occ = cell_occupancy(cell_model, occ_kind, unknown_payload[0], sh > 1 ? unknown_payload[1] : 0.0,
                                 sh > 2 ? unknown_payload[2] : 0.0);
  if (variant == 1) sg_generate_host<true>(m, n_poses, poses_xyt, n_angles, angles, max_dist, occ_threshold, range_out, status_out);
  else sg_generate_host<false>(m, n_poses, poses_xyt, n_angles, angles, max_dist, occ_threshold, range_out, status_out);
  return SLAMHIP_OK;
}

int slamhip_scan_generate_host_tiled(int variant, int tiles_x, int tiles_y, int origin_x, int origin_y, double scale,
                                     double unknown_occ, const double *pool, int n_tiles, const int *table, int n_poses,
                                     const double *poses_xyt, int n_angles, const double *angles, double max_dist,
                                     double occ_threshold, double *range_out, unsigned char *status_out) {
  // (the extent's cell coordinates fit an int: the limit of the device pool is far below)
  if (tiles_x <= 0 || tiles_y <= 0 || tiles_x > 32768 || tiles_y > 32768) return sg_invalid("bad extent");
  if (!pool || n_tiles <= 0 || !table) return sg_invalid("null pool or table");
  for (int i = 0; i < tiles_x * tiles_y; ++i)
    if (table[i] < 0 || table[i] >= n_tiles) return sg_invalid("a table entry names no tile of the pool");
  const char *why = sg_check_call(SLAMHIP_CELL_GMAPPING, 0, variant, n_poses, poses_xyt, n_angles, angles, range_out, status_out);
  if (!why) why = sg_check_beams(scale, n_poses, poses_xyt, n_angles, angles, max_dist);
  if (why) return sg_invalid(why);
  const SgTiledMap m{pool, table, tiles_x, tiles_y, origin_x, origin_y, scale, unknown_occ};
  if (variant == 1) sg_generate_host<true>(m, n_poses, poses_xyt, n_angles, angles, max_dist, occ_threshold, range_out, status_out);
  else sg_generate_host<false>(m, n_poses, poses_xyt, n_angles, angles, max_dist, occ_threshold, range_out, status_out);
  return SLAMHIP_OK;
}
