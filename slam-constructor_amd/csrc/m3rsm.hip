// m3rsm.hip -- expand and bound in one launch: the children of a layer of matches of the multi-resolution matcher
// (BF_M3RSM) made on the device by the reference's refinement rule and bounded by the pyramid's scorer
// (include/slamhip.h "map pyramid", slamhip_pyramid_expand_matches).
//
// What it replaces (paths relative to the reference root):
//   M3RSMEngine::branch                            src/core/scan_matchers/m3rsm_engine.h:338-357 -- per popped match two
//                                                  or four Match constructions, one scorer call each, one after the other
//   BruteForceMultiResolutionScanMatcher           src/core/scan_matchers/bf_multi_res_scan_matcher.h:55-64 -- the five
//                                                  crucial points of a box that no longer branches
//
// One workgroup of 256 threads per child SLOT (m3rsm_split.h: five per node, breadth first to depth D).  A workgroup
// walks its own ancestor path from the parent's rectangle in registers -- at most D refinements, a handful of FP64
// operations each, the same ones in every thread -- so no workgroup waits for another and nothing is exchanged.  A slot
// whose path ends early writes level -1 / NaN and leaves, the whole workgroup at once; the others run pyr_score_one,
// the body of k_pyr_score (map_pyramid_score.h), on the rectangle they arrived at.  Compute bound like k_pyr_score: a
// beam costs a sincos-free rotation, a window of at most 3 x 3 cells and one multiply-add chain.
//
// k_m3rsm_expand_many is the same launch for parents of SEVERAL scan matching requests
// (M3RSMEngine::add_scan_matching_request :291-316 called more than once: one queue, so a layer of its matches mixes
// requests): scan, level table and base pose come per parent from a request table in HBM
// (slamhip_pyramid_expand_requests), everything else is k_m3rsm_expand.
#include <cmath>
#include <cstring>
#include <vector>

#include "kernel_pick.h"
#include "m3rsm_split.h"
#include "map_pyramid_score.h"

namespace slamhip {
namespace {

struct ExpandArgs {
  MatchArgs m;       // rotation / rect / pose_sc: the n PARENTS; scores / level_out / terms: n x slots outputs
  double *rect_out;  // n x slots x (bot, top, left, right)
  double step;
  int slots;  // per parent: m3rsm::slots_of(depth)
};

// the multi-request form: the parents of one launch belong to different requests (the shared queue of
// m3rsm::run_many), each with its own scan, level table and base pose in a table in HBM
struct ExpandManyArgs {
  ManyArgs q;  // q.m as ExpandArgs::m (its own levels / scan / base are not read); q.request: per PARENT
  double *rect_out;
  double step;
  int slots;
};

template <int MODEL, bool RAW>
__global__ __launch_bounds__(kPyrThreads) void k_m3rsm_expand(ExpandArgs a) {
  __shared__ double s_trig[2];
  __shared__ double s_part[4];
  const size_t g = blockIdx.x;
  const size_t parent = g / (size_t)a.slots;
  const int slot = (int)(g - parent * (size_t)a.slots);
  const m3rsm::Rect top{a.m.rect[4 * parent], a.m.rect[4 * parent + 1], a.m.rect[4 * parent + 2], a.m.rect[4 * parent + 3]};
  m3rsm::Rect node;
  const bool there = m3rsm::slot_node(top, a.step, slot, &node);  // (uniform: every thread computes the same path)
  if (!there) {
    if (threadIdx.x == 0) {
      const double nan = __builtin_nan("");
      a.m.scores[g] = nan;
      a.m.level_out[g] = -1;
      a.rect_out[4 * g] = a.rect_out[4 * g + 1] = a.rect_out[4 * g + 2] = a.rect_out[4 * g + 3] = nan;
    }
    return;
  }
  if (threadIdx.x == 0) {
    a.rect_out[4 * g] = node.bot;
    a.rect_out[4 * g + 1] = node.top;
    a.rect_out[4 * g + 2] = node.left;
    a.rect_out[4 * g + 3] = node.right;
  }
  pyr_score_one<MODEL, RAW>(a.m, a.m, parent, g, a.m.terms, g * (size_t)a.m.scan.n, node.bot, node.top, node.left, node.right,
                            s_trig, s_part);
}

// One workgroup per slot, the same walk and the same outputs as above (the two kernels spell the slot's prologue out
// each: handed to a shared function through a pointer to the node it cost k_m3rsm_expand 13 VGPRs).  The request's entry
// of the table is uniform over the workgroup: it is read once, after the slot is known to hold a node, and everything
// per beam comes from that copy.
template <int MODEL, bool RAW>
__global__ __launch_bounds__(kPyrThreads) void k_m3rsm_expand_many(ExpandManyArgs a) {
  __shared__ double s_trig[2];
  __shared__ double s_part[4];
  const size_t g = blockIdx.x;
  const size_t parent = g / (size_t)a.slots;
  const int slot = (int)(g - parent * (size_t)a.slots);
  const MatchArgs &m = a.q.m;
  const m3rsm::Rect top{m.rect[4 * parent], m.rect[4 * parent + 1], m.rect[4 * parent + 2], m.rect[4 * parent + 3]};
  m3rsm::Rect node;
  const bool there = m3rsm::slot_node(top, a.step, slot, &node);  // (uniform, as above)
  if (!there) {
    if (threadIdx.x == 0) {
      const double nan = __builtin_nan("");
      m.scores[g] = nan;
      m.level_out[g] = -1;
      a.rect_out[4 * g] = a.rect_out[4 * g + 1] = a.rect_out[4 * g + 2] = a.rect_out[4 * g + 3] = nan;
    }
    return;
  }
  if (threadIdx.x == 0) {
    a.rect_out[4 * g] = node.bot;
    a.rect_out[4 * g + 1] = node.top;
    a.rect_out[4 * g + 2] = node.left;
    a.rect_out[4 * g + 3] = node.right;
  }
  const PyrSource q = a.q.table[a.q.request[parent]];
  const size_t terms_at = a.q.m.terms ? (size_t)a.q.terms_off[parent] + (size_t)slot * (size_t)q.scan.n : 0;
  pyr_score_one<MODEL, RAW>(q, a.q.m, parent, g, a.q.m.terms, terms_at, node.bot, node.top, node.left, node.right, s_trig,
                            s_part);
}

int check_expand(slamhip_ctx *ctx, slamhip_pyramid *p, const slamhip_spe_cfg *cfg, const double base_pose[3], int n,
                 double step, int depth) {
  int rc = pyr_check_fresh(p);
  if (rc) return rc;
  if (ctx != p->ctx) return pyr_invalid("the pyramid belongs to another context");
  rc = pyr_check_score_cfg(p, cfg);
  if (rc) return rc;
  if (n < 0 || !base_pose) return pyr_invalid("bad parent batch");
  if (!(step > 0.0) || !std::isfinite(step)) return pyr_invalid("the translation step must be positive and finite");
  if (depth < 1 || depth > m3rsm::kMaxDepth) return pyr_invalid("depth: 1, 2 or 3");
  if ((long long)n * m3rsm::slots_of(depth) > 0x7fffffffll) return pyr_invalid("too many slots for one launch");
  for (int k = 0; k < 3; ++k)
    if (!std::isfinite(base_pose[k])) return pyr_invalid("the base pose is not finite");
  return SLAMHIP_OK;
}

// queues the expansion of n parents whose arrays are in HBM (pose_sc may be null; raw: the table of beam directions
// queued in front of this launch -- a row per parent, its children inherit the rotation --, or null)
int queue_expand(slamhip_pyramid *p, const slamhip_spe_cfg *cfg, const double base[3], int n, const double *d_rotation,
                 const double *d_rect, const double *d_pose_sc, const RawTrig *raw, double step, int depth, double *d_rect_out,
                 double *d_scores, int *d_levels) {
  slamhip_ctx *ctx = p->ctx;
  const int slots = m3rsm::slots_of(depth);
  const size_t n_out = (size_t)n * slots;
  ExpandArgs a;
  std::memset(&a, 0, sizeof(a));
  int rc = pyr_fill_args(p, cfg, base, n_out, &a.m);
  if (rc) return rc;
  a.m.rotation = d_rotation;
  a.m.rect = d_rect;
  a.m.pose_sc = d_pose_sc;
  a.m.scores = d_scores;
  a.m.level_out = d_levels;
  a.m.n = n;
  if (raw) a.m.raw = *raw;
  a.rect_out = d_rect_out;
  a.step = step;
  a.slots = slots;
  ProfilePairGuard prof;
  rc = prof.open(ctx, ctx->stream, 0);
  if (rc) return rc;
  typedef void (*Kernel)(ExpandArgs);
  const Kernel kernel = pick_cell_model(p->cell_model, [raw](auto m) -> Kernel {
    return raw ? k_m3rsm_expand<decltype(m)::value, true> : k_m3rsm_expand<decltype(m)::value, false>;
  });
  SLAMHIP_CHECK(launch_kernel(kernel, dim3((unsigned)n_out), dim3(kPyrThreads), 0, ctx->stream, nullptr, nullptr, a));
  if (a.m.terms) {
    rc = pyr_launch_sum_sequential(a.m, n_out, ctx->stream);
    if (rc) return rc;
  }
  rc = prof.close();
  if (rc) return rc;
  if (ctx->profile) {
    ctx->prof_launches += 1;
    ctx->prof_units += (long long)n_out * a.m.scan.n;
  }
  return SLAMHIP_OK;
}

}  // namespace
}  // namespace slamhip

using namespace slamhip;

int slamhip_pyramid_expand_matches_device(slamhip_ctx *ctx, slamhip_pyramid *p, const slamhip_spe_cfg *cfg,
                                          const double base_pose[3], int n, const double *d_rotation, const double *d_rect,
                                          double translation_step, int depth, double *d_rect_out, double *d_score_out,
                                          int *d_level_out) {
  int rc = check_expand(ctx, p, cfg, base_pose, n, translation_step, depth);
  if (rc) return rc;
  if (n == 0) return SLAMHIP_OK;
  if (!d_rotation || !d_rect || !d_rect_out || !d_score_out || !d_level_out) return pyr_invalid("null device buffers");
  const bool raw = cfg->pose_trig == SLAMHIP_POSE_TRIG_RAW_EXACT;
  if (cfg->pose_trig != SLAMHIP_POSE_TRIG_DEVICE && !raw)
    return pyr_invalid("device-resident parents use device sincos (pose_trig = DEVICE) or RAW_EXACT: the host-trig mode takes "
                       "host arrays");
  SLAMHIP_CHECK(hipSetDevice(ctx->device));
  RawTrig rt{};
  if (raw) {
    // (the host does not see the rotations: every parent is a row of its own, row i for parent i)
    bool fma = false;
    const double *d_angle = nullptr;
    rc = pyr_raw_prepare(ctx, &fma, &d_angle);
    if (rc) return rc;
    rc = pyr_raw_queue_table(p, fma, d_rotation, n, base_pose[2], d_angle, ctx->scan_n, &rt);
    if (rc) return rc;
  }
  return queue_expand(p, cfg, base_pose, n, d_rotation, d_rect, nullptr, raw ? &rt : nullptr, translation_step, depth, d_rect_out,
                      d_score_out, d_level_out);
}

int slamhip_pyramid_expand_matches(slamhip_ctx *ctx, slamhip_pyramid *p, const slamhip_spe_cfg *cfg, const double base_pose[3],
                                   int n, const double *rotation, const double *rect, double translation_step, int depth,
                                   double *rect_out, double *score_out, int *level_out) {
  int rc = check_expand(ctx, p, cfg, base_pose, n, translation_step, depth);
  if (rc) return rc;
  if (n == 0) return SLAMHIP_OK;
  if (!rotation || !rect || !rect_out || !score_out || !level_out) return pyr_invalid("null parent or output arrays");
  const bool raw = cfg->pose_trig == SLAMHIP_POSE_TRIG_RAW_EXACT;
  if (cfg->pose_trig != SLAMHIP_POSE_TRIG_DEVICE && cfg->pose_trig != SLAMHIP_POSE_TRIG_HOST && !raw)
    return pyr_invalid("pose_trig: DEVICE, HOST or RAW_EXACT");
  for (int i = 0; i < n; ++i) {
    const double *r = rect + 4 * (size_t)i;
    // (a reversed rectangle is let through: it has no children, every slot of it comes back empty)
    if (!std::isfinite(rotation[i]) || !std::isfinite(r[0]) || !std::isfinite(r[1]) || !std::isfinite(r[2]) ||
        !std::isfinite(r[3]))
      return pyr_invalid("a parent's rotation or rectangle is not finite");
  }
  SLAMHIP_CHECK(hipSetDevice(ctx->device));
  bool fma = false;
  const double *d_angle = nullptr;
  if (raw) {  // (before anything is queued)
    rc = pyr_raw_prepare(ctx, &fma, &d_angle);
    if (rc) return rc;
  }
  const int slots = m3rsm::slots_of(depth);
  const size_t n_out = (size_t)n * slots;
  // (the parents' block and the slots' are sized anew together, whichever ran out: 256 and 2048 doubled)
  if (n > p->x_parent_cap) p->x_slot_cap = 0;
  rc = grow_blocks({ctx->stream}, p->x_slot_cap, n_out, 2048, [&](size_t scap) -> int {
    p->x_parent_cap = 0;
    int pcap = 256;
    while (pcap < n) pcap *= 2;
    // per slot 4 doubles of rectangle, the score and the level (an int behind the doubles): one block, one copy back;
    // the host side is pinned, parents in front of the results
    const size_t slot_doubles = 5 * scap + scap / 2;  // (5 doubles and an int per slot; scap is a power of two)
    SLAMHIP_CHECK(p->d_x_in.alloc(7 * (size_t)pcap));
    SLAMHIP_CHECK(p->d_x_out.alloc(slot_doubles));
    SLAMHIP_CHECK(p->h_x.alloc(7 * (size_t)pcap + slot_doubles));
    p->x_parent_cap = pcap;
    return SLAMHIP_OK;
  });
  if (rc) return rc;
  const bool host_trig = cfg->pose_trig == SLAMHIP_POSE_TRIG_HOST;
  double *stage = p->h_x.get(), *h_out = p->h_x.get() + 7 * (size_t)p->x_parent_cap;
  std::memcpy(stage, rotation, sizeof(double) * n);
  std::memcpy(stage + n, rect, sizeof(double) * 4 * n);
  if (host_trig)  // (one sincos call per parent: its children share the heading)
    for (int i = 0; i < n; ++i)
      ::sincos(rotation[i] + base_pose[2], &stage[5 * (size_t)n + 2 * i], &stage[5 * (size_t)n + 2 * i + 1]);
  // RAW_EXACT: the (sin, cos) part holds the rows' rotations (at most n doubles) and, behind them, a row per parent
  std::vector<double> rot_rows;
  if (raw) {
    pyr_raw_rows(n, rotation, reinterpret_cast<int *>(stage + 6 * (size_t)n), &rot_rows);
    std::memcpy(stage + 5 * (size_t)n, rot_rows.data(), sizeof(double) * rot_rows.size());
  }
  SLAMHIP_CHECK(hipMemcpyAsync(p->d_x_in.get(), stage, sizeof(double) * (host_trig || raw ? 7 : 5) * n, hipMemcpyHostToDevice,
                               ctx->stream));
  RawTrig rt{};
  if (raw) {
    rc = pyr_raw_queue_table(p, fma, p->d_x_in.get() + 5 * (size_t)n, (int)rot_rows.size(), base_pose[2], d_angle, ctx->scan_n, &rt);
    if (rc) return rc;
    rt.row = reinterpret_cast<const int *>(p->d_x_in.get() + 6 * (size_t)n);
  }
  double *d_rect_out = p->d_x_out.get(), *d_scores = p->d_x_out.get() + 4 * n_out;
  int *d_levels = reinterpret_cast<int *>(p->d_x_out.get() + 5 * n_out);
  rc = queue_expand(p, cfg, base_pose, n, p->d_x_in.get(), p->d_x_in.get() + n, host_trig ? p->d_x_in.get() + 5 * (size_t)n : nullptr,
                    raw ? &rt : nullptr, translation_step, depth, d_rect_out, d_scores, d_levels);
  if (rc) return rc;
  SLAMHIP_CHECK(hipMemcpyAsync(h_out, p->d_x_out.get(), (sizeof(double) * 5 + sizeof(int)) * n_out, hipMemcpyDeviceToHost, ctx->stream));
  SLAMHIP_CHECK(hipStreamSynchronize(ctx->stream));
  std::memcpy(rect_out, h_out, sizeof(double) * 4 * n_out);
  std::memcpy(score_out, h_out + 4 * n_out, sizeof(double) * n_out);
  std::memcpy(level_out, h_out + 5 * n_out, sizeof(int) * n_out);
  return SLAMHIP_OK;
}

int slamhip_pyramid_expand_requests(slamhip_ctx *ctx, const slamhip_spe_cfg *cfg, int n_requests,
                                    const slamhip_m3rsm_request *table, int n, const int *request, const double *rotation,
                                    const double *rect, double translation_step, int depth, double *rect_out,
                                    double *score_out, int *level_out) {
  std::vector<PyrSource> src;
  const int rc = pyr_many_sources(ctx, cfg, n_requests, table, &src);
  if (rc) return rc;
  return pyr_expand_sources(ctx, cfg, src, table[0].pyramid->cell_model, n, request, rotation, rect, translation_step, depth,
                            rect_out, score_out, level_out);
}

int slamhip::pyr_expand_sources(slamhip_ctx *ctx, const slamhip_spe_cfg *cfg, const std::vector<PyrSource> &src, int cell_model,
                                int n, const int *request, const double *rotation, const double *rect, double translation_step,
                                int depth, double *rect_out, double *score_out, int *level_out) {
  const int n_requests = (int)src.size();
  int rc = SLAMHIP_OK;
  if (n < 0) return pyr_invalid("bad parent batch");
  if (!(translation_step > 0.0) || !std::isfinite(translation_step))
    return pyr_invalid("the translation step must be positive and finite");
  if (depth < 1 || depth > m3rsm::kMaxDepth) return pyr_invalid("depth: 1, 2 or 3");
  if ((long long)n * m3rsm::slots_of(depth) > 0x7fffffffll) return pyr_invalid("too many slots for one launch");
  if (n == 0) return SLAMHIP_OK;
  if (!rect_out || !score_out || !level_out) return pyr_invalid("null output arrays");
  // (a reversed rectangle is let through: it has no children, every slot of it comes back empty)
  rc = pyr_many_check_batch(n_requests, n, request, rotation, rect, true);
  if (rc) return rc;
  SLAMHIP_CHECK(hipSetDevice(ctx->device));
  const int slots = m3rsm::slots_of(depth);
  const size_t n_out = (size_t)n * slots;
  ExpandManyArgs a;
  std::memset(&a, 0, sizeof(a));
  rc = pyr_many_stage(ctx, cfg, src, n, request, rotation, rect, slots, &a.q, &a.rect_out);
  if (rc) return rc;
  a.step = translation_step;
  a.slots = slots;
  ProfilePairGuard prof;
  rc = prof.open(ctx, ctx->stream, 0);
  if (rc) return rc;
  typedef void (*Kernel)(ExpandManyArgs);
  const bool raw = a.q.m.raw.cos != nullptr;
  const Kernel kernel = pick_cell_model(cell_model, [raw](auto m) -> Kernel {
    return raw ? k_m3rsm_expand_many<decltype(m)::value, true> : k_m3rsm_expand_many<decltype(m)::value, false>;
  });
  SLAMHIP_CHECK(launch_kernel(kernel, dim3((unsigned)n_out), dim3(kPyrThreads), 0, ctx->stream, nullptr, nullptr, a));
  if (a.q.m.terms) {
    rc = pyr_launch_sum_sequential_many(a.q, n_out, slots, ctx->stream);
    if (rc) return rc;
  }
  rc = prof.close();
  if (rc) return rc;
  if (ctx->profile) {
    ctx->prof_launches += 1;
    for (int i = 0; i < n; ++i) ctx->prof_units += (long long)slots * src[request[i]].scan.n;
  }
  return pyr_many_fetch(ctx, n_out, true, rect_out, score_out, level_out);
}
