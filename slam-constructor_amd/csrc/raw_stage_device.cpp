// raw_stage_device.cpp -- see raw_stage_device.h.

#include "raw_stage_device.h"

#include <type_traits>

namespace slamhip {

static int refused(const char *msg) {
  set_error(msg);
  return SLAMHIP_ERR_INVALID;
}

int RawDeviceStage::check_scan(const slamhip_raw_scan &s) {
  if (s.n <= 0 || !s.range || !s.angle) return kBadScan;
  if (s.trig_mode != SLAMHIP_TRIG_RAW && s.trig_mode != SLAMHIP_TRIG_CACHED) return kBadTrigMode;
  if (s.weighting < 0 || s.weighting > 2) return kBadWeighting;
  return kScanFine;
}

template <class Entry>
int RawDeviceStage::assemble(slamhip_ctx *ctx, const RawBatchJob *jobs) {
  constexpr bool kSixRows = std::is_same<Entry, ScanAssembleEachArgs>::value;
  const int n_jobs = (int)host.plan.size();
  int rc = grow_block(ctx->stream, h_arena_, h_cap_, host.arena_bytes, 1 << 16, 1, hipHostMallocMapped);
  if (rc) return rc;
  rc = host.fill(jobs, h_arena_.get());
  if (rc) return refused(scan_error_text(rc));
  // ---- the last check of the arguments lies behind: from here on the last call's blocks go (they point into the
  // block that a regrow frees)
  blocks.assign(n_jobs, Block{});
  rc = grow_block(ctx->stream, d_blocks_, d_cap_, host.dst_doubles, 1 << 14);
  if (rc) return rc;
  if (tabs_.size() < host.slots.size()) tabs_.resize(host.slots.size());
  bool sent = false;
  for (size_t q = 0; q < host.slots.size(); ++q) {
    RawBatchStage::Slot &sl = host.slots[q];
    if (!sl.fresh || sl.used != host.call) continue;
    rc = tabs_[q].upload(ctx->stream, sl.t, kSixRows ? 4 : 3);
    if (rc) return rc;
    sl.fresh = false;
    sent = true;
    ++ctx->scan_tab_uploads;
  }
  if (sent) SLAMHIP_CHECK(hipStreamSynchronize(ctx->stream));
  Entry *table = reinterpret_cast<Entry *>(h_arena_.get());
  for (int c = 0; c < n_jobs; ++c) {
    const RawBatchPlan &p = host.plan[c];
    if (p.live < 0) continue;
    const ScanTablesDevice &t = tabs_[p.table];
    host.entry(c, h_arena_.get(), ScanTablePlanes{t.cos(), t.sin(), t.viny(), t.angle()}, d_blocks_.get(), &table[p.live]);
    blocks[c] = Block{d_blocks_.get() + p.dst_at, p.stride, p.k, false};
  }
  hipEvent_t e0 = nullptr, e1 = nullptr;
  rc = profile_event_pair(ctx, &e0, &e1);
  if (rc) return rc;
  if (e0) SLAMHIP_CHECK(hipEventRecord(e0, ctx->stream));
  SLAMHIP_CHECK(launch_scan_assemble_table(table, host.n_live, host.max_stride, ctx->stream));
  if (e1) SLAMHIP_CHECK(hipEventRecord(e1, ctx->stream));
  if (ctx->profile) ++ctx->prof_launches;
  return SLAMHIP_OK;
}
template int RawDeviceStage::assemble<ScanAssembleArgs>(slamhip_ctx *, const RawBatchJob *);
template int RawDeviceStage::assemble<ScanAssembleEachArgs>(slamhip_ctx *, const RawBatchJob *);

int RawDeviceStage::download(slamhip_ctx *ctx, int job, int cap, double *out5, double *angle_out, int *n,
                             const char *too_small) const {
  const Block &k = blocks[job];
  *n = k.n;
  if (cap == 0 || k.n <= 0) return SLAMHIP_OK;
  if (k.lone || !k.d) return refused("that job went through the lone call: its scan is not in the batch's arena");
  if (cap < k.n) return refused(too_small);
  SLAMHIP_CHECK(hipSetDevice(ctx->device));
  SLAMHIP_CHECK(hipMemcpy2DAsync(out5, sizeof(double) * cap, k.d, sizeof(double) * k.stride, sizeof(double) * k.n, 5,
                                 hipMemcpyDeviceToHost, ctx->stream));
  if (angle_out)
    SLAMHIP_CHECK(hipMemcpyAsync(angle_out, k.d + 5 * k.stride, sizeof(double) * k.n, hipMemcpyDeviceToHost, ctx->stream));
  SLAMHIP_CHECK(hipStreamSynchronize(ctx->stream));
  return SLAMHIP_OK;
}

}  // namespace slamhip
