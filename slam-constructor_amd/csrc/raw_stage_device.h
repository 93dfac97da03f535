// raw_stage_device.h -- K raw scans of one call on their way into HBM, stated once for the chains' batch
// (slamhip_matcher_process_raw_scan_batch) and for the multi-resolution matcher's fleet call
// (slamhip_matcher_m3rsm_match_each_raw): the host half (RawBatchStage, scan_filter.h: filter, rows, the scanners'
// tables), the ONE pinned arena k_scan_assemble_table reads, the arena in HBM it writes the scan blocks into, the
// scanners' tables in HBM (one ScanTablesDevice per slot of host.slots), and where each job's block of the last call
// lies.
#pragma once

#include "slamhip_internal.h"

namespace slamhip {

struct RawDeviceStage {
  RawBatchStage host;
  struct Block {
    const double *d = nullptr;  // null: none in the arena (nothing kept, or the job went through the lone call)
    size_t stride = 0;
    int n = 0;
    bool lone = false;
  };
  std::vector<Block> blocks;  // per job of the last call

  // What both calls refuse of a raw scan before anything else: 0, or which check fails (the caller has the texts).
  enum { kScanFine = 0, kBadScan, kBadTrigMode, kBadWeighting };
  static int check_scan(const slamhip_raw_scan &s);

  int prepare(int n_jobs, const RawBatchJob *jobs, size_t entry_bytes, int dst_rows) {
    return host.prepare(n_jobs, jobs, entry_bytes, dst_rows);
  }
  // The prepared call's live jobs into HBM on the context's stream, which must be idle (the call before returned after
  // what it had launched behind its assembly kernel had ended): the pinned arena grown and filled -- the last refusal;
  // the last call's blocks dropped before the arena in HBM may move; that arena grown; the tables of the scanners met
  // for the first time sent (the call waits for the copies instead of keeping the sources alive; a later call with
  // these scanners sends none); the args table of Entry at the pinned arena's offset 0; `blocks`; ONE launch.
  // Entry = ScanAssembleArgs: five rows per block.  ScanAssembleEachArgs: six, and the tables' angle plane.
  template <class Entry>
  int assemble(slamhip_ctx *ctx, const RawBatchJob *jobs);
  // job's block of the last call: *n its points, rows 0..4 to out5 (rows of `cap` doubles) and the sixth row to
  // angle_out where given.  too_small: the refusal's text where cap is below *n.
  int download(slamhip_ctx *ctx, int job, int cap, double *out5, double *angle_out, int *n, const char *too_small) const;

 private:
  PinnedBuf<unsigned char> h_arena_;
  DeviceBuf<double> d_blocks_;
  size_t h_cap_ = 0, d_cap_ = 0;
  std::vector<ScanTablesDevice> tabs_;
};

}  // namespace slamhip
