// matchers.cpp -- C-ABI of the matcher tier (include/slamhip.h): MC / HC / BF process_scan over the
// speculative drivers of matchers.h, and the host drivers of the device accept chains: ONE lone-chain driver
// (hill climbing, Monte Carlo) and ONE many-chains driver (K matches per call, one chain per particle).

#include <cstdlib>
#include <limits>
#include <mutex>

#include "bf_batch.h"
#include "bf_batch_plan.h"
#include "bf_device.h"
#include "bf_peaks_device.h"
#include "hc_chain_device.h"
#include "hc_shape.h"
#include "m3rsm_each.h"
#include "m3rsm_engine.h"
#include "map_pyramid_score.h"
#include "mc_chain_device.h"
#include "matchers.h"
#include "raw_stage_device.h"
#include "resident_policy.h"

namespace slamhip {

// {chains-done counter (0), initial poses, a table with one Entry per chain}: one block per side that ONE pull kernel
// moves in front of a launch (launch_block_pull)
template <class Entry>
struct StageBlock {
  PinnedBuf<char> h;
  DeviceBuf<char> d;
  size_t table_at = 0;
  int alloc(int cap, hipStream_t stream) {
    // [0, 16): the chains-done counter; then the initial poses; then the table (a pull copies the front of the
    // block up to the last entry in use)
    table_at = 16 + ((sizeof(double) * 3 * (size_t)cap + 15) & ~(size_t)15);
    const size_t bytes = table_at + ((sizeof(Entry) * (size_t)cap + 15) & ~(size_t)15);
    SLAMHIP_CHECK(h.alloc(bytes, hipHostMallocMapped));
    std::memset(h.get(), 0, bytes);
    SLAMHIP_CHECK(d.alloc(bytes));
    SLAMHIP_CHECK(hipMemsetAsync(d.get(), 0, bytes, stream));
    return SLAMHIP_OK;
  }
  unsigned *d_n_done() const { return reinterpret_cast<unsigned *>(d.get()); }
  double *h_inits() const { return reinterpret_cast<double *>(h.get() + 16); }
  double *d_inits() const { return reinterpret_cast<double *>(d.get() + 16); }
  Entry *h_table() const { return reinterpret_cast<Entry *>(h.get() + table_at); }
  Entry *d_table() const { return reinterpret_cast<Entry *>(d.get() + table_at); }
  size_t bytes_upto_inits(int n) const { return 16 + sizeof(double) * 3 * (size_t)n; }
  size_t bytes_upto_table(int n) const { return table_at + sizeof(Entry) * (size_t)n; }
};

// the speculation-tree shapes of a driver: instances per shape, instances of the largest one (grid size of a super-step)
struct ShapeSizes {
  int n_inst[kHcShapes] = {0};
  int max_inst = 1;
  unsigned long long packed() const {  // (HcChainArgs::n_inst)
    unsigned long long v = 0;
    for (int b = 0; b < kHcShapes; ++b) v |= (unsigned long long)(n_inst[b] & 0xff) << (8 * b);
    return v;
  }
};

// What the many-chains driver (run_many_chains) owns for its caller: per-chain control / result blocks, the staging
// block, the shapes, the co-resident form's exchange blocks.  `Rctl` is the exchange block of a chain, `Entry` what the
// staging table holds per chain.
template <class Rctl, class Entry>
struct ChainSet {
  int cap = 0;
  DeviceBuf<HcChainCtl> d_ctl;
  PinnedBuf<HcHostOut> h_out;  // one per chain
  StageBlock<Entry> stage;
  DeviceBuf<HcShape> d_shapes;
  ShapeSizes shapes;
  int built_inst = 0, nt = 256;
  PinnedBuf<unsigned> h_done_count;
  DeviceBuf<Rctl> d_rctl;            // co-resident form: one exchange block per chain (cap of them)
  PinnedBuf<unsigned> h_all_done;    // the last chain to end stores the epoch here
  int rctl_grid = 0, rctl_chains = 0;  // slots per chain / chains of the last co-resident launch
  unsigned rctl_launches = 0;          // co-resident launches on d_rctl (hc_tag)
  unsigned epoch = 0;
  double steps_avg;
  explicit ChainSet(double steps_avg0) : steps_avg(steps_avg0) {}
};

}  // namespace slamhip

struct BatchJobResult {
  double pose[3] = {0, 0, 0}, prob = 0;
  long long calls = 0, evaluated = 0, rescored = 0;
  int steps = 0, error = 0;
  bool on_chain = false;
};
// slamhip_matcher_process_scan_batch: blocks of the last batch (hc_batch_run); the staging table is the job table
struct HcBatch : slamhip::ChainSet<slamhip::HcResidentCtl, slamhip::HcJobView> {
  HcBatch() : ChainSet(16.0) {}
  bool resident_call = false;  // hc_resident_asked() of the call in flight, asked once
  slamhip::PinnedBuf<double> h_scan;  // the batch's scans: per match five arrays of its beam count
  slamhip::DeviceBuf<double> d_scan;
  size_t scan_cap = 0, h_scan_cap = 0;  // doubles d_scan / h_scan hold (they grow together)
  bool pair = false;    // the co-resident launch's workgroups (512 threads) score two poses per super-step
  int cus = 0;          // CUs of the device (sizes the pair form's trees)
  slamhip::PinnedBuf<slamhip::HcTraceEntry> h_trace;  // cap x trace_per entries (observer attached only)
  int trace_per = 0, trace_chains = 0;
  long long kernels = 0;
  std::vector<BatchJobResult> res;
  // slamhip_matcher_process_raw_scan_batch (the HC, MC and BF routes alike): the call's scans on their way into HBM,
  // and where each job's block of the last raw batch lies
  slamhip::RawDeviceStage raw;
};

// K Monte-Carlo matches per call (mc_batch_run): per-chain control / result blocks, the staged job table, the ONE arena
// the jobs' tape windows go through, the observer's trace slices
struct McBatch {
  int cap = 0;  // chains the blocks hold
  slamhip::DeviceBuf<slamhip::McChainCtl> d_ctl;
  slamhip::PinnedBuf<slamhip::McHostOut> h_out;
  slamhip::StageBlock<slamhip::McJobView> stage;
  slamhip::PinnedBuf<unsigned> h_done_count;
  slamhip::DeviceBuf<slamhip::McPair> d_tape;
  slamhip::PinnedBuf<double> h_tape;
  size_t tape_cap = 0, h_tape_cap = 0;  // pairs d_tape / h_tape hold (they grow together)
  slamhip::PinnedBuf<slamhip::McTraceEntry> h_trace;  // trace_chains x trace_per entries (observer attached only)
  size_t trace_per = 0;
  int trace_chains = 0;
  unsigned epoch = 0;
  double kernels_avg = 6.0;  // kernels the longest chain of a call needed, smoothed: sizes the first burst
  int slots = 0;             // candidates per job and super-step of the last call
};

// K brute-force sweeps per call (bf_batch_run): the staged job table, the jobs' slices of the flat score / fingerprint /
// prefix arrays, per job its aggregates, three counter words and its entry of the pinned result array, the call's ONE
// completion word, and what the hand-over needs to turn a best index into a pose
struct BfBatch {
  int job_cap = 0;
  long long pose_cap = 0, blk_cap = 0;
  slamhip::PinnedBuf<slamhip::BfJobView> h_jobs;
  slamhip::DeviceBuf<slamhip::BfJobView> d_jobs;
  slamhip::DeviceBuf<double> d_scores, d_agg_s;
  slamhip::DeviceBuf<unsigned long long> d_fp;
  slamhip::DeviceBuf<long long> d_pidx, d_agg_i;
  slamhip::DeviceBuf<unsigned> d_counters;
  slamhip::PinnedBuf<slamhip::BfHostOut> h_out;
  slamhip::PinnedBuf<unsigned> h_done;
  unsigned seq = 0;
  long long n = 0;                // poses per job of the last call
  std::vector<double> poses6;     // per job of the last call: its initial pose, its base
  std::vector<double> scores_host;  // the last call's K x n scores (observer attached only)
};

// The peaks of K score landscapes (bf_peaks_run): the volumes (job j's np = 1 + nx ny nt scores, the volume behind its
// first), the poses of a lone call, the staged job table of the shared scoring launch, the peaks kernels' scratch and the
// pinned block their results arrive in.  The matcher's sweeps and their counters never see any of it.
struct BfPeaksScratch {
  long long pose_cap = 0, lone_cap = 0, surv_cap = 0, out_cap = 0;
  int job_cap = 0;
  slamhip::DeviceBuf<double> d_scores, d_poses, d_plane_s;
  slamhip::DeviceBuf<int> d_plane_i;
  slamhip::PinnedBuf<slamhip::BfJobView> h_jobs;
  slamhip::DeviceBuf<slamhip::BfJobView> d_jobs;
  slamhip::DeviceBuf<unsigned long long> d_job_max;
  slamhip::DeviceBuf<unsigned> d_job_count;
  slamhip::DeviceBuf<slamhip::BfPeakKey> d_surv;
  slamhip::PinnedBuf<slamhip::BfPeaksHostOut> h_hdr;
  slamhip::PinnedBuf<slamhip::BfPeakKey> h_out;
  // the two scratch words of a job are zero between calls because k_bf_peaks_order clears them; a call whose launches
  // went out and whose wait did not come back leaves them unknown: the next call clears them first
  bool words_unknown = false;
  // slamhip_matcher_bf_peaks_stats: the last call that launched anything -- kernels counted where they are launched
  long long launches = 0, bound = 0;
  int shared = 0;
};

struct slamhip_matcher {
  // ---- what every kind of matcher has
  slamhip_ctx *ctx = nullptr;
  slamhip_spe_cfg cfg{};
  std::unique_ptr<slamhip::PoseEnumerator> pe;
  slamhip_observer obs{};
  bool has_obs = false;
  bool is_hc = false, is_mc = false, is_bf = false;
  int max_batch = 0;
  double p_accept0 = 0.25;  // prior per-candidate acceptance rate of a fresh match
  slamhip::MatchJob job;
  double t_stage_us = 0, t_score_us = 0;
  int device = 0;
  int tie_check = -1;  // checked default mode: -1 = not set yet (on), 0, 1 (slamhip_matcher_set_tie_check)
  long long chain_rescored = 0;  // super-steps (device chain) / batches (host-driven) of the last match scored twice
  long long tail_calls = 0;      // scorer calls of the last match / batch the co-resident chain reported in closed form
  long long rescored_poses = 0;
  std::vector<double> keep_scores;
  std::vector<unsigned long long> keep_fprints;
  // ---- the device chains (lone HC, lone MC, the HC batch): mode, epochs, the co-resident policy they share
  int chain_mode = -1;  // -1 = decide at the first match, 0 off, 1 the chain of kernels, 2 one co-resident launch
  bool chain_mode_explicit = false;  // set through slamhip_matcher_set_device_chain (not the default)
  int chain_nt = 1024, chain_ahead = 3;
  unsigned chain_epoch = 0;
  double chain_steps_avg = 12.0;
  long long chain_launched = 0;  // kernels launched by the last process_scan (steps + run-ahead)
  unsigned rctl_launches = 0;  // co-resident launches on this matcher's exchange block: the epoch bits of the tags (hc_tag)
  slamhip::ResidentPolicy resident;  // bounded spins that ran out: the kernel chain instead (resident_policy.h)
  // answers of the occupancy query so far, keyed by everything the answer depends on (kernel instantiation: cell model,
  // workgroup size, lone / batch / window form, sweep width via max_inst; dynamic LDS: scan length, beam constants)
  // (Pair: a batch whose workgroups score two poses; LoneRaw: a lone chain that assembles the raw scan itself)
  enum class ResidentForm { Lone, Batch, Window, MonteCarlo, Pair, LoneRaw };
  struct ResidentCap {
    int cell_model, nt;
    ResidentForm form;
    int n_beams, lds_consts, max_inst, cap, per_cu;
  };
  std::vector<ResidentCap> resident_caps;
  slamhip::PinnedBuf<slamhip::HcTraceEntry> h_trace;  // the observer's trace of a lone chain (HC and MC)
  int trace_cap = 0;
  slamhip::DeviceBuf<long long> d_stamps;  // debugging (slamhip_matcher_debug_stamps)
  int debug_resident_mute = 0;  // testing (slamhip_matcher_debug_resident_mute)
  int debug_trace_cap = 0;      // testing (slamhip_matcher_debug_trace_cap): pretend the trace buffer is this small
  int debug_fail_next = 0;      // testing (slamhip_matcher_debug_fail_next): injected failures left
  double debug_ends[5] = {0, 0, 0, 0, 0};  // testing: the host's clock at the ends of a lone match (SLAMHIP_MATCH_END)
  // ---- hill climbing kept on the device (hc_chain.h): parameters of the enumerator, device / pinned blocks
  struct HcChain {
    unsigned max_failed = 0;
    double dt = 0, dr = 0;
    slamhip::DeviceBuf<slamhip::HcChainCtl> d_chain;
    slamhip::DeviceBuf<slamhip::HcShape> d_shapes;
    slamhip::PinnedBuf<slamhip::HcHostOut> h_chain;
    slamhip::ShapeSizes shapes;
    // the co-resident form (hc_resident.hip, hc_resident_gm.hip): exchange block
    slamhip::DeviceBuf<slamhip::HcResidentCtl> d_rctl;
    slamhip::DeviceBuf<slamhip::HcResidentGmCtl> d_rctl_gm;
  } hc;
  std::unique_ptr<HcBatch> batch;  // K matches per call
  // ---- Monte Carlo kept on the device (mc_chain.h)
  struct McChain {
    slamhip::DeviceBuf<slamhip::McChainCtl> d_mc;
    slamhip::PinnedBuf<slamhip::McHostOut> h_mc;
    slamhip::DeviceBuf<slamhip::McResidentCtl> d_rctl;
    int rctl_grid = 0;  // workgroups of the last co-resident Monte-Carlo launch
    slamhip::DeviceBuf<slamhip::McPair> d_tape;
    slamhip::PinnedBuf<double> h_tape;  // staging of the tape window
    size_t tape_cap = 0;                // pairs d_tape / h_tape hold
    size_t tape_base = 0;               // absolute tape position of d_tape[0]
    size_t tape_filled = 0;             // pairs of the window already in HBM (or on their way, see tape_ready)
    hipStream_t tape_stream = nullptr;  // uploads the next match's pairs while this match's chain runs
    hipEvent_t tape_ready = nullptr;
    const void *tape_owner = nullptr;   // the enumerator whose tape the window holds (an engine stream may be swapped in)
    int slots = 0;
    ~McChain() {
      if (tape_stream) hipStreamDestroy(tape_stream);
      if (tape_ready) hipEventDestroy(tape_ready);
    }
  } mc;
  // ---- K robots' engines on one Monte-Carlo matcher (slamhip_matcher_set_mc_streams): stream k is the enumerator a
  // matcher created with seeds[k] would own, never reseeded, carried on from batch call to batch call
  struct McStream {
    std::unique_ptr<slamhip::PoseEnumerator> pe;  // a GaussianPoseEnumerator
    long long matches = 0;
  };
  std::vector<McStream> mc_streams;
  std::vector<int> mc_job_streams;  // stream of job j of the next batch calls (empty: job j uses stream j)
  long long mc_matches = 0;         // matches run on the matcher's own engine
  std::unique_ptr<McBatch> mc_batch;
  int debug_mc_batch_slots = 0;  // testing (slamhip_matcher_testing_mc_batch_slots): candidates per job and super-step
  // ---- brute force as one flat sweep + a device arg-max (bf_device.hip)
  struct BfSweep {
    double r[9] = {0};
    std::vector<double> off;  // x offsets, y offsets, theta offsets as the enumerator accumulates them
    int nx = 0, ny = 0, nt = 0;
    slamhip::DeviceBuf<double> d_off, d_poses, d_scores, d_agg_s;
    slamhip::DeviceBuf<unsigned long long> d_fp;
    slamhip::DeviceBuf<long long> d_pidx, d_agg_i;
    slamhip::DeviceBuf<unsigned> d_counters;
    slamhip::PinnedBuf<slamhip::BfHostOut> h_out;
    long long cap = 0;
    unsigned seq = 0;
    std::vector<double> scores_host;
    bool skip_device = false;  // the next lone match goes straight to the host-driven batches (a batch's ambiguous job)
  } bf;
  // ---- K robots' enumerators on one brute-force matcher (slamhip_matcher_set_bf_streams; bf_batch_plan.h)
  slamhip::BfStreams bf_streams;
  long long bf_matches = 0;  // matches run on the matcher's own enumerator
  std::unique_ptr<BfBatch> bf_batch;
  std::unique_ptr<BfPeaksScratch> bf_peaks;  // slamhip_matcher_bf_peaks / _batch
  // ---- the multi-resolution matcher (BF_M3RSM): the best-first engine of m3rsm_engine.h over a pyramid's expand launches
  struct M3rsm {
    slamhip_pyramid *pyr = nullptr;  // the caller's; must outlive the matcher's matches
    slamhip::m3rsm::Config cfg;
    slamhip::m3rsm::Result res;
    std::vector<slamhip::m3rsm::Call> trace;  // the committed calls of the last match
    bool per_pop = false;  // no expand launches: a slamhip_pyramid_score_matches launch per popped match
    // slamhip_matcher_set_m3rsm_rotation_slots: a request's scan_slot is the FIRST of one slot per root rotation
    bool rot_slots = false;
    // the last slamhip_matcher_m3rsm_match_each: per request its result, the engine's code and its committed calls
    std::vector<slamhip::m3rsm::Result> each_res;
    std::vector<int> each_code;
    std::vector<std::vector<slamhip::m3rsm::Call>> each_trace;
    int each_threads = 0;  // workers of the host half of a round (0: min(requests, 8))
    std::unique_ptr<slamhip::m3rsm::Pool> each_pool;  // ... kept from call to call, made anew when the count changes
    long long copied_back = 0;  // bytes the launches of the last match wrote back to the host (scores, levels, rectangles)
    // slamhip_matcher_m3rsm_match_each_raw: its own raw-scan stage (the chains' HcBatch is not touched), made by its first call
    std::unique_ptr<slamhip::RawDeviceStage> raw;
  };
  bool is_m3rsm = false;
  std::unique_ptr<M3rsm> m3;
};

using namespace slamhip;

namespace {

int invalid_arg(const char *msg) {
  set_error(msg);
  return SLAMHIP_ERR_INVALID;
}

int make_matcher(slamhip_ctx *ctx, const slamhip_spe_cfg *cfg, std::unique_ptr<PoseEnumerator> pe,
                 int default_batch, slamhip_matcher **out) {
  if (!ctx || !cfg || !out) return invalid_arg("null argument");
  auto *m = new slamhip_matcher;
  m->ctx = ctx;
  m->device = ctx->device;
  m->cfg = *cfg;
  m->pe = std::move(pe);
  m->max_batch = default_batch;
  *out = m;
  return SLAMHIP_OK;
}

constexpr int kChainNeedsHost = 1;  // internal: positive, never leaves the library
// internal: a GMapping-OOPE chain met a comparison its tree sums (device exp) cannot settle the reference's way; nothing
// has been reported: the match is redone in the exact mode (call order, beam-order sums, glibc's exp: exact_kernels.hip)
constexpr int kChainUnsettled = 3;
constexpr int kChainDefaultMode = 2;  // device chains: 1 = a kernel per super-step, 2 = one co-resident launch where it applies

// ---- pieces every driver uses ----------------------------------------------------------------------

// the next value of an epoch / sequence counter; 0 is never handed out (it is what cleared memory holds)
unsigned next_epoch(unsigned &counter) {
  if (++counter == 0) ++counter;
  return counter;
}

// the observer's events of a device chain, from its pinned trace, in call order
void replay_trace(const slamhip_observer &obs, const HcTraceEntry *entries, long long calls) {
  for (long long i = 0; i < calls; ++i) {
    const HcTraceEntry &e = entries[i];
    const double p3[3] = {e.x, e.y, e.theta};
    if (obs.on_scan_test) obs.on_scan_test(obs.user, p3, e.score);
    if (e.accepted && obs.on_pose_update) obs.on_pose_update(obs.user, p3, e.score);
  }
}

// the speculation-tree shapes for at most `want` round instances, built and uploaded; `reach`: the probability of
// being on the walked path below which no instance is added (repeated outcomes weigh 1.0)
int build_shapes(int want, double reach, HcShape *d_shapes, ShapeSizes *sizes) {
  std::vector<HcShape> shapes(kHcShapes);
  sizes->max_inst = 1;
  for (int b = 0; b < kHcShapes; ++b) {
    hc_build_shape(hc_bucket_rate(b), 1.0, reach, want, &shapes[b]);
    sizes->n_inst[b] = shapes[b].n_inst;
    sizes->max_inst = std::max(sizes->max_inst, shapes[b].n_inst);
  }
  SLAMHIP_CHECK(hipMemcpy(d_shapes, shapes.data(), sizeof(HcShape) * kHcShapes, hipMemcpyHostToDevice));
  return SLAMHIP_OK;
}

// ---- hill climbing on the device ------------------------------------------------------------------
// Failed-round limits the device chains cover.  A chain halves both steps once per failed round -- as ONE exact
// multiplication by 2^-f per walked segment (hc_chain.h) where the reference halves f times: the two agree as long as
// no intermediate is subnormal, i.e. as long as step * 2^-(limit + 1) is a normal double (limit <= 1000 keeps 2^-f
// itself representable).  r01-r03 stopped at 250 for no better reason than the size of a byte.
bool hc_limit_on_device(const slamhip_matcher *m) {
  if (m->hc.max_failed == 0 || m->hc.max_failed > 1000) return false;  // (also: 16 bits in HcNextEntry::counts)
  for (double step : {m->hc.dt, m->hc.dr}) {
    if (step == 0.0) continue;  // (a zero step stays zero either way)
    int e = 0;
    (void)std::frexp(std::fabs(step), &e);
    if (!std::isfinite(step) || e - 1 - (int)m->hc.max_failed - 1 < -1021) return false;
  }
  return true;
}

bool is_window_oope(int oope) {
  return oope == SLAMHIP_OOPE_MAX || oope == SLAMHIP_OOPE_MEAN || oope == SLAMHIP_OOPE_OVERLAP;
}

bool tie_check_default(slamhip_matcher *m) {
  if (m->tie_check < 0) m->tie_check = 1;  // (slamhip_matcher_set_tie_check switches it off)
  return m->tie_check == 1;
}

// The device chain covers hill climbing over the 1-cell, the window and the GMapping OOPEs with device pose
// trigonometry on the zero-copy path; everything else (strict order, host trigonometry, staged copies, small
// batches) keeps the host-driven path.
bool chain_eligible(slamhip_matcher *m) {
  if (!m->is_hc || !hc_limit_on_device(m)) return false;
  const bool gm = m->cfg.oope == SLAMHIP_OOPE_GMAPPING;
  // (the window OOPEs ride the co-resident form only: hc_resident.hip's WIN instantiations, default sum order)
  const bool win = is_window_oope(m->cfg.oope);
  if (win && (m->cfg.sum_order != SLAMHIP_SUM_TREE256 || m->chain_mode == 1)) return false;
  if ((m->cfg.oope != SLAMHIP_OOPE_OBSTACLE && !gm && !win) || m->cfg.pose_trig != SLAMHIP_POSE_TRIG_DEVICE) return false;
  // the GMapping OOPE rides K3's one-pose body: 3x3 window, up to 1280 beams, canonical sum
  if (gm && (m->cfg.gm_window != 1 || m->cfg.sum_order != SLAMHIP_SUM_TREE256 || m->ctx->scan_n > 1280)) return false;
  if (!m->ctx->low_latency || m->ctx->stage_poses) return false;
  if (m->ctx->scan_n > 4096) return false;  // the terms of a pose sit in LDS (8 bytes per beam next to 15 KB of replay state)
  if (m->max_batch < 6 * kHcMaxInst) return false;  // slamhip_matcher_set_batch asked for small batches
  if (m->chain_mode < 0) m->chain_mode = kChainDefaultMode;  // (slamhip_matcher_set_device_chain changes it)
  return m->chain_mode >= 1;
}

// Is this hill-climbing call asked to run as ONE launch of co-resident workgroups?  (Whether the grid fits the device
// at once is the driver's question.)  Asks the policy, so: once per call.
bool hc_resident_asked(slamhip_matcher *m) {
  // A LONE chain over the GMapping OOPE is co-resident only when asked for (mode 2 set explicitly): measured on
  // MI355X it is no faster than the chain of kernels (r05: 12.46 against 12.40 us per super-step,
  // profiles/r05_resident_stamps.txt / r05_chain_stamps.txt; the shared-map filter step 12.9 against 13.0 ms) -- four
  // granules per pose instead of one, a second workgroup barrier per super-step -- while a filter step's MANY chains
  // in one launch are (gm_multi_chain_run: 0.58 -> 0.44 ms per 100 particles).
  const bool gm = m->cfg.oope == SLAMHIP_OOPE_GMAPPING && m->chain_mode_explicit;
  const bool armed = m->resident.armed();
  return m->chain_mode == 2 && (m->cfg.oope == SLAMHIP_OOPE_OBSTACLE || is_window_oope(m->cfg.oope) || gm) && armed;
}
// ---- co-resident launches of ONE process on one device (two contexts -- two robots -- on a GPU).
// A co-resident grid only runs when ALL its workgroups are on the chip; two such grids launched at once can each get
// half and wait for the other's slots until their spin bounds run out.  Within a process the library knows who is
// resident: a launch takes its CUs' worth of slots from this per-device ledger for as long as its host call lasts
// (process_scan is synchronous) and, when they are not there, runs as the chain of kernels AT ONCE -- nobody stalls.
// (Across processes only the bounded spins help: sized from the matches seen, ResidentPolicy::spin_limit.)
std::mutex g_resident_mu;
int g_resident_cus[64] = {0};
int g_device_cus[64] = {0};
struct ResidentLease {
  int device = -1, cus = 0;
  bool take(int dev, int wgs, int per_cu) {
    if (dev < 0 || dev >= 64 || per_cu <= 0) return false;
    std::lock_guard<std::mutex> lk(g_resident_mu);
    if (g_device_cus[dev] == 0) {
      int n = 0;
      if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 1) return false;
      g_device_cus[dev] = n;
    }
    const int need = (wgs + per_cu - 1) / per_cu;
    if (g_resident_cus[dev] + need > g_device_cus[dev] - 1) return false;  // (the capacity's one CU of margin stays free)
    g_resident_cus[dev] += need;
    device = dev;
    cus = need;
    return true;
  }
  void release() {
    if (device < 0) return;
    std::lock_guard<std::mutex> lk(g_resident_mu);
    g_resident_cus[device] -= cus;
    device = -1;
  }
  ~ResidentLease() { release(); }
};

using ResidentForm = slamhip_matcher::ResidentForm;
int resident_capacity(slamhip_matcher *m, int cell_model, int nt, ResidentForm form, int n_beams, bool lds_consts, int max_inst,
                      int *wgs, int *per_cu = nullptr) {
  for (const auto &c : m->resident_caps)
    if (c.cell_model == cell_model && c.nt == nt && c.form == form && c.n_beams == n_beams &&
        c.lds_consts == (lds_consts ? 1 : 0) && c.max_inst == max_inst) {
      *wgs = c.cap;
      if (per_cu) *per_cu = c.per_cu;
      return SLAMHIP_OK;
    }
  int cap = 0, pc = 0;
  if (form == ResidentForm::MonteCarlo) {
    SLAMHIP_CHECK(mc_resident_capacity(cell_model, nt, n_beams, lds_consts, &cap, &pc));
  } else {
    const bool pair = form == ResidentForm::Pair;
    const HcResidentKey key{nt, max_inst, false, pair || form == ResidentForm::Batch, pair, form == ResidentForm::Window,
                            form == ResidentForm::LoneRaw};
    SLAMHIP_CHECK(hc_resident_capacity(cell_model, key, n_beams, lds_consts, &cap, &pc));
  }
  if (cap < 0) cap = 0;
  if (m->resident_caps.size() >= 64) m->resident_caps.clear();  // (scans of ever-changing lengths: start over)
  m->resident_caps.push_back({cell_model, nt, form, n_beams, lds_consts ? 1 : 0, max_inst, cap, pc});
  *wgs = cap;
  if (per_cu) *per_cu = pc;
  return SLAMHIP_OK;
}
// the 1-cell form keeps the further beams' constants in LDS (HcChainArgs::lds_consts) when `wgs_needed` workgroups
// are resident together with that much LDS each
int resident_capacity_pick(slamhip_matcher *m, int cell_model, int nt, ResidentForm form, int n_beams, int max_inst, int wgs_needed,
                           bool may_lds_consts, int *lds_consts, int *wgs, int *per_cu = nullptr) {
  *lds_consts = 0;
  if (may_lds_consts) {
    int rc = resident_capacity(m, cell_model, nt, form, n_beams, true, max_inst, wgs, per_cu);
    if (rc) return rc;
    if (wgs_needed <= *wgs) {
      *lds_consts = 1;
      return SLAMHIP_OK;
    }
  }
  return resident_capacity(m, cell_model, nt, form, n_beams, false, max_inst, wgs, per_cu);
}

// ---- the lone-chain driver (hill climbing, Monte Carlo) -----------------------------------------------
struct LoneChainText {  // what the messages call the chain
  const char *resident_ended, *resident, *no_end, *step;
};

// Waits on pinned memory until the chain has published its result under `epoch`.  kResident: ONE launch is running;
// else the chain of kernels, which the host keeps `ahead` launches in front of the step the GPU reports (a launch
// costs the host ~3.5 us, a super-step the GPU ~5 us).  `idle` is what the host does between two polls: at least a
// pause.  Every 2^20 polls the stream is asked whether something went wrong.
template <bool kResident, class HostOut, class LaunchOne, class Idle>
int lone_chain_wait(slamhip_ctx *ctx, volatile HostOut *h, unsigned epoch, int ahead, const int &launched,
                    LaunchOne &&launch_one, Idle &&idle, const LoneChainText &text) {
  unsigned long long spins = 0;
  while (h->done_seq != epoch) {
    if constexpr (!kResident) {
      const int started = (int)h->progress;
      if (launched - started < ahead) {
        if (launched >= (1 << 20)) {
          set_error(text.no_end);
          return SLAMHIP_ERR_STATE;
        }
        const int rc = launch_one();
        if (rc) return rc;
        continue;
      }
    }
    const int rc = idle();
    if (rc) return rc;
    if ((++spins & 0xfffffull) == 0) {
      hipError_t qe = hipStreamQuery(ctx->stream);
      if (kResident && qe == hipSuccess && h->done_seq != epoch) {
        set_error(text.resident_ended);
        return SLAMHIP_ERR_STATE;
      }
      if (qe != hipSuccess && qe != hipErrorNotReady) return hip_fail(qe, kResident ? text.resident : text.step);
    }
  }
  __atomic_thread_fence(__ATOMIC_ACQUIRE);
  return SLAMHIP_OK;
}

// One match as one chain.  `resident`: try the co-resident form first --
//   fit(lease, &fits)           capacity, the lease, the exchange block (allocated / cleared on the context's stream):
//                               the kind's own; fits = false: the chain of kernels at once
//   launch_resident(e0, e1)     the ONE launch
//   fail_over(gave_up)          the co-resident form did not run (gave_up: it was launched and left without a result,
//                               the stream has been drained): the kind prepares `a` for the chain of kernels
//   launch_step(step, e0, e1)   one kernel of the chain
// On return the result is in *h (acquire fence passed), *t0 is the start of the form that ran.
template <class Args, class HostOut, class Fit, class LaunchResident, class FailOver, class LaunchStep, class Idle>
int run_lone_chain(slamhip_matcher *m, Args &a, volatile HostOut *h, bool resident, const double &t0, int *launched_out,
                   Fit &&fit, LaunchResident &&launch_resident, FailOver &&fail_over, LaunchStep &&launch_step,
                   Idle &&idle, const LoneChainText &text) {
  slamhip_ctx *ctx = m->ctx;
  int launched = 0, rc = SLAMHIP_OK;
  auto launch_one = [&]() -> int {
    hipEvent_t e0, e1;
    int r = profile_event_pair(ctx, &e0, &e1);
    if (r) return r;
    SLAMHIP_CHECK(launch_step(launched, e0, e1));
    ++launched;
    return SLAMHIP_OK;
  };
  bool ran_resident = false;
  if (resident) {
    // ---- ONE launch: every workgroup of the tree stays on the chip for the whole match
    ResidentLease lease;
    bool fits = false, gave_up = false;
    rc = fit(lease, &fits);
    if (rc) return rc;
    if (fits) {
      a.spin_limit = m->resident.spin_limit();
      a.tag_epoch = ++m->rctl_launches;
      a.debug_mute = m->debug_resident_mute;
      hipEvent_t e0, e1;
      rc = profile_event_pair(ctx, &e0, &e1);
      if (rc) return rc;
      SLAMHIP_CHECK(launch_resident(e0, e1));
      launched = 1;
      m->resident.note_launch();
      rc = lone_chain_wait<true>(ctx, h, a.epoch, 0, launched, launch_one, idle, text);
      if (rc) return rc;
      if (h->error == 4 || h->error == 5) {
        // a workgroup was not resident with the others (the bounded sweep ran out), or the chain is longer than a
        // tag counts: nothing has been reported; wait for the stragglers to leave, then the kernel chain runs the match
        SLAMHIP_CHECK(hipStreamSynchronize(ctx->stream));
        if (h->error == 4) m->resident.note_give_up();
        h->error = 0;
        launched = 0;
        gave_up = true;
      } else {
        m->resident.note_success(MatchJob::now_us() - t0);
        ran_resident = true;
      }
    }
    if (!ran_resident) {
      rc = fail_over(gave_up);
      if (rc) return rc;
    }
  }
  if (!ran_resident) {
    // the expected number of super-steps goes out at once; afterwards the host stays a few launches ahead
    const int first = std::max(2, std::min(256, (int)(m->chain_steps_avg * 0.75)));
    for (int i = 0; i < first; ++i) {
      rc = launch_one();
      if (rc) return rc;
    }
    rc = lone_chain_wait<false>(ctx, h, a.epoch, m->chain_ahead, launched, launch_one, idle, text);
    if (rc) return rc;
  }
  *launched_out = launched;
  return SLAMHIP_OK;
}

// a lone chain's result into the matcher and out to the caller / the observer (the kind has mapped h->error already)
template <class HostOut>
int lone_chain_report(slamhip_matcher *m, volatile HostOut *h, int launched, int scan_n, double t0,
                      const double init_pose[3], double out_delta[3], double *out_prob) {
  slamhip_ctx *ctx = m->ctx;
  MatchJob &job = m->job;
  job.scorer_calls = h->calls;
  job.poses_evaluated = h->evaluated;
  job.launches = h->steps;
  job.t_build_us = job.t_replay_us = 0;
  m->chain_launched = launched;
  m->chain_rescored = h->rescored;
  m->chain_steps_avg = 0.75 * m->chain_steps_avg + 0.25 * (double)h->steps;
  if (ctx->profile) {
    // every kernel launched carries an event pair, the run-ahead ones that found the chain finished too
    // (rocprofv3 counts them as dispatches of the same kernel)
    ctx->prof_launches += launched;
    ctx->prof_units += h->evaluated * (long long)scan_n;
  }
  out_delta[0] = h->pose[0] - init_pose[0];
  out_delta[1] = h->pose[1] - init_pose[1];
  out_delta[2] = h->pose[2] - init_pose[2];
  *out_prob = h->best_prob;
  m->t_score_us = MatchJob::now_us() - t0;
  if (m->has_obs) {
    const double t1 = MatchJob::now_us();
    replay_trace(m->obs, m->h_trace.get(), h->calls);
    job.t_replay_us = MatchJob::now_us() - t1;
    if (m->obs.on_matching_end) m->obs.on_matching_end(m->obs.user, out_delta, *out_prob);
  }
  return SLAMHIP_OK;
}

int chain_prepare(slamhip_matcher *m) {
  slamhip_matcher::HcChain &hc = m->hc;
  if (hc.d_chain) return SLAMHIP_OK;
  SLAMHIP_CHECK(hc.d_chain.alloc(1));
  // (every clearing of a fresh device block goes on the context's own stream: that stream is non-blocking, a hipMemset
  // on the null stream is asynchronous for device memory and NOT ordered with it -- the block's first user could run
  // ahead of the memset and have its staged data zeroed under it: r05, a sharded step that started from pose 0 once
  // in fifteen runs with three contexts on one device)
  SLAMHIP_CHECK(hipMemsetAsync(hc.d_chain.get(), 0, sizeof(HcChainCtl), m->ctx->stream));
  SLAMHIP_CHECK(hc.d_shapes.alloc(kHcShapes));
  // 42 instances = 253 workgroups of 1024 threads: ONE per CU, all resident at once.  Measured against 64
  // instances x 512 threads (two workgroups per CU, a tree half as large again): cfg2 0.149 -> 0.138 ms per match
  // (one more super-step, each 0.8 us shorter), the shared-map filter step 4.3 k -> 5.0 k particles/s (K3's one-pose
  // body 10.7 -> 7 us); 32 or 52 instances, or 512 threads with 42, are slower again.
  const int rc = build_shapes(kHcDefaultInst, 0.002, hc.d_shapes.get(), &hc.shapes);
  if (rc) return rc;
  SLAMHIP_CHECK(hc.h_chain.alloc(1, kPinnedCoherent));
  std::memset(hc.h_chain.get(), 0, sizeof(HcHostOut));
  return SLAMHIP_OK;
}

// testing builds: the host's clock at the ends of a lone hill-climbing match behind slamhip_matcher_process_raw_scan --
// 0 entry, 1 filter and staging done, 2 the co-resident launch called, 3 the launch call returned, 4 the result seen.
// slamhip_matcher_timing of such a match without an observer then reports build_us = 0 -> 1, stage_us = 1 -> 2 and
// replay_us = 3 -> 4 (tools/match_ends.py); the shipped library reads no clock for them
#ifdef SLAMHIP_TESTING
#define SLAMHIP_MATCH_END(m, i) ((m)->debug_ends[i] = slamhip::MatchJob::now_us())
#else
#define SLAMHIP_MATCH_END(m, i) ((void)0)
#endif

int chain_process_scan(slamhip_matcher *m, int map_id, const double init_pose[3], double out_delta[3],
                       double *out_prob, bool resident) {
  slamhip_ctx *ctx = m->ctx;
  slamhip_matcher::HcChain &hc = m->hc;
  int rc = chain_prepare(m);
  if (rc) return rc;
  HcChainArgs a;
  std::memset(&a, 0, sizeof(a));
  int cell_model = 0, oie_eff = m->cfg.oie;
  // (window OOPEs read the cells themselves: the view stays the map's own; the 1-cell form may come through a TBM
  // map's probability plane -- then as an OCC view under the occupancy OIE)
  rc = score_views(ctx, map_id, &m->cfg, &a.map, &a.scan, &cell_model, nullptr, &oie_eff);
  if (rc) return rc;
  if (m->has_obs && !m->h_trace) {
    m->trace_cap = 1 << 16;
    SLAMHIP_CHECK(m->h_trace.alloc(m->trace_cap, kPinnedCoherent));
  }
  const bool win = is_window_oope(m->cfg.oope), gm = m->cfg.oope == SLAMHIP_OOPE_GMAPPING;
  // A raw scan whose block nobody has assembled yet (slamhip_matcher_process_raw_scan): the lone co-resident 1-cell
  // chain in the default sum order takes the assembly into its own launch, once it is known to fit (below);
  // everything else reads the block
  if (!resident || win || gm || m->cfg.sum_order == SLAMHIP_SUM_SEQUENTIAL || !ctx->raw_prologue) {
    rc = scan_assemble_now(ctx);
    if (rc) return rc;
  }
  a.oie = oie_eff;
  a.oope = win ? m->cfg.oope : SLAMHIP_OOPE_OBSTACLE;
  for (int k = 0; k < 4; ++k) a.area[k] = m->cfg.area[k];
  if (win && !resident) return kChainNeedsHost;  // (no kernel-chain form: host-driven batches)
  a.max_inst = hc.shapes.max_inst;
  a.gm.fullness_th = m->cfg.gm_fullness_th;
  a.gm.window = m->cfg.gm_window;
  a.gm_cx = ctx->gm_cx;
  a.gm_cy = ctx->gm_cy;
  a.gm_prob = ctx->gm_prob;
  a.seq = m->cfg.sum_order == SLAMHIP_SUM_SEQUENTIAL ? 1 : 0;
  // (the 1-cell AND the window OOPEs: `max` is as discrete as the 1-cell value, so mathematically tied candidates
  // are as likely -- VERDICT r4 item 2; the GMapping OOPE's chains decide from the tree sums: include/slamhip.h)
  // (the 1-cell OOPE: unsettled comparisons re-decided on the device from beam-order sums; the GMapping OOPE, r06: reported
  // -- error 7 -- and the match redone in the exact mode)
  a.verify = (tie_check_default(m) && !a.seq) ? 1 : 0;
  a.inert_tail = ctx->inert_tail;
  a.ctl = hc.d_chain.get();
  a.shapes = hc.d_shapes.get();
  a.n_inst = hc.shapes.packed();
  for (int k = 0; k < 3; ++k) a.init[k] = init_pose[k];
  a.dt0 = hc.dt;
  a.dr0 = hc.dr;
  a.max_failed = hc.max_failed;
  a.shape0 = hc_bucket_of(m->p_accept0);
  a.epoch = next_epoch(m->chain_epoch);
  a.host = hc.h_chain.get();
  a.trace = m->has_obs ? m->h_trace.get() : nullptr;
  a.trace_cap = m->has_obs ? m->trace_cap : 0;
  if (m->has_obs && m->debug_trace_cap > 0) a.trace_cap = std::min(a.trace_cap, m->debug_trace_cap);
  a.stamps = m->d_stamps.get();
  volatile HcHostOut *h = hc.h_chain.get();
  h->error = 0;
  h->progress = 0;
  h->tail_calls = 0;
  double t0 = MatchJob::now_us();
  const HcChainArgs a_chain = a;  // (what the chain of kernels gets: nothing of the co-resident attempt)
  const int grid = 6 * a.max_inst + 1;
  int launched = 0;
  rc = run_lone_chain(
      m, a, h, resident, t0, &launched,
      [&](ResidentLease &lease, bool *fits) -> int {
        int cap = 0, per_cu = 0, r = SLAMHIP_OK;
        if (gm) SLAMHIP_CHECK(hc_resident_gm_capacity(m->chain_nt, a.scan.n, &cap, &per_cu));
        else r = resident_capacity_pick(m, cell_model, m->chain_nt, win ? ResidentForm::Window : ResidentForm::Lone, a.scan.n,
                                        a.max_inst, grid, !win, &a.lds_consts, &cap, &per_cu);
        if (r) return r;
        // (not counted as a give-up: this matcher's grid never fits / another context of this process holds the
        // device's resident slots: the chain of kernels at once, no stall)
        if (grid > cap || !lease.take(m->device, grid, per_cu)) return SLAMHIP_OK;
        if (gm && !hc.d_rctl_gm) {
          SLAMHIP_CHECK(hc.d_rctl_gm.alloc(1));
          SLAMHIP_CHECK(hipMemsetAsync(hc.d_rctl_gm.get(), 0, sizeof(HcResidentGmCtl), ctx->stream));
        }
        if (!gm && !hc.d_rctl) {
          SLAMHIP_CHECK(hc.d_rctl.alloc(1));
          SLAMHIP_CHECK(hipMemsetAsync(hc.d_rctl.get(), 0, sizeof(HcResidentCtl), ctx->stream));  // (ordered with the launch)
        }
        // (every workgroup clears its own granules when a match starts, and this matcher's grid never changes: nothing
        // stale can carry a current tag -- hc_tag in hc_resident.hip)
        a.rctl = hc.d_rctl.get();
        a.rctl_gm = hc.d_rctl_gm.get();
        if (ctx->scan_pending.active) {
          // the RAW kernel keeps five constants per further beam in LDS where the plain one keeps three: its own query
          bool fuse = false;
          int nt_v = 0, g_v = 0;
          if (a.lds_consts && hc_resident_variant(HcResidentKey{m->chain_nt, a.max_inst, false, false, false, false, true}, &nt_v, &g_v)) {
            int cap_raw = 0;
            r = resident_capacity(m, cell_model, m->chain_nt, ResidentForm::LoneRaw, a.scan.n, true, a.max_inst, &cap_raw);
            if (r) return r;
            fuse = grid <= cap_raw;
          }
          if (fuse) {
            a.raw = ctx->scan_pending.as;
          } else {
            r = scan_assemble_now(ctx);
            if (r) return r;
          }
        }
        *fits = true;
        return SLAMHIP_OK;
      },
      [&](hipEvent_t e0, hipEvent_t e1) {
        SLAMHIP_MATCH_END(m, 2);
        const hipError_t e = gm ? launch_hc_chain_resident_gm(a, m->chain_nt, ctx->stream, e0, e1)
                                : launch_hc_chain_resident(a, cell_model, m->chain_nt, ctx->stream, e0, e1);
        SLAMHIP_MATCH_END(m, 3);
        scan_record_finish(ctx);  // (the host's copies of the raw scan's weights / factors: while the GPU runs)
        return e;
      },
      [&](bool) -> int {
        // (a raw scan the co-resident launch was to assemble -- no fit, no lease, or it gave up: the assembly kernel
        // first, as on the plain path)
        const int arc = scan_assemble_now(ctx);
        if (arc) return arc;
        // the kernel chain redoes the match from its start, under an epoch of its own
        if (win) return kChainNeedsHost;
        a = a_chain;
        a.epoch = next_epoch(m->chain_epoch);
        h->progress = 0;
        h->tail_calls = 0;
        t0 = MatchJob::now_us();
        return SLAMHIP_OK;
      },
      [&](int step, hipEvent_t e0, hipEvent_t e1) {
        return launch_hc_chain_step(a, cell_model, step, m->chain_nt, ctx->stream, e0, e1);
      },
      []() -> int {
        __builtin_ia32_pause();
        return SLAMHIP_OK;
      },
      LoneChainText{"internal: the co-resident chain ended without publishing a result", "co-resident hill-climbing chain",
                    "hill-climbing chain did not end", "hill-climbing chain kernel"});
  SLAMHIP_MATCH_END(m, 4);
  if (ctx->scan_pending.active) {
    // the RAW launch has reported: every workgroup read its beams before its first granule, the result needed every
    // granule, and the bookkeeping workgroup wrote the block behind the first super-step -- the staging buffer's turn is
    // over.  (Anything else -- an error on the way, a replay that stopped: the assembly kernel)
    const int src = (rc == SLAMHIP_OK && h->error != 1) ? scan_fused_done(ctx) : scan_assemble_now(ctx);
    if (!rc) rc = src;
  }
  if (rc) return rc;
  m->chain_launched = launched;
  if (h->error == 1) {
    set_error("internal: the device replay found no terminal round (hill-climbing chain bug)");
    return SLAMHIP_ERR_STATE;
  }
  // 2: the observer's trace outgrew its buffer (65536 scorer calls), 3: a one-run scan sat on the path.  Nothing has
  // been reported to the observer or stored in the matcher yet, so the host-driven path -- which has neither limit --
  // redoes the match.
  if (h->error == 7) return kChainUnsettled;
  if (h->error == 2 || h->error == 3) return kChainNeedsHost;
  if (gm) {
    ctx->gm_cx = h->gm_cx;
    ctx->gm_cy = h->gm_cy;
    ctx->gm_prob = h->gm_prob;
  }
  m->tail_calls = h->tail_calls;
  return lone_chain_report(m, h, launched, a.scan.n, t0, init_pose, out_delta, out_prob);
}

// ---- the many-chains driver (K matches per call, one chain per particle) ------------------------------
// All chains advance one super-step per kernel (grid.y = chain); a chain that has ended leaves the launch at
// once.  The host queues the kernels in bursts, each closed by a one-thread marker that reports how many chains
// are through, and always has the next burst queued before it waits for a marker.  Where all chains' workgroups fit the
// device at once, ONE co-resident launch runs them instead: the chains then advance independently -- no chain waits at
// a kernel boundary for the slowest one of its super-step.
struct ManyChainsText {
  const char *resident, *no_end;
};
inline void set_rctl(HcChainArgs &a, HcResidentCtl *p) { a.rctl = p; }
inline void set_rctl(HcChainArgs &a, HcResidentGmCtl *p) { a.rctl_gm = p; }

// the blocks of `s` made ready for n chains: the trees for at most `want` round instances (shape `reach`: build_shapes),
// room for n chains (capacities double from `cap0`)
template <class Set>
int many_chains_prepare(slamhip_ctx *ctx, Set &s, int n, int want, double reach, int cap0) {
  if (want != s.built_inst) {
    SLAMHIP_CHECK(hipStreamSynchronize(ctx->stream));
    const int rc = build_shapes(want, reach, s.d_shapes.get(), &s.shapes);
    if (rc) return rc;
    s.built_inst = want;
  }
  const int total = n * (6 * s.shapes.max_inst + 1);
  s.nt = total <= 256 ? 1024 : (total <= 512 ? 512 : 256);
  return grow_blocks({ctx->stream}, s.cap, (size_t)n, (size_t)cap0, [&](size_t cap) -> int {
    s.d_rctl.reset();
    s.rctl_grid = s.rctl_chains = 0;
    SLAMHIP_CHECK(s.d_ctl.alloc(cap));
    SLAMHIP_CHECK(hipMemsetAsync(s.d_ctl.get(), 0, sizeof(HcChainCtl) * cap, ctx->stream));
    SLAMHIP_CHECK(s.h_out.alloc(cap, kPinnedCoherent));
    std::memset(s.h_out.get(), 0, sizeof(HcHostOut) * cap);
    return s.stage.alloc((int)cap, ctx->stream);
  });
}

// what every many-chains call puts into its arguments: blocks, shapes, a new epoch; the chains' result blocks re-armed
template <class Set>
void many_chains_args(Set &s, int n, HcChainArgs &a) {
  a.max_inst = s.shapes.max_inst;
  a.ctl = s.d_ctl.get();
  a.inits = s.stage.d_inits();
  a.n_done = s.stage.d_n_done();
  a.shapes = s.d_shapes.get();
  a.n_inst = s.shapes.packed();
  a.epoch = next_epoch(s.epoch);
  a.host = s.h_out.get();
  volatile HcHostOut *h = s.h_out.get();
  for (int c = 0; c < n; ++c) {
    h[c].error = 0;
    h[c].progress = 0;
    h[c].tail_calls = 0;
  }
}

//   fit(lease, &fits)            capacity and the lease: the caller's own; fits = false: the kernel chains at once
//   launch_resident(e0, e1)      the ONE launch
//   launch_step(step, e0, e1)    one kernel of the chains
//   collect(c, h)                chain c's result (published under this call's epoch, no replay error)
// first_burst: the share of the expected super-steps that goes out at once.
template <class Set, class Fit, class LaunchResident, class LaunchStep, class Collect>
int run_many_chains(slamhip_ctx *ctx, ResidentPolicy &policy, Set &s, HcChainArgs &a, int n, bool resident,
                    double first_burst, bool *ran_resident_out, int *launched_out, Fit &&fit,
                    LaunchResident &&launch_resident, LaunchStep &&launch_step, Collect &&collect,
                    const ManyChainsText &text) {
  hipStream_t st = ctx->stream;
  volatile HcHostOut *h_out = s.h_out.get();
  int launched = 0, rc = SLAMHIP_OK;
  bool ran_resident = false;
  if (resident) {
    ResidentLease lease;  // (the device's resident slots may be another context's: the kernel chains at once then)
    bool fits = false;
    rc = fit(lease, &fits);
    if (rc) return rc;
    if (fits) {
      const double t_res0 = MatchJob::now_us();
      a.spin_limit = policy.spin_limit();
      if (!s.d_rctl) {
        SLAMHIP_CHECK(s.d_rctl.alloc(s.cap));
        SLAMHIP_CHECK(hipMemsetAsync(s.d_rctl.get(), 0, sizeof(*s.d_rctl.get()) * s.cap, st));  // (ordered with the launch)
      }
      if (!s.h_all_done) {
        SLAMHIP_CHECK(s.h_all_done.alloc(1, kPinnedCoherent));
        *s.h_all_done.get() = 0;
      }
      // a launch with more slots per chain than the one before meets granules no workgroup has cleared since an
      // older launch of that size: clear the block (queued in front of the launch)
      if (6 * s.shapes.max_inst + 1 > s.rctl_grid || n > s.rctl_chains)
        SLAMHIP_CHECK(hipMemsetAsync(s.d_rctl.get(), 0, sizeof(*s.d_rctl.get()) * s.cap, st));
      s.rctl_grid = 6 * s.shapes.max_inst + 1;
      s.rctl_chains = n;
      set_rctl(a, s.d_rctl.get());
      a.tag_epoch = ++s.rctl_launches;
      a.h_all_done = s.h_all_done.get();
      hipEvent_t e0, e1;
      rc = profile_event_pair(ctx, &e0, &e1);
      if (rc) return rc;
      SLAMHIP_CHECK(launch_resident(e0, e1));
      launched = 1;
      policy.note_launch();
      volatile unsigned *all_done = s.h_all_done.get();
      unsigned long long spins = 0;
      bool gave_up = false;
      for (;;) {
        if (*all_done == a.epoch) break;
        __builtin_ia32_pause();
        if ((++spins & 0xffffull) == 0) {
          // a chain that gave up publishes its own done_seq with error 4 / 5 and never counts as ended
          for (int c = 0; c < n && !gave_up; ++c)
            gave_up = h_out[c].done_seq == a.epoch && (h_out[c].error == 4 || h_out[c].error == 5);
          if (gave_up) break;
          hipError_t qe = hipStreamQuery(st);
          if (qe == hipSuccess && *all_done != a.epoch) {
            gave_up = true;  // (every workgroup has left and the chains are not through: treated like a give-up)
            break;
          }
          if (qe != hipSuccess && qe != hipErrorNotReady) return hip_fail(qe, text.resident);
        }
      }
      if (gave_up) {
        // nothing of this call has been reported: wait for the stragglers, then the kernel chains redo it
        SLAMHIP_CHECK(hipStreamSynchronize(st));
        policy.note_give_up();
        SLAMHIP_CHECK(hipMemsetAsync(s.stage.d_n_done(), 0, sizeof(unsigned), st));
        for (int c = 0; c < n; ++c) h_out[c].error = 0;
        a.rctl = nullptr;
        a.rctl_gm = nullptr;
        a.h_all_done = nullptr;
        a.debug_mute = 0;
        launched = 0;
        a.epoch = next_epoch(s.epoch);
      } else {
        ran_resident = true;
        policy.note_success(MatchJob::now_us() - t_res0);
      }
    }
  }
  auto burst = [&](int count, unsigned *seq_out) -> int {
    for (int i = 0; i < count; ++i) {
      hipEvent_t e0, e1;
      int r = profile_event_pair(ctx, &e0, &e1);
      if (r) return r;
      SLAMHIP_CHECK(launch_step(launched, e0, e1));
      ++launched;
    }
    const unsigned seq = next_epoch(ctx->seq);
    SLAMHIP_CHECK(launch_chain_marker(s.stage.d_n_done(), s.h_done_count.get(), ctx->h_done_flag.get(), seq, st));
    *seq_out = seq;
    return SLAMHIP_OK;
  };
  unsigned seq_prev = 0, seq_next = 0;
  if (!ran_resident) rc = burst(std::max(3, (int)(s.steps_avg * first_burst)), &seq_prev);
  if (rc) return rc;
  while (!ran_resident) {
    rc = burst(3, &seq_next);  // queued before the wait: the GPU never runs dry
    if (rc) return rc;
    rc = score_wait(ctx, seq_prev);
    if (rc) return rc;
    if (*(volatile unsigned *)s.h_done_count.get() >= (unsigned)n) break;
    if (launched >= (1 << 16)) {
      set_error(text.no_end);
      return SLAMHIP_ERR_STATE;
    }
    seq_prev = seq_next;
  }
  __atomic_thread_fence(__ATOMIC_ACQUIRE);
  int max_steps = 0;
  for (int c = 0; c < n; ++c) {
    const volatile HcHostOut *h = &h_out[c];
    if (h->done_seq != a.epoch) {
      set_error("internal: a chain was counted as finished without publishing its result");
      return SLAMHIP_ERR_STATE;
    }
    if (h->error == 1) {
      set_error("internal: the device replay found no terminal round (hill-climbing chain bug)");
      return SLAMHIP_ERR_STATE;
    }
    collect(c, h);
    max_steps = std::max(max_steps, (int)h->steps);
  }
  s.steps_avg = 0.75 * s.steps_avg + 0.25 * (double)max_steps;
  if (ctx->profile) ctx->prof_launches += launched;
  *ran_resident_out = ran_resident;
  *launched_out = launched;
  return SLAMHIP_OK;
}

// ---- K independent hill-climbing matches in shared launches ---------------------------------------
// PoseEnumerationScanMatcher::process_scan once per robot (pose_enumeration_scan_matcher.h:31-77; SURVEY 8e
// "replicas only"): match c = (scan c, initial pose c, map c).  The chain kernel takes the match from grid.y and
// its map / scan from a job table in HBM; everything else -- control block, replay, trace -- is per chain already
// (the filter's one-chain-per-particle launches, gm_multi_chain_run below, are the same mechanism with one map and
// one scan).  A lone match is latency-bound: 253 one-pose workgroups, one per CU, 15-18 dependent kernels.  K of them
// fill the chip: the tree of a chain shrinks with K (about kBatchWgs scoring workgroups per super-step over all
// chains), workgroups get narrower, and several chains' poses are resident per CU.

// the matcher-level conditions of chain_eligible (the per-scan ones are tested job by job)
bool batch_chain_eligible(slamhip_matcher *m) {
  if (!m->is_hc || !hc_limit_on_device(m)) return false;
  if (m->cfg.oope != SLAMHIP_OOPE_OBSTACLE || m->cfg.pose_trig != SLAMHIP_POSE_TRIG_DEVICE) return false;
  if (m->cfg.sum_order != SLAMHIP_SUM_TREE256) return false;
  if (!m->ctx->low_latency || m->ctx->stage_poses) return false;
  if (m->max_batch < 6 * kHcMaxInst) return false;
  if (m->chain_mode < 0) m->chain_mode = kChainDefaultMode;  // (slamhip_matcher_set_device_chain changes it)
  return m->chain_mode >= 1;
}

// scoring workgroups per super-step over all chains of a batch.  Measured on MI355X (cfg2 scenes, G units/s at
// K = 8): see DESIGN.md section 4d -- larger budgets buy fewer super-steps with more discarded poses.
constexpr int kBatchWgs = 1024;
constexpr int kBatchTracePer = 1 << 14;  // trace entries per chain (a longer match is redone by the single path)

// the maps of a batch's jobs, asked ONCE per call, before anything is staged or launched: bound -- and, for the shared
// launches (cell_model_out given), 1-cell and of one cell model
template <class Job>
int batch_maps_check(slamhip_ctx *ctx, int n, const Job *jobs, int *cell_model_out) {
  int cell_model = -1;
  for (int c = 0; c < n; ++c) {
    const int id = jobs[c].map_id;
    const DeviceMap *dm = (id >= 0 && id < (int)ctx->maps.size() && ctx->maps[id].bound) ? &ctx->maps[id] : nullptr;
    if (!dm) return invalid_arg("unknown map id in a match job");
    if (!cell_model_out) continue;
    if (dm->cell_model == SLAMHIP_CELL_GMAPPING) return invalid_arg("the batch form covers the 1-cell OOPE (OCC / TBM cells)");
    if (cell_model >= 0 && dm->cell_model != cell_model) return invalid_arg("the maps of one batch must share a cell model");
    cell_model = dm->cell_model;
  }
  if (cell_model_out) *cell_model_out = cell_model;
  return SLAMHIP_OK;
}

// a match's scan where it lies in HBM: five rows of `stride` doubles
struct BatchScanBlock {
  const double *d = nullptr;
  size_t stride = 0;
  int n = 0;
  double tot_w = 0;
};
// a job's map and scan in its entry of a staged job table (HcJobView, McJobView)
template <class JobView>
void fill_job_view(JobView &v, const DeviceMap &dm, const BatchScanBlock &k) {
  v.map = view_of(dm);
  v.scan = scan_view_of(k.d, k.stride, k.n, k.tot_w);
}

// The batch's scans: stored scans are read where they lie; scans handed over as host arrays go into one arena with one
// copy (the staging buffers are free: the previous batch returned after its chains had ended, i.e. long after its
// copies).  blocks: n entries out.
int hc_batch_stage_scans(slamhip_matcher *m, int n, const slamhip_match_job *jobs, BatchScanBlock *blocks) {
  slamhip_ctx *ctx = m->ctx;
  HcBatch *b = m->batch.get();
  size_t doubles = 0;
  for (int c = 0; c < n; ++c)
    if (jobs[c].scan_slot < 0) doubles += 5 * (size_t)((jobs[c].n + 7) & ~7);
  int rc = grow_block(ctx->stream, b->h_scan, b->h_scan_cap, doubles, 1 << 14, 1, hipHostMallocDefault);
  if (!rc) rc = grow_block(ctx->stream, b->d_scan, b->scan_cap, doubles, 1 << 14);
  if (rc) return rc;
  size_t at = 0;
  for (int c = 0; c < n; ++c) {
    const slamhip_match_job &j = jobs[c];
    BatchScanBlock &k = blocks[c];
    if (j.scan_slot >= 0) {
      const slamhip_ctx::ScanSlot &sl = ctx->scan_slots[j.scan_slot];
      k.d = sl.d.get();
      k.stride = (size_t)sl.cap;
      k.n = sl.n;
      k.tot_w = sl.tot_w;
    } else {
      const size_t stride = (size_t)((j.n + 7) & ~7);
      double *hs = b->h_scan.get() + at;
      const size_t bytes = sizeof(double) * (size_t)j.n;
      std::memcpy(hs, j.range, bytes);
      std::memcpy(hs + stride, j.cos_a, bytes);
      std::memcpy(hs + 2 * stride, j.sin_a, bytes);
      std::memcpy(hs + 3 * stride, j.weight, bytes);
      if (j.factor) std::memcpy(hs + 4 * stride, j.factor, bytes);
      else for (int i = 0; i < j.n; ++i) hs[4 * stride + i] = 1.0;
      double tot_w = 0;  // in beam order, pose independent (weighted_mean_point_probability_spe.h:125)
      for (int i = 0; i < j.n; ++i) tot_w += j.weight[i];
      k.d = b->d_scan.get() + at;
      k.stride = stride;
      k.n = j.n;
      k.tot_w = tot_w;
      at += 5 * stride;
    }
  }
  if (at) SLAMHIP_CHECK(hipMemcpyAsync(b->d_scan.get(), b->h_scan.get(), sizeof(double) * at, hipMemcpyHostToDevice, ctx->stream));
  return SLAMHIP_OK;
}

// The shared launches over n matches whose scans lie in HBM (blocks); a job gives its map and its initial pose
// (cell_model: batch_maps_check's answer, asked by the entry point).
template <class Job>
int hc_batch_run(slamhip_matcher *m, int n, const Job *jobs, const BatchScanBlock *blocks, int cell_model) {
  slamhip_ctx *ctx = m->ctx;
  HcBatch *b = m->batch.get();
  if (!b->d_shapes) {
    SLAMHIP_CHECK(b->d_shapes.alloc(kHcShapes));
    SLAMHIP_CHECK(b->h_done_count.alloc(1, kPinnedCoherent));
  }
  {
    // Trees and workgroups.  Up to two chains: one pose per workgroup of 1024 / 512 threads (a lone chain's form).
    // More: the chains' poses in PAIRS -- 512 threads, two poses per workgroup and super-step, which sweep, replay
    // and tabulate once for the two (hc_resident.hip) --, two workgroups per CU, the trees sized so that all chains'
    // workgroups are resident together with one CU to spare.
    if (!b->cus) SLAMHIP_CHECK(hipDeviceGetAttribute(&b->cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
    // (a chain is 6 x instances + 1 workgroups: r05 sized by 6 x instances alone, and batches of 10, 24 ... 28 matches --
    // 1030 ... 1036 workgroups against 1020 resident ones at 1080 beams -- fell back to the kernel chains)
    int want = std::min(kHcDefaultInst, std::max(1, (kBatchWgs / n - 1) / 6));
    // (measured, ms per call, pairs / one pose per 256-thread workgroup: K = 4 0.170 / 0.179, 8: 0.191 / 0.193, 16: 0.288 /
    // 0.276 -- a pair's super-step is 7 % shorter (7.4 against 8.0 us at K = 8: the beam constants fit in LDS again and
    // the sweep, the replay and the table are made once for two poses), but two workgroups per CU with a CU to spare
    // leave room for 20 instead of 21 round instances per chain at K = 8 and 10 instead of 10 at K = 16, where the
    // narrower workgroups' finer interleaving wins: pairs up to eight chains)
    // (the policy counts the calls towards its re-arm, so it is asked ONCE per call: the trees are sized
    // for the form the call will run in)
    b->resident_call = hc_resident_asked(m);
    b->pair = n * (6 * want + 1) > 512 && n <= 8 && b->resident_call && m->cfg.sum_order != SLAMHIP_SUM_SEQUENTIAL;
    if (b->pair) want = std::min(kHcDefaultInst, std::max(1, (2 * (b->cus - 1) / n - 1) / 3));
    const int rc = many_chains_prepare(ctx, *b, n, want, 0.002, 8);
    if (rc) return rc;
  }
  if (m->has_obs) {  // (one slice of kBatchTracePer entries per chain the blocks hold)
    b->trace_per = kBatchTracePer;
    const int rc = grow_block(ctx->stream, b->h_trace, b->trace_chains, b->cap, b->cap, kBatchTracePer, kPinnedCoherent);
    if (rc) return rc;
  }
  int max_n = 0;
  for (int c = 0; c < n; ++c) {
    max_n = std::max(max_n, blocks[c].n);
    fill_job_view(b->stage.h_table()[c], ctx->maps[jobs[c].map_id], blocks[c]);
    for (int q = 0; q < 3; ++q) b->stage.h_inits()[3 * c + q] = jobs[c].init_pose[q];
  }
  hipStream_t st = ctx->stream;
  // (counter = 0, initial poses, job table: one pull of the pinned block)
  SLAMHIP_CHECK(launch_block_pull(b->stage.h.get(), b->stage.d.get(), b->stage.bytes_upto_table(n), st));
  HcChainArgs a;
  std::memset(&a, 0, sizeof(a));
  a.jobs = b->stage.d_table();
  a.scan.n = max_n;  // (the launch's LDS size)
  a.oie = m->cfg.oie;
  a.gm_cx = a.gm_cy = -1;
  a.gm_prob = -1.0;
  a.verify = tie_check_default(m) ? 1 : 0;
  a.inert_tail = ctx->inert_tail;
  a.stamps = m->d_stamps.get();  // (debugging: chain 0's workgroup 1)
  a.dt0 = m->hc.dt;
  a.dr0 = m->hc.dr;
  a.max_failed = m->hc.max_failed;
  a.shape0 = hc_bucket_of(m->p_accept0);
  a.trace = m->has_obs ? b->h_trace.get() : nullptr;
  a.trace_cap = m->has_obs ? b->trace_per : 0;
  a.trace_stride = b->trace_per;
  if (m->has_obs && m->debug_trace_cap > 0) a.trace_cap = std::min(a.trace_cap, m->debug_trace_cap);
  many_chains_args(*b, n, a);
  m->tail_calls = 0;
  const int res_nt = b->pair ? 512 : b->nt;
  const int res_wgs = n * (b->pair ? 3 * b->shapes.max_inst + 1 : 6 * b->shapes.max_inst + 1);
  long long units = 0;
  bool ran_resident = false;
  int launched = 0;
  const int rc = run_many_chains(
      ctx, m->resident, *b, a, n, b->resident_call && !a.seq, 0.9, &ran_resident, &launched,
      [&](ResidentLease &lease, bool *fits) -> int {
        int cap_wgs = 0, per_cu = 0;
        const int r = resident_capacity_pick(m, cell_model, res_nt, b->pair ? ResidentForm::Pair : ResidentForm::Batch, max_n,
                                             b->shapes.max_inst, res_wgs, true, &a.lds_consts, &cap_wgs, &per_cu);
        if (r) return r;
        if (res_wgs <= cap_wgs && lease.take(m->device, res_wgs, per_cu)) {
          a.pair = b->pair ? 1 : 0;
          a.debug_mute = m->debug_resident_mute;
          *fits = true;
        }
        return SLAMHIP_OK;
      },
      [&](hipEvent_t e0, hipEvent_t e1) { return launch_hc_chain_resident(a, cell_model, res_nt, st, e0, e1, n); },
      [&](int step, hipEvent_t e0, hipEvent_t e1) { return launch_hc_chain_step(a, cell_model, step, b->nt, st, e0, e1, n); },
      [&](int c, const volatile HcHostOut *h) {
        BatchJobResult &r = b->res[c];
        r.error = h->error;
        r.on_chain = h->error == 0;
        for (int q = 0; q < 3; ++q) r.pose[q] = h->pose[q];
        r.prob = h->best_prob;
        r.calls = h->calls;
        r.evaluated = h->evaluated;
        r.rescored = h->rescored;
        r.steps = h->steps;
        m->tail_calls += h->tail_calls;
        units += h->evaluated * (long long)blocks[c].n;
      },
      ManyChainsText{"co-resident hill-climbing chains", "the batch's hill-climbing chains did not end"});
  if (rc) return rc;
  b->kernels = launched;
  if (ctx->profile) ctx->prof_units += units;
  return SLAMHIP_OK;
}

}  // namespace

namespace slamhip {

// one chain per particle over the GMapping OOPE; the staging table holds the chains' tile-pool slots (per-particle maps)
struct GmMultiChain : ChainSet<HcResidentGmCtl, int> {
  GmMultiChain() : ChainSet(14.0) {}
  int device = 0;
  ResidentPolicy resident;  // (the filter's own: not a matcher's)
};

void gm_multi_chain_free(GmMultiChain *s) {
  if (!s) return;
  hipSetDevice(s->device);
  hipDeviceSynchronize();
  delete s;
}

// (the same sizing as gm_multi_chain_run's: one round instance per chain from 47 chains on, 256-thread workgroups)
bool gm_multi_chain_fits_resident(slamhip_ctx *ctx, int n) {
  if (!ctx->resident_chains || n <= 0 || ctx->scan_n > 1280) return false;
  const int inst = std::min(kHcDefaultInst, std::max(1, 280 / (6 * n)));
  const int total = n * (6 * inst + 1);
  const int nt = total <= 256 ? 1024 : (total <= 512 ? 512 : 256);
  int cap_wgs = 0;
  if (hc_resident_gm_capacity(nt, ctx->scan_n, &cap_wgs) != hipSuccess) return false;
  return total <= cap_wgs;
}

int gm_multi_chain_run(slamhip_ctx *ctx, GmMultiChain **scratch, int map_id, const slamhip_spe_cfg *cfg,
                       unsigned max_failed, double dt, double dr, int n, const double *inits, GmChainResult *out,
                       long long *kernels_launched, const TiledTarget *tiled, const int *slots) {
  if (n <= 0) return SLAMHIP_OK;
  if (tiled && !slots) return SLAMHIP_ERR_INVALID;
  if (!*scratch) {
    GmMultiChain *s = new GmMultiChain;
    s->device = ctx->device;
    *scratch = s;
    SLAMHIP_CHECK(s->d_shapes.alloc(kHcShapes));
    SLAMHIP_CHECK(s->h_done_count.alloc(1, kPinnedCoherent));
  }
  GmMultiChain *s = *scratch;
  {
    // The tree of a chain is as large as the launch can afford: about `wgs` scoring workgroups per super-step over
    // all chains.  A hundred chains share them (one round instance each: a launch is throughput-bound, an instance
    // has to be LIKELY on the path to be worth its six workgroups); a shard of a dozen particles gets deep trees and
    // wide workgroups, like a lone matcher.  Measured (cfg4 scene, ms per step, chains / the lock-step jobs they
    // replace): 100 particles 0.74 / 0.83 (1 instance; 2: 0.87, 4: 1.12), 25: 0.45 / 0.51, 13: 0.36 / 0.48; budgets
    // of 200..300 workgroups are equal, 500 and more slower.
    // (r04, the co-resident launch: 280 / 500 / 700 / 950 workgroups give 0.304 / 0.322 / 0.369 / 0.383 ms per step
    // for a 13-particle shard and 0.443 / 0.445 / 0.477 / 0.510 for 50 -- deeper trees cost more per pose than the
    // super-steps they save here too)
    constexpr int wgs = 280;
    const int rc = many_chains_prepare(ctx, *s, n, std::min(kHcDefaultInst, std::max(1, wgs / (6 * n))), 0.01, 16);
    if (rc) return rc;
  }
  HcChainArgs a;
  std::memset(&a, 0, sizeof(a));
  int cell_model = 0;
  int rc = score_views(ctx, map_id, cfg, &a.map, &a.scan, &cell_model, tiled);
  if (rc) return rc;
  if (tiled) {
    a.tables = tiled->tables;
    a.table_stride = tiled->table_stride;
    a.slots = s->stage.d_table();
    std::memcpy(s->stage.h_table(), slots, sizeof(int) * n);
  }
  a.oie = cfg->oie;
  a.gm.fullness_th = cfg->gm_fullness_th;
  a.gm.window = cfg->gm_window;
  a.gm_cx = a.gm_cy = -1;  // every chain starts without a carry-in (the filter checks the hand-overs afterwards)
  a.gm_prob = -1.0;
  a.dt0 = dt;
  a.dr0 = dr;
  a.max_failed = max_failed;
  a.shape0 = hc_bucket_of(0.25);
  many_chains_args(*s, n, a);
  std::memcpy(s->stage.h_inits(), inits, sizeof(double) * 3 * n);
  // (counter = 0, initial poses, tile-pool slots: one pull of the pinned block)
  SLAMHIP_CHECK(launch_block_pull(s->stage.h.get(), s->stage.d.get(),
                                  tiled ? s->stage.bytes_upto_table(n) : s->stage.bytes_upto_inits(n), ctx->stream));
  // ---- ONE launch for all chains (hc_resident_gm.hip) when their workgroups fit the device at once: every
  // particle's chain then advances at its own pace instead of in lock-step launches
  const bool armed = s->resident.armed();
  const int grid = n * (6 * s->shapes.max_inst + 1);
  long long evaluated = 0;
  bool ran_resident = false;
  int launched = 0;
  rc = run_many_chains(
      ctx, s->resident, *s, a, n, ctx->resident_chains && armed && a.scan.n <= 1280, 0.8, &ran_resident, &launched,
      [&](ResidentLease &lease, bool *fits) -> int {
        int cap_wgs = 0, per_cu = 0;
        SLAMHIP_CHECK(hc_resident_gm_capacity(s->nt, a.scan.n, &cap_wgs, &per_cu));
        *fits = grid <= cap_wgs && lease.take(s->device, grid, per_cu);
        return SLAMHIP_OK;
      },
      [&](hipEvent_t e0, hipEvent_t e1) { return launch_hc_chain_resident_gm(a, s->nt, ctx->stream, e0, e1, n); },
      [&](int step, hipEvent_t e0, hipEvent_t e1) {
        return launch_hc_chain_step(a, cell_model, step, s->nt, ctx->stream, e0, e1, n);
      },
      [&](int c, const volatile HcHostOut *h) {
        GmChainResult &r = out[c];
        r.error = h->error;
        for (int k = 0; k < 3; ++k) r.pose[k] = h->pose[k];
        r.prob = h->best_prob;
        r.calls = h->calls;
        r.evaluated = h->evaluated;
        r.steps = h->steps;
        r.cx = h->gm_cx;
        r.cy = h->gm_cy;
        r.cprob = h->gm_prob;
        std::memcpy(&r.first_info, const_cast<const GmPoseInfo *>(&h->first_info), sizeof(GmPoseInfo));
        r.first_raw = h->first_raw;
        evaluated += h->evaluated;
      },
      ManyChainsText{"co-resident GMapping chains", "the filter's hill-climbing chains did not end"});
  if (rc) return rc;
  if (kernels_launched) *kernels_launched = launched;
  if (ctx->profile) ctx->prof_units += evaluated * (long long)a.scan.n;
  return SLAMHIP_OK;
}

}  // namespace slamhip

namespace {

// ---- brute force on the device (bf_device.hip) -----------------------------------------------------
// One flat sweep over the enumerator's whole pose list + a device arg-max with the reference's first-wins rule
// (brute_force_scan_matcher.h:10-81, pose_enumeration_scan_matcher.h:48-69).  Covers the point and window OOPEs in
// the default sum order with device pose trigonometry; everything else, and a sweep whose walk meets a comparison
// the tree sums cannot settle, takes the host-driven batches.
bool bf_device_eligible(slamhip_matcher *m) {
  if (!m->is_bf || m->cfg.oope == SLAMHIP_OOPE_GMAPPING || m->cfg.pose_trig != SLAMHIP_POSE_TRIG_DEVICE) return false;
  if (m->cfg.sum_order != SLAMHIP_SUM_TREE256 || !m->ctx->low_latency || m->ctx->stage_poses) return false;
  if (m->chain_mode < 0) m->chain_mode = kChainDefaultMode;
  return m->chain_mode >= 1;  // (slamhip_matcher_set_device_chain(0) keeps the host-driven batches)
}

// the enumerator's offsets on the host and in HBM, made once per matcher (kChainNeedsHost: an axis too long for a sweep)
int bf_sweep_offsets(slamhip_matcher *m) {
  slamhip_ctx *ctx = m->ctx;
  slamhip_matcher::BfSweep &bf = m->bf;
  if (bf.off.empty()) {
    // the enumerator's offsets, made by ITS additions (feedback(): x fastest, then y, then theta; each axis
    // accumulates `+= step` from `from` while the value is still below `to`; theta while t <= to)
    const double *r = bf.r;
    std::vector<double> xs, ys, ts;
    for (double x = r[0];; x += r[2]) {
      xs.push_back(x);
      if (!(x < r[1]) || xs.size() > (1u << 22)) break;
    }
    for (double y = r[3];; y += r[5]) {
      ys.push_back(y);
      if (!(y < r[4]) || ys.size() > (1u << 22)) break;
    }
    for (double t = r[6]; t <= r[7] && ts.size() <= (1u << 22); t += r[8]) ts.push_back(t);
    if (xs.size() > (1u << 22) || ys.size() > (1u << 22) || ts.size() > (1u << 22)) return kChainNeedsHost;
    bf.nx = (int)xs.size();
    bf.ny = (int)ys.size();
    bf.nt = (int)ts.size();
    bf.off = xs;
    bf.off.insert(bf.off.end(), ys.begin(), ys.end());
    bf.off.insert(bf.off.end(), ts.begin(), ts.end());
    if (bf.off.empty()) bf.off.push_back(0.0);
    SLAMHIP_CHECK(bf.d_off.alloc(bf.off.size()));
    SLAMHIP_CHECK(hipMemcpyAsync(bf.d_off.get(), bf.off.data(), sizeof(double) * bf.off.size(), hipMemcpyHostToDevice,
                                 ctx->stream));
    SLAMHIP_CHECK(hipStreamSynchronize(ctx->stream));
    SLAMHIP_CHECK(bf.h_out.alloc(1, kPinnedCoherent));
    std::memset(bf.h_out.get(), 0, sizeof(BfHostOut));
  }
  return SLAMHIP_OK;
}

// pose i of a sweep around `base` whose match started at `init` (k_bf_poses' additions)
void bf_pose_of_host(const slamhip_matcher::BfSweep &bf, const double *init, const double *base, long long i, double p3[3]) {
  p3[0] = init[0];
  p3[1] = init[1];
  p3[2] = init[2];
  if (i > 0) {
    const long long j = i - 1;
    const int ix = (int)(j % bf.nx);
    const long long r = j / bf.nx;
    const int iy = (int)(r % bf.ny), it = (int)(r / bf.ny);
    p3[0] = base[0] + bf.off[ix];
    p3[1] = base[1] + bf.off[bf.nx + iy];
    p3[2] = base[2] + bf.off[bf.nx + bf.ny + it];
  }
}

// the observer's events of one sweep in the reference's order, from its score array (:43-46, :53-60); on_matching_end
// is the caller's
void bf_replay_scores(const slamhip_observer &obs, const slamhip_matcher::BfSweep &bf, const double *init, const double *base,
                      const double *sc, long long n) {
  double b = sc[0];
  double p3[3];
  bf_pose_of_host(bf, init, base, 0, p3);
  if (obs.on_scan_test) obs.on_scan_test(obs.user, p3, sc[0]);
  if (obs.on_pose_update) obs.on_pose_update(obs.user, p3, sc[0]);
  for (long long i = 1; i < n; ++i) {
    bf_pose_of_host(bf, init, base, i, p3);
    if (obs.on_scan_test) obs.on_scan_test(obs.user, p3, sc[i]);
    if (b < sc[i]) {
      b = sc[i];
      if (obs.on_pose_update) obs.on_pose_update(obs.user, p3, sc[i]);
    }
  }
}

int bf_device_process_scan(slamhip_matcher *m, int map_id, const double init_pose[3], double out_delta[3],
                           double *out_prob) {
  slamhip_ctx *ctx = m->ctx;
  slamhip_matcher::BfSweep &bf = m->bf;
  {
    const int prc = bf_sweep_offsets(m);
    if (prc) return prc;
  }
  const long long n = 1 + (long long)bf.nx * bf.ny * bf.nt;
  if (n > (1ll << 26)) return kChainNeedsHost;
  if (n > bf.cap) {
    SLAMHIP_CHECK(hipStreamSynchronize(ctx->stream));
    bf.cap = 0;
    const long long blocks = (n + 1023) / 1024;
    SLAMHIP_CHECK(bf.d_poses.alloc(3 * n));
    SLAMHIP_CHECK(bf.d_scores.alloc(n));
    SLAMHIP_CHECK(bf.d_fp.alloc(n));
    SLAMHIP_CHECK(bf.d_pidx.alloc(n));
    SLAMHIP_CHECK(bf.d_agg_s.alloc(blocks));
    SLAMHIP_CHECK(bf.d_agg_i.alloc(blocks));
    if (!bf.d_counters) {
      SLAMHIP_CHECK(bf.d_counters.alloc(4));
      SLAMHIP_CHECK(hipMemsetAsync(bf.d_counters.get(), 0, sizeof(unsigned) * 4, ctx->stream));
    }
    bf.cap = n;
  }
  ScoreArgs a;
  std::memset(&a, 0, sizeof(a));
  int cell_model = 0, oie_eff = m->cfg.oie;
  int rc = score_views(ctx, map_id, &m->cfg, &a.map, &a.scan, &cell_model, nullptr, &oie_eff);  // (TBM: through the plane)
  if (rc) return rc;
  (void)tie_check_default(m);
  const bool verify = m->tie_check == 1;  // (the GMapping OOPE never gets here: bf_device_eligible)
  const double t0 = MatchJob::now_us();
  // (the enumerator object stays the one source of the latched base pose: a match that falls back to the host-driven
  // batches enumerates around the same pose)
  const Pose base = static_cast<BruteForcePoseEnumerator *>(m->pe.get())->latch_base(Pose{init_pose[0], init_pose[1], init_pose[2]});
  const double base3[3] = {base.x, base.y, base.theta};
  BfPoseArgs pa;
  for (int k = 0; k < 3; ++k) {
    pa.init[k] = init_pose[k];
    pa.base[k] = base3[k];
  }
  pa.off = bf.d_off.get();
  pa.nx = bf.nx;
  pa.ny = bf.ny;
  pa.nt = bf.nt;
  pa.n = n;
  pa.poses = bf.d_poses.get();
  SLAMHIP_CHECK(launch_bf_poses(pa, ctx->stream));
  a.poses = bf.d_poses.get();
  a.scores = bf.d_scores.get();
  a.n_poses = (int)n;
  a.oie = oie_eff;
  for (int k = 0; k < 4; ++k) a.area[k] = m->cfg.area[k];
  a.gm.fullness_th = m->cfg.gm_fullness_th;
  a.gm.window = m->cfg.gm_window;
  a.fprints = verify ? bf.d_fp.get() : nullptr;
  hipEvent_t e0, e1;
  rc = profile_event_pair(ctx, &e0, &e1);
  if (rc) return rc;
  SLAMHIP_CHECK(launch_score(a, cell_model, m->cfg.oope, m->cfg.sum_order, ctx->stream, e0, e1));
  const unsigned seq = next_epoch(bf.seq);
  BfArgmaxArgs ga;
  ga.scores = bf.d_scores.get();
  ga.fprints = verify ? bf.d_fp.get() : nullptr;
  ga.n = n;
  ga.verify = verify ? 1 : 0;
  ga.out = bf.h_out.get();
  ga.seq = seq;
  ga.pidx = bf.d_pidx.get();
  ga.agg_s = bf.d_agg_s.get();
  ga.agg_i = bf.d_agg_i.get();
  ga.counters = bf.d_counters.get();
  if (n < 2) return kChainNeedsHost;  // (no candidate at all: nothing for the sweep to do)
  SLAMHIP_CHECK(launch_bf_argmax(ga, ctx->stream));
  if (m->has_obs) {
    bf.scores_host.resize((size_t)n);
    SLAMHIP_CHECK(hipMemcpyAsync(bf.scores_host.data(), bf.d_scores.get(), sizeof(double) * n, hipMemcpyDeviceToHost,
                                 ctx->stream));
  }
  volatile BfHostOut *h = bf.h_out.get();
  unsigned long long spins = 0;
  while (h->seq != seq) {
    __builtin_ia32_pause();
    if ((++spins & 0xfffffull) == 0) {
      hipError_t qe = hipStreamQuery(ctx->stream);
      if (qe != hipSuccess && qe != hipErrorNotReady) return hip_fail(qe, "brute-force sweep");
    }
  }
  __atomic_thread_fence(__ATOMIC_ACQUIRE);
  if (m->has_obs) SLAMHIP_CHECK(hipStreamSynchronize(ctx->stream));
  if (ctx->profile) {
    ctx->prof_launches += 1;
    ctx->prof_units += n * (long long)a.scan.n;
  }
  if (h->ambiguous) return kChainNeedsHost;  // nothing reported yet: the host-driven batches settle it
  double best[3];
  bf_pose_of_host(bf, init_pose, base3, h->best_index, best);
  for (int k = 0; k < 3; ++k) out_delta[k] = best[k] - init_pose[k];
  *out_prob = h->best_score;
  MatchJob &job = m->job;
  job.scorer_calls = n;
  job.poses_evaluated = n;
  job.launches = 1;
  job.t_build_us = job.t_replay_us = 0;
  m->chain_launched = 4;  // poses, sweep, scan, decide
  m->chain_rescored = 0;
  m->tail_calls = 0;
  m->t_stage_us = 0;
  m->t_score_us = MatchJob::now_us() - t0;
  if (m->has_obs) {
    // the observer's events in the reference's order, from the score array (:43-46, :53-60)
    const double t1 = MatchJob::now_us();
    bf_replay_scores(m->obs, bf, init_pose, base3, bf.scores_host.data(), n);
    job.t_replay_us = MatchJob::now_us() - t1;
    if (m->obs.on_matching_end) m->obs.on_matching_end(m->obs.user, out_delta, *out_prob);
  }
  return SLAMHIP_OK;
}

// ---- Monte Carlo on the device (mc_chain.hip) -------------------------------------------------------
// the 1-cell OOPE with device pose trigonometry on the zero-copy path, like the hill-climbing chain
bool mc_chain_eligible(slamhip_matcher *m) {
  if (!m->is_mc) return false;
  if (m->cfg.oope != SLAMHIP_OOPE_OBSTACLE || m->cfg.pose_trig != SLAMHIP_POSE_TRIG_DEVICE) return false;
  if (!m->ctx->low_latency || m->ctx->stage_poses) return false;
  if (m->ctx->scan_n > 4096) return false;  // (see chain_eligible)
  if (m->max_batch < 64) return false;  // slamhip_matcher_set_batch asked for small batches
  if (m->chain_mode < 0) m->chain_mode = kChainDefaultMode;  // (slamhip_matcher_set_device_chain changes it)
  return m->chain_mode >= 1;
}

// pairs of the tape one match can consume: three pairs per two candidates, and every reset_shift (at most one per
// max_failed / 3 + 1 candidates) may drop a triple's second half
size_t mc_tape_need(const GaussianPoseEnumerator *pe) {
  const size_t max_poses = pe->max_poses();
  const size_t resets = max_poses / (pe->max_failed() / 3 + 1) + 2;
  return 3 * (max_poses / 2 + 2 + resets) + 8;
}

int mc_chain_process_scan(slamhip_matcher *m, int map_id, const double init_pose[3], double out_delta[3],
                          double *out_prob) {
  slamhip_ctx *ctx = m->ctx;
  slamhip_matcher::McChain &mc = m->mc;
  auto *pe = static_cast<GaussianPoseEnumerator *>(m->pe.get());
  if (!mc.d_mc) {
    SLAMHIP_CHECK(mc.d_mc.alloc(1));
    SLAMHIP_CHECK(hipMemsetAsync(mc.d_mc.get(), 0, sizeof(McChainCtl), ctx->stream));
    SLAMHIP_CHECK(mc.h_mc.alloc(1, kPinnedCoherent));
    std::memset(mc.h_mc.get(), 0, sizeof(McHostOut));
  }
  // 511 candidates per super-step in workgroups of 512 threads (with the bookkeeping workgroup two on EVERY CU): a
  // Monte-Carlo chain is a long run of rejections, so the larger tree pays (r03: 384 x 512 threads against 252 x 1024,
  // 16 super-steps of 7.2 us against 21 of 6.5; r05: 511 against 384, mc_chain_device.h).  slamhip_matcher_set_batch
  // caps it (at least 64: mc_chain_eligible).
  mc.slots = std::min(kMcSlots, m->max_batch);
  McChainArgs a;
  std::memset(&a, 0, sizeof(a));
  int cell_model = 0, oie_eff = m->cfg.oie;
  int rc = score_views(ctx, map_id, &m->cfg, &a.map, &a.scan, &cell_model, nullptr, &oie_eff);  // (TBM: through the plane)
  if (rc) return rc;
  // the enumerator is reset when a match starts (pose_enumeration_scan_matcher.h:47): what carries over from
  // match to match is the engine, i.e. the position on the pair tape.
  pe->reset();
  const size_t max_poses = pe->max_poses();
  const size_t need = mc_tape_need(pe);
  // The pairs live in HBM as a window [tape_base, tape_base + tape_filled) of the tape, filled AHEAD: while a
  // chain runs, the host (spinning anyway) generates the pairs of the next match and a side stream uploads them,
  // so a match in steady state starts without touching the tape.  The window is restarted when it runs out.
  const double t0 = MatchJob::now_us();
  const size_t pos = pe->tape_pos();
  if (!mc.tape_stream) {
    SLAMHIP_CHECK(hipStreamCreateWithFlags(&mc.tape_stream, hipStreamNonBlocking));
    SLAMHIP_CHECK(hipEventCreateWithFlags(&mc.tape_ready, hipEventDisableTiming));
  }
  auto upload_upto = [&](size_t abs_end) -> int {  // pairs [tape_base + tape_filled, abs_end) -> HBM, asynchronously
    const size_t have = mc.tape_base + mc.tape_filled;
    if (abs_end <= have) return SLAMHIP_OK;
    const size_t cnt = abs_end - have;
    double *dst = mc.h_tape.get() + 2 * mc.tape_filled;
    pe->copy_tape_abs(have, cnt, dst);
    SLAMHIP_CHECK(hipMemcpyAsync(mc.d_tape.get() + mc.tape_filled, dst, sizeof(McPair) * cnt, hipMemcpyHostToDevice,
                                 mc.tape_stream));
    SLAMHIP_CHECK(hipEventRecord(mc.tape_ready, mc.tape_stream));
    mc.tape_filled += cnt;
    return SLAMHIP_OK;
  };
  if (!mc.d_tape || mc.tape_owner != pe || pos < mc.tape_base || pos + need > mc.tape_base + mc.tape_cap) {
    // (re)start the window at the current position (of THIS enumerator's tape: a batch call's fall-back runs a job on
    // its engine stream, swapped in for the call)
    mc.tape_owner = pe;
    SLAMHIP_CHECK(hipStreamSynchronize(ctx->stream));
    SLAMHIP_CHECK(hipStreamSynchronize(mc.tape_stream));
    static_assert(sizeof(McPair) == 2 * sizeof(double), "the pinned staging holds pairs as two doubles");
    const size_t want = std::max<size_t>(64 * need, 1 << 16);  // (exactly: the floor is the size itself)
    const int grc = grow_blocks({ctx->stream, mc.tape_stream}, mc.tape_cap, want, want, [&](size_t cap) -> int {
      SLAMHIP_CHECK(mc.d_tape.alloc(cap));
      SLAMHIP_CHECK(mc.h_tape.alloc(2 * cap, hipHostMallocDefault));
      return SLAMHIP_OK;
    });
    if (grc) return grc;
    mc.tape_base = pos;
    mc.tape_filled = 0;
  }
  rc = upload_upto(pos + need);  // nothing to do when the last match filled ahead
  if (rc) return rc;
  SLAMHIP_CHECK(hipStreamWaitEvent(ctx->stream, mc.tape_ready, 0));
  m->t_stage_us = MatchJob::now_us() - t0;
  const size_t trace_need = max_poses + 2;
  if (m->has_obs && (!m->h_trace || (size_t)m->trace_cap < trace_need)) {
    m->trace_cap = (int)std::max<size_t>(1 << 16, trace_need);
    SLAMHIP_CHECK(m->h_trace.alloc(m->trace_cap, kPinnedCoherent));
  }
  static_assert(sizeof(McTraceEntry) == sizeof(HcTraceEntry), "one trace buffer serves both chains");
  a.oie = oie_eff;
  a.seq = m->cfg.sum_order == SLAMHIP_SUM_SEQUENTIAL ? 1 : 0;
  a.verify = (tie_check_default(m) && !a.seq) ? 1 : 0;
  a.ctl = mc.d_mc.get();
  a.tape = mc.d_tape.get() + (pos - mc.tape_base);
  a.n_slots = mc.slots;
  for (int k = 0; k < 3; ++k) a.init[k] = init_pose[k];
  a.td0 = pe->base_td();
  a.rd0 = pe->base_rd();
  a.max_failed = pe->max_failed();
  a.max_poses = pe->max_poses();
  a.epoch = next_epoch(m->chain_epoch);
  a.host = mc.h_mc.get();
  a.trace = m->has_obs ? reinterpret_cast<McTraceEntry *>(m->h_trace.get()) : nullptr;
  a.trace_cap = m->has_obs ? m->trace_cap : 0;
  volatile McHostOut *h = mc.h_mc.get();
  h->error = 0;
  h->progress = 0;
  bool ahead_done = false;
  // polar pairs of the next match while this one runs: generated a few at a time, uploaded once they are there
  auto fill_ahead = [&]() -> int {
    if (ahead_done) {
      __builtin_ia32_pause();
      return SLAMHIP_OK;
    }
    pe->prefetch_ahead(2 * need, 32);
    if (pe->tape_generated_upto() >= pos + 2 * need) {
      if (pos + 2 * need <= mc.tape_base + mc.tape_cap) {
        int r = upload_upto(pos + 2 * need);
        if (r) return r;
      }
      ahead_done = true;
    }
    return SLAMHIP_OK;
  };
  // (the policy is asked once per match, whatever the mode: every match counts towards the re-arm)
  const bool armed = m->resident.armed();
  int launched = 0;
  rc = run_lone_chain(
      m, a, h, m->chain_mode == 2 && armed, t0, &launched,
      [&](ResidentLease &lease, bool *fits) -> int {
        int cap = 0, per_cu = 0;
        // (1024-thread workgroups are resident one per CU: 252 candidates per super-step then, like the hill-climbing tree)
        if (m->chain_nt == 1024) a.n_slots = std::min(a.n_slots, 252);
        a.lds_consts = 1;
        int r = resident_capacity(m, cell_model, m->chain_nt, ResidentForm::MonteCarlo, a.scan.n, true, 0, &cap, &per_cu);
        if (r) return r;
        if (a.n_slots + 1 > cap) {  // (fewer workgroups fit with the beam constants in LDS than without?)
          int cap_plain = 0, pc_plain = 0;
          r = resident_capacity(m, cell_model, m->chain_nt, ResidentForm::MonteCarlo, a.scan.n, false, 0, &cap_plain, &pc_plain);
          if (r) return r;
          if (cap_plain > cap) {
            a.lds_consts = 0;
            cap = cap_plain;
            per_cu = pc_plain;
          }
        }
        // (the capacity leaves one CU's worth of workgroups free: 509 candidates + the bookkeeping workgroup on an MI355X)
        a.n_slots = std::min(a.n_slots, cap - 1);
        if (a.n_slots < 64 || !lease.take(m->device, a.n_slots + 1, per_cu)) return SLAMHIP_OK;
        if (!mc.d_rctl) {
          SLAMHIP_CHECK(mc.d_rctl.alloc(1));
          SLAMHIP_CHECK(hipMemsetAsync(mc.d_rctl.get(), 0, sizeof(McResidentCtl), ctx->stream));  // (ordered with the launch)
        }
        // (every workgroup clears its own granules when a match starts; a launch with MORE slots than the one before --
        // the workgroup size or the batch limit was changed -- could meet what a slot held sixteen launches ago before
        // its owner has started: the block is cleared then, hc_tag in hc_resident_device.h)
        if (a.n_slots + 1 > mc.rctl_grid && mc.rctl_grid > 0)
          SLAMHIP_CHECK(hipMemsetAsync(mc.d_rctl.get(), 0, sizeof(McResidentCtl), ctx->stream));
        mc.rctl_grid = a.n_slots + 1;
        a.rctl = mc.d_rctl.get();
        a.stamps = m->d_stamps.get();
        *fits = true;
        return SLAMHIP_OK;
      },
      [&](hipEvent_t e0, hipEvent_t e1) { return launch_mc_chain_resident(a, cell_model, m->chain_nt, ctx->stream, e0, e1); },
      [&](bool gave_up) -> int {
        // nothing has been reported and the enumerator has not been touched: the chain of kernels runs the match with
        // the matcher's own candidate count -- after a launch that gave up, under a new epoch
        if (gave_up) a.epoch = next_epoch(m->chain_epoch);
        a.n_slots = mc.slots;
        return SLAMHIP_OK;
      },
      [&](int step, hipEvent_t e0, hipEvent_t e1) {
        return launch_mc_chain_step(a, cell_model, step, m->chain_nt, ctx->stream, e0, e1);
      },
      fill_ahead,
      LoneChainText{"internal: the co-resident Monte-Carlo chain ended without publishing a result",
                    "co-resident Monte-Carlo chain", "Monte-Carlo chain did not end", "Monte-Carlo chain kernel"});
  if (rc) return rc;
  // the observer's trace outgrew its buffer: the enumerator has not been touched yet (set_chain_result below),
  // the host-driven path redoes the match from the same engine position
  if (h->error == 2) return kChainNeedsHost;
  if ((size_t)h->tape_pos + 3 > need) {
    set_error("internal: the Monte-Carlo chain ran past the uploaded window of the pair tape");
    return SLAMHIP_ERR_STATE;
  }
  {
    const double saved[3] = {h->saved[0], h->saved[1], h->saved[2]};
    pe->set_chain_result((size_t)h->tape_pos, h->failed, h->poses, h->td, h->rd, h->has_saved != 0, saved);
    pe->trim();
  }
  m->tail_calls = 0;
  return lone_chain_report(m, h, launched, a.scan.n, t0, init_pose, out_delta, out_prob);
}

// ---- K independent Monte-Carlo matches in shared launches -----------------------------------------
// MonteCarloScanMatcher::process_scan once per robot, every robot on ITS engine (init_scan_matching.h:118-135: each
// matcher object owns a GaussianPoseEnumerator{mt19937(seed)}): match c = (scan c, initial pose c, map c, stream c).
// A lone match at the reference's preset (20 failed / 100 poses) can speculate on at most 20 candidates per super-step,
// so K chains advancing together -- one kernel = one super-step of every chain still alive, grid.y = chain -- are what
// fills the device.  The driver is run_many_chains' burst pattern: kernels queued in bursts, each closed by the marker,
// the next burst queued before the wait.

// the matcher-level conditions of the shared Monte-Carlo launches: mc_chain_eligible's (without the context's current
// scan, which a batch does not use) and the canonical sum -- the beam-order sum stays with the lone route
bool mc_batch_eligible(slamhip_matcher *m) {
  if (!m->is_mc || m->mc_streams.empty()) return false;
  if (m->cfg.oope != SLAMHIP_OOPE_OBSTACLE || m->cfg.pose_trig != SLAMHIP_POSE_TRIG_DEVICE) return false;
  if (m->cfg.sum_order != SLAMHIP_SUM_TREE256) return false;
  if (!m->ctx->low_latency || m->ctx->stage_poses) return false;
  if (m->max_batch < 64) return false;
  if (m->chain_mode < 0) m->chain_mode = kChainDefaultMode;
  return m->chain_mode >= 1;
}

// Workgroups per launch over all chains: the element-wise rule of thumb (about 2048 blocks keep every CU of an MI355X
// busy with several workgroups without a long tail).  Candidates per job and super-step:
//   S = min(kMcSlots, max_failed, max_poses, kMcBatchWgs / K - 1)
// -- slots beyond max_failed (or max_poses) can never hold a candidate (mc_available), and K x (S + 1) workgroups stay
// within the budget.  A speed knob only: the replay consumes min(available, S) candidates whatever S is.
constexpr int kMcBatchWgs = 2048;

int mc_batch_slots(const slamhip_matcher *m, int n, unsigned max_failed, unsigned max_poses) {
  if (m->debug_mc_batch_slots > 0) return std::min(kMcSlots, m->debug_mc_batch_slots);
  long long s = std::min<long long>(kMcSlots, std::min<long long>(max_failed, max_poses));
  s = std::min<long long>(s, kMcBatchWgs / n - 1);
  return (int)std::max<long long>(1, s);
}

// The shared launches over n matches whose scans lie in HBM (blocks); job c gives its map and initial pose and runs on
// engine stream streams[c].  Results go to m->batch->res[c]; a chain whose trace outgrew its slice is left to the lone
// route (on_chain false, its stream as it was).
template <class Job>
int mc_batch_run(slamhip_matcher *m, int n, const Job *jobs, const BatchScanBlock *blocks, const int *streams,
                 int cell_model) {
  slamhip_ctx *ctx = m->ctx;
  hipStream_t st = ctx->stream;
  if (!m->mc_batch) m->mc_batch = std::make_unique<McBatch>();
  McBatch *s = m->mc_batch.get();
  auto stream_pe = [&](int c) { return static_cast<GaussianPoseEnumerator *>(m->mc_streams[streams[c]].pe.get()); };
  const GaussianPoseEnumerator *pe0 = stream_pe(0);
  const unsigned max_failed = pe0->max_failed(), max_poses = pe0->max_poses();
  const size_t need = mc_tape_need(pe0);
  if (!s->h_done_count) SLAMHIP_CHECK(s->h_done_count.alloc(1, kPinnedCoherent));
  int grc = grow_blocks({st}, s->cap, (size_t)n, 8, [&](size_t cap) -> int {
    SLAMHIP_CHECK(s->d_ctl.alloc(cap));
    SLAMHIP_CHECK(hipMemsetAsync(s->d_ctl.get(), 0, sizeof(McChainCtl) * cap, st));
    SLAMHIP_CHECK(s->h_out.alloc(cap, kPinnedCoherent));
    std::memset(s->h_out.get(), 0, sizeof(McHostOut) * cap);
    return s->stage.alloc((int)cap, st);
  });
  static_assert(sizeof(McPair) == 2 * sizeof(double), "the pinned staging holds pairs as two doubles");
  if (!grc) grc = grow_block(st, s->d_tape, s->tape_cap, (size_t)n * need, 1 << 14);
  if (!grc) grc = grow_block(st, s->h_tape, s->h_tape_cap, (size_t)n * need, 1 << 14, 2, hipHostMallocDefault);
  if (grc) return grc;
  const size_t trace_need = (size_t)max_poses + 2;
  if (m->has_obs) {  // (one slice of trace_per entries per chain the blocks hold)
    if (s->trace_per < trace_need) {  // (slices too short for these matches: all of them anew)
      s->trace_chains = 0;
      s->trace_per = trace_need;
    }
    grc = grow_block(st, s->h_trace, s->trace_chains, s->cap, s->cap, s->trace_per, kPinnedCoherent);
    if (grc) return grc;
  }
  // every job's enumerator starts its match (pose_enumeration_scan_matcher.h:47); the windows of the K tapes in ONE
  // arena, one copy (the arena is free: the call before returned after its chains had ended)
  int max_n = 0;
  for (int c = 0; c < n; ++c) {
    GaussianPoseEnumerator *pe = stream_pe(c);
    pe->reset();
    pe->copy_tape_abs(pe->tape_pos(), need, s->h_tape.get() + 2 * need * (size_t)c);
    max_n = std::max(max_n, blocks[c].n);
  }
  SLAMHIP_CHECK(hipMemcpyAsync(s->d_tape.get(), s->h_tape.get(), sizeof(McPair) * need * (size_t)n, hipMemcpyHostToDevice, st));
  for (int c = 0; c < n; ++c) {
    const Job &j = jobs[c];
    McJobView &v = s->stage.h_table()[c];
    fill_job_view(v, ctx->maps[j.map_id], blocks[c]);
    v.tape = s->d_tape.get() + need * (size_t)c;
    for (int q = 0; q < 3; ++q) v.init[q] = j.init_pose[q];
    v.trace = m->has_obs ? s->h_trace.get() + s->trace_per * (size_t)c : nullptr;
  }
  // (counter = 0, job table with the initial poses: one pull of the pinned block)
  SLAMHIP_CHECK(launch_block_pull(s->stage.h.get(), s->stage.d.get(), s->stage.bytes_upto_table(n), st));
  McChainArgs a;
  std::memset(&a, 0, sizeof(a));
  a.jobs = s->stage.d_table();
  a.n_done = s->stage.d_n_done();
  a.scan.n = max_n;  // (the launch's LDS size)
  a.oie = m->cfg.oie;
  a.verify = tie_check_default(m) ? 1 : 0;
  a.ctl = s->d_ctl.get();
  a.n_slots = s->slots = mc_batch_slots(m, n, max_failed, max_poses);
  a.td0 = pe0->base_td();
  a.rd0 = pe0->base_rd();
  a.max_failed = max_failed;
  a.max_poses = max_poses;
  a.epoch = next_epoch(s->epoch);
  a.host = s->h_out.get();
  a.trace_cap = m->has_obs ? (int)s->trace_per : 0;
  if (m->has_obs && m->debug_trace_cap > 0) a.trace_cap = std::min(a.trace_cap, m->debug_trace_cap);
  volatile McHostOut *h_out = s->h_out.get();
  for (int c = 0; c < n; ++c) {
    h_out[c].error = 0;
    h_out[c].progress = 0;
  }
  int launched = 0;
  auto burst = [&](int count, unsigned *seq_out) -> int {
    for (int i = 0; i < count; ++i) {
      hipEvent_t e0, e1;
      const int r = profile_event_pair(ctx, &e0, &e1);
      if (r) return r;
      SLAMHIP_CHECK(launch_mc_chain_step(a, cell_model, launched, m->chain_nt, st, e0, e1, n));
      ++launched;
    }
    const unsigned seq = next_epoch(ctx->seq);
    SLAMHIP_CHECK(launch_chain_marker(s->stage.d_n_done(), s->h_done_count.get(), ctx->h_done_flag.get(), seq, st));
    *seq_out = seq;
    return SLAMHIP_OK;
  };
  unsigned seq_prev = 0, seq_next = 0;
  int rc = burst(std::max(2, (int)(s->kernels_avg * 0.9)), &seq_prev);
  if (rc) return rc;
  for (;;) {
    rc = burst(2, &seq_next);  // queued before the wait: the GPU never runs dry
    if (rc) return rc;
    rc = score_wait(ctx, seq_prev);
    if (rc) return rc;
    if (*(volatile unsigned *)s->h_done_count.get() >= (unsigned)n) break;
    if (launched >= (1 << 16)) {
      set_error("the batch's Monte-Carlo chains did not end");
      return SLAMHIP_ERR_STATE;
    }
    seq_prev = seq_next;
  }
  __atomic_thread_fence(__ATOMIC_ACQUIRE);
  HcBatch *b = m->batch.get();
  long long units = 0;
  int max_steps = 0;
  for (int c = 0; c < n; ++c) {
    const volatile McHostOut *h = &h_out[c];
    if (h->done_seq != a.epoch) {
      set_error("internal: a Monte-Carlo chain was counted as finished without publishing its result");
      return SLAMHIP_ERR_STATE;
    }
    max_steps = std::max(max_steps, (int)h->steps);
    BatchJobResult &r = b->res[c];
    r.error = h->error;
    r.on_chain = h->error == 0;
    units += h->evaluated * (long long)blocks[c].n;
    if (!r.on_chain) continue;  // (2: the trace outgrew its slice -- nothing reported, the stream not advanced)
    if ((size_t)h->tape_pos + 3 > need) {
      set_error("internal: a Monte-Carlo chain ran past the uploaded window of its pair tape");
      return SLAMHIP_ERR_STATE;
    }
    const double saved[3] = {h->saved[0], h->saved[1], h->saved[2]};
    GaussianPoseEnumerator *pe = stream_pe(c);
    pe->set_chain_result((size_t)h->tape_pos, h->failed, h->poses, h->td, h->rd, h->has_saved != 0, saved);
    pe->trim();
    ++m->mc_streams[streams[c]].matches;
    for (int q = 0; q < 3; ++q) r.pose[q] = h->pose[q];
    r.prob = h->best_prob;
    r.calls = h->calls;
    r.evaluated = h->evaluated;
    r.rescored = h->rescored;
    r.steps = h->steps;
  }
  s->kernels_avg = 0.75 * s->kernels_avg + 0.25 * (double)(max_steps + 1);
  b->kernels = launched;
  if (ctx->profile) {
    ctx->prof_launches += launched;
    ctx->prof_units += units;
  }
  return SLAMHIP_OK;
}

// the engine stream of every job of a batch call (slamhip_matcher_set_mc_job_streams; none set: job j on stream j),
// checked before anything is staged or launched
int mc_job_streams_of(const slamhip_matcher *m, int n_jobs, std::vector<int> *out) {
  const int ns = (int)m->mc_streams.size();
  if (n_jobs > ns) return invalid_arg("more jobs than engine streams (slamhip_matcher_set_mc_streams)");
  if (!m->mc_job_streams.empty() && n_jobs > (int)m->mc_job_streams.size())
    return invalid_arg("more jobs than slamhip_matcher_set_mc_job_streams named streams for");
  out->resize(n_jobs);
  std::vector<char> used(ns, 0);
  for (int c = 0; c < n_jobs; ++c) {
    const int k = m->mc_job_streams.empty() ? c : m->mc_job_streams[c];
    if (k < 0 || k >= ns) return invalid_arg("a job's engine stream is out of range");
    if (used[k]) return invalid_arg("two jobs of one batch on the same engine stream");
    used[k] = 1;
    (*out)[c] = k;
  }
  return SLAMHIP_OK;
}

// ---- K brute-force sweeps in three shared launches (bf_batch.hip) ---------------------------------------------
// BruteForceScanMatcher::process_scan once per robot: job c = (scan c, initial pose c, map c) on enumerator stream
// streams[c] (slamhip_matcher_set_bf_streams).  A brute-force enumerator hands out the same poses whatever the scorer
// says, so nothing is speculated: the K sweeps are one grid (grid.y = job) through score, scan and decide, and ONE
// completion word tells the host that all K results lie in the pinned array.

// the matcher-level conditions of the shared sweeps: the lone sweep's (bf_device_eligible) over the 1-cell OOPE, with
// enumerator streams set
bool bf_batch_eligible(slamhip_matcher *m) {
  if (!m->is_bf || !m->bf_streams.any()) return false;
  if (m->cfg.oope != SLAMHIP_OOPE_OBSTACLE) return false;
  return bf_device_eligible(m);
}

// whether the shared sweeps take n jobs of this matcher: its offsets made, K x n within the scratch budget
int bf_batch_fits(slamhip_matcher *m, int n_jobs, bool *fits) {
  *fits = false;
  const int rc = bf_sweep_offsets(m);
  if (rc == kChainNeedsHost) return SLAMHIP_OK;
  if (rc) return rc;
  const long long n = 1 + (long long)m->bf.nx * m->bf.ny * m->bf.nt;
  *fits = n >= 2 && n <= (1ll << 26) && n_jobs <= 65535 && (long long)n_jobs * n <= kBfBatchMaxPoses;
  return SLAMHIP_OK;
}

// The shared launches over n matches whose scans lie in HBM (blocks); job c gives its map and initial pose and runs on
// enumerator stream streams[c].  Everything that can fail for the caller's arguments has been checked (the entry
// points), the views and the blocks are made before a stream latches its base.  Results go to m->batch->res[c]; a job
// whose walk met a comparison the tree sums cannot settle is left to the lone route (on_chain false, error 4).
template <class Job>
int bf_batch_run(slamhip_matcher *m, int n, const Job *jobs, const BatchScanBlock *blocks, const int *streams) {
  slamhip_ctx *ctx = m->ctx;
  hipStream_t st = ctx->stream;
  slamhip_matcher::BfSweep &bf = m->bf;
  if (!m->bf_batch) m->bf_batch = std::make_unique<BfBatch>();
  BfBatch *s = m->bf_batch.get();
  const long long np = 1 + (long long)bf.nx * bf.ny * bf.nt;
  const long long per_blk = (np - 1 + 1023) / 1024;
  int grc = grow_blocks({st}, s->job_cap, (size_t)n, 8, [&](size_t cap) -> int {
    SLAMHIP_CHECK(s->h_jobs.alloc(cap, hipHostMallocDefault));
    SLAMHIP_CHECK(s->d_jobs.alloc(cap));
    SLAMHIP_CHECK(s->d_counters.alloc(3 * (size_t)cap + 1));
    SLAMHIP_CHECK(hipMemsetAsync(s->d_counters.get(), 0, sizeof(unsigned) * (3 * (size_t)cap + 1), st));
    SLAMHIP_CHECK(s->h_out.alloc(cap, kPinnedCoherent));
    std::memset(s->h_out.get(), 0, sizeof(BfHostOut) * cap);
    if (!s->h_done) {
      SLAMHIP_CHECK(s->h_done.alloc(1, kPinnedCoherent));
      *s->h_done.get() = 0;
    }
    return SLAMHIP_OK;
  });
  // (the jobs-done word lies behind the LAST job's counters of the call: zero, as every word of the block between calls)
  if (!grc) grc = grow_blocks({st}, s->pose_cap, (size_t)(n * np), 1 << 14, [&](size_t cap) -> int {
    SLAMHIP_CHECK(s->d_scores.alloc(cap));
    SLAMHIP_CHECK(s->d_fp.alloc(cap));
    SLAMHIP_CHECK(s->d_pidx.alloc(cap));
    return SLAMHIP_OK;
  });
  if (!grc) grc = grow_blocks({st}, s->blk_cap, (size_t)(n * per_blk), 64, [&](size_t cap) -> int {
    SLAMHIP_CHECK(s->d_agg_s.alloc(cap));
    SLAMHIP_CHECK(s->d_agg_i.alloc(cap));
    return SLAMHIP_OK;
  });
  if (grc) return grc;
  // the views a lone sweep of each job would score through; one effective cell model and OIE for the launch
  int cell_model = -1, oie_eff = m->cfg.oie, max_n = 0;
  std::vector<double> inits(3 * (size_t)n);
  for (int c = 0; c < n; ++c) {
    BfJobView &v = s->h_jobs.get()[c];
    std::memset(&v, 0, sizeof(v));
    int model = 0, oie = 0;
    const int rc = score_map_view(ctx, jobs[c].map_id, &m->cfg, &v.map, &model, &oie);
    if (rc) return rc;
    if (c > 0 && (model != cell_model || oie != oie_eff)) return invalid_arg("the maps of one batch must share a cell model");
    cell_model = model;
    oie_eff = oie;
    v.scan = scan_view_of(blocks[c].d, blocks[c].stride, blocks[c].n, blocks[c].tot_w);
    max_n = std::max(max_n, blocks[c].n);
    for (int q = 0; q < 3; ++q) inits[3 * (size_t)c + q] = v.init[q] = jobs[c].init_pose[q];
    v.at = (long long)c * np;
    v.blk = (long long)c * per_blk;
  }
  (void)tie_check_default(m);
  const bool verify = m->tie_check == 1;
  // ---- validation lies behind: the streams latch, the jobs learn their bases
  const BfBatchPlan plan = m->bf_streams.plan(n, streams, inits.data(), nullptr);
  m->bf_streams.commit(plan);
  s->poses6.resize(6 * (size_t)n);
  for (int c = 0; c < n; ++c) {
    BfJobView &v = s->h_jobs.get()[c];
    for (int q = 0; q < 3; ++q) {
      v.base[q] = plan.base[3 * (size_t)c + q];
      s->poses6[6 * (size_t)c + q] = v.init[q];
      s->poses6[6 * (size_t)c + 3 + q] = v.base[q];
    }
  }
  s->n = np;
  const double t0 = MatchJob::now_us();
  SLAMHIP_CHECK(hipMemcpyAsync(s->d_jobs.get(), s->h_jobs.get(), sizeof(BfJobView) * (size_t)n, hipMemcpyHostToDevice, st));
  BfBatchArgs a;
  std::memset(&a, 0, sizeof(a));
  a.jobs = s->d_jobs.get();
  a.off = bf.d_off.get();
  a.nx = bf.nx;
  a.ny = bf.ny;
  a.nt = bf.nt;
  a.n = (int)np;
  a.n_jobs = n;
  a.oie = oie_eff;
  a.poses_per_block = 0;  // (launch_bf_batch: pick_poses_per_block(K n))
  a.verify = verify ? 1 : 0;
  a.scores = s->d_scores.get();
  a.fprints = s->d_fp.get();
  a.pidx = s->d_pidx.get();
  a.agg_s = s->d_agg_s.get();
  a.agg_i = s->d_agg_i.get();
  a.counters = s->d_counters.get();
  a.out = s->h_out.get();
  a.done = s->h_done.get();
  const unsigned seq = a.seq = next_epoch(s->seq);
  hipEvent_t e0 = nullptr, e1 = nullptr;
  {
    const int rc = profile_event_pair(ctx, &e0, &e1);
    if (rc) return rc;
  }
  if (e0) SLAMHIP_CHECK(hipEventRecord(e0, st));
  SLAMHIP_CHECK(launch_bf_batch(a, cell_model, max_n, st));
  if (e1) SLAMHIP_CHECK(hipEventRecord(e1, st));
  if (m->has_obs) {  // (the K x n scores in one copy)
    s->scores_host.resize((size_t)n * (size_t)np);
    SLAMHIP_CHECK(hipMemcpyAsync(s->scores_host.data(), s->d_scores.get(), sizeof(double) * (size_t)n * (size_t)np,
                                 hipMemcpyDeviceToHost, st));
  }
  volatile unsigned *done = s->h_done.get();
  unsigned long long spins = 0;
  while (*done != seq) {
    __builtin_ia32_pause();
    if ((++spins & 0xfffffull) == 0) {
      hipError_t qe = hipStreamQuery(st);
      if (qe != hipSuccess && qe != hipErrorNotReady) return hip_fail(qe, "batched brute-force sweeps");
    }
  }
  __atomic_thread_fence(__ATOMIC_ACQUIRE);
  if (m->has_obs) SLAMHIP_CHECK(hipStreamSynchronize(st));
  HcBatch *b = m->batch.get();
  long long units = 0;
  for (int c = 0; c < n; ++c) {
    const volatile BfHostOut *h = &s->h_out.get()[c];
    BatchJobResult &r = b->res[c];
    units += np * (long long)blocks[c].n;
    if (h->ambiguous) {  // nothing reported yet: the host-driven batches settle it, on the job's stream
      r.error = 4;
      r.on_chain = false;
      continue;
    }
    r.error = 0;
    r.on_chain = true;
    bf_pose_of_host(bf, &s->poses6[6 * (size_t)c], &s->poses6[6 * (size_t)c + 3], h->best_index, r.pose);
    r.prob = h->best_score;
    r.calls = r.evaluated = np;
    r.rescored = 0;
    r.steps = 1;
    ++m->bf_streams.s[(size_t)streams[c]].matches;
  }
  b->kernels = 3;  // score, scan, decide
  m->tail_calls = 0;
  m->t_stage_us = 0;
  m->t_score_us = MatchJob::now_us() - t0;
  if (ctx->profile) {
    ctx->prof_launches += 1;
    ctx->prof_units += units;
  }
  return SLAMHIP_OK;
}

// the enumerator stream of every job of a batch call (slamhip_matcher_set_bf_job_streams; none set: job j on stream
// j), checked before anything is staged, launched or latched
int bf_job_streams_of(const slamhip_matcher *m, int n_jobs, std::vector<int> *out) {
  if (const char *why = m->bf_streams.streams_of(n_jobs, out)) return invalid_arg(why);
  return SLAMHIP_OK;
}

// a batch call's fall-back: the lone path on the job's OWN stream -- its enumerator (and match count) in the matcher's
// place for the call.  A Monte-Carlo stream IS an enumerator object; a brute-force stream's is made for the call from
// the stream's record (its base, if latched) and the record follows what the call did to it.
struct JobStreamSwap {
  slamhip_matcher *m;
  int k;
  std::unique_ptr<slamhip::PoseEnumerator> own;  // (brute force: the matcher's own enumerator while the stream's is in)
  JobStreamSwap(slamhip_matcher *m_, int k_) : m(m_), k(k_) {
    if (k < 0) return;
    if (m->is_bf) {
      BfStream &rec = m->bf_streams.s[(size_t)k];
      auto pe = std::make_unique<BruteForcePoseEnumerator>(m->bf.r);
      if (rec.base_set) pe->latch_base(Pose{rec.base[0], rec.base[1], rec.base[2]});
      own = std::move(m->pe);
      m->pe = std::move(pe);
      std::swap(m->bf_matches, rec.matches);
    } else {
      swap_mc();
    }
  }
  ~JobStreamSwap() {
    if (k < 0) return;
    if (m->is_bf) {
      BfStream &rec = m->bf_streams.s[(size_t)k];
      const auto *pe = static_cast<const BruteForcePoseEnumerator *>(m->pe.get());
      rec.base_set = pe->base_set();
      if (rec.base_set) {
        rec.base[0] = pe->base().x;
        rec.base[1] = pe->base().y;
        rec.base[2] = pe->base().theta;
      }
      m->pe = std::move(own);
      std::swap(m->bf_matches, rec.matches);
    } else {
      swap_mc();
    }
  }
  void swap_mc() {
    std::swap(m->pe, m->mc_streams[k].pe);
    std::swap(m->mc_matches, m->mc_streams[k].matches);
  }
};

// A batch call's fall-backs work on the context's CURRENT scan: each selects, uploads or filters its job's scan into that
// place.  The keeper records the caller's own selection in front of the first of them (arm) and puts it back when the
// call ends, error returns included -- or, where that selection was the upload buffer and a fall-back has overwritten
// it, invalidates it, so that a later process_scan fails loudly instead of scoring another robot's scan.
struct ScanKeeper {
  slamhip_ctx *ctx;
  bool armed = false, saved_is_upload = false;
  bool upload_overwritten = false;  // set by the call: a fall-back's scan went through the context's upload buffer
  const double *saved_ptr = nullptr;
  size_t saved_stride = 0;
  int saved_n = 0;
  double saved_tot_w = 0;
  std::vector<double> saved_w, saved_f;
  explicit ScanKeeper(slamhip_ctx *ctx_) : ctx(ctx_) {}
  ScanKeeper(const ScanKeeper &) = delete;
  ScanKeeper &operator=(const ScanKeeper &) = delete;
  void arm() {
    if (armed) return;
    armed = true;
    saved_ptr = ctx->scan_ptr;
    saved_stride = ctx->scan_stride;
    saved_n = ctx->scan_n;
    saved_tot_w = ctx->scan_tot_w;
    // (asked now: a lone call may replace the upload buffer by a larger one)
    saved_is_upload = !saved_ptr || saved_ptr == ctx->d_scan.get();
    saved_w = ctx->h_weight;
    saved_f = ctx->h_factor;
  }
  ~ScanKeeper() {
    if (!armed) return;
    if (saved_is_upload && upload_overwritten) {
      ctx->scan_n = 0;  // (its contents are gone: "no scan uploaded" from here on)
    } else {
      ctx->scan_ptr = saved_ptr;
      ctx->scan_stride = saved_stride;
      ctx->scan_n = saved_n;
      ctx->scan_tot_w = saved_tot_w;
      ctx->h_weight.swap(saved_w);
      ctx->h_factor.swap(saved_f);
      ctx->h_scan_angle.clear();  // (a stored scan has its slot's, if any, as slamhip_scan_select leaves it)
      for (const slamhip_ctx::ScanSlot &sl : ctx->scan_slots)
        if (sl.d.get() == saved_ptr) ctx->h_scan_angle = sl.angle;
      ctx->scan_angle_on_device = false;
    }
    ctx->scan_angle_lazy = false;
  }
};

// THE hand-over of both batch calls, behind their chains: results in job order, the observer's events, the totals.
//   live_of(c)   job c's place among the chains' jobs (its slice of their trace); negative: its scan kept nothing -- no
//                launch, no observer call, its engine not advanced: 0 / 0 for every candidate, the lone call's answer
//   lone(j, keep, delta, prob, &kept)   the lone call for a job the chains did not take or did not settle (a
//                configuration they do not cover, a trace longer than a chain's slice), run on the job's engine stream
//                and under the keeper; kept: the points of its scan
// sid: the jobs' engine streams (empty: the matcher's own enumerator).  kept_n (optional): the points each job kept.
template <class Job, class LiveOf, class Lone>
int batch_hand_over(slamhip_matcher *m, int n_jobs, const Job *jobs, const std::vector<int> &sid, LiveOf &&live_of,
                    double *out_deltas, double *out_probs, int *kept_n, Lone &&lone) {
  constexpr bool kRaw = std::is_same<Job, slamhip_raw_match_job>::value;  // (its jobs' blocks are on record: raw.blocks)
  HcBatch *b = m->batch.get();
  const HcTraceEntry *chain_trace = b->h_trace.get();
  size_t chain_trace_per = (size_t)b->trace_per;
  if (!sid.empty() && m->mc_batch) {
    chain_trace = reinterpret_cast<const HcTraceEntry *>(m->mc_batch->h_trace.get());
    chain_trace_per = m->mc_batch->trace_per;
  }
  ScanKeeper keep(m->ctx);
  long long calls = 0, evaluated = 0, steps = 0, rescored = 0;
  for (int c = 0; c < n_jobs; ++c) {
    BatchJobResult &r = b->res[c];
    const Job &j = jobs[c];
    double *dl = out_deltas + 3 * c;
    const int live = live_of(c);
    int kept = 0;
    if (r.on_chain) {
      if constexpr (kRaw) kept = b->raw.blocks[c].n;
      for (int q = 0; q < 3; ++q) dl[q] = r.pose[q] - j.init_pose[q];
      out_probs[c] = r.prob;
      if (m->has_obs) {
        if (m->is_bf) {  // (a sweep has no trace: its events from its slice of the call's score array)
          const BfBatch *s = m->bf_batch.get();
          bf_replay_scores(m->obs, m->bf, &s->poses6[6 * (size_t)live], &s->poses6[6 * (size_t)live + 3],
                           s->scores_host.data() + (size_t)live * (size_t)s->n, s->n);
        } else {
          replay_trace(m->obs, chain_trace + (size_t)live * chain_trace_per, r.calls);
        }
        if (m->obs.on_matching_end) m->obs.on_matching_end(m->obs.user, dl, r.prob);
      }
    } else {
      const bool bf_unsettled = m->is_bf && r.error == 4;  // (the shared sweeps met a comparison they cannot settle)
      r = BatchJobResult{};
      if (live < 0) {
        dl[0] = dl[1] = dl[2] = 0.0;
        out_probs[c] = std::numeric_limits<double>::quiet_NaN();
      } else {
        keep.arm();
        int rc;
        {
          JobStreamSwap own(m, sid.empty() ? -1 : sid[c]);  // (the job's engine / enumerator for the call)
          m->bf.skip_device = bf_unsettled;
          rc = lone(j, keep, dl, &out_probs[c], &kept);
          m->bf.skip_device = false;
        }
        if (rc) return rc;
        if constexpr (kRaw) b->raw.blocks[c] = RawDeviceStage::Block{nullptr, 0, kept, true};
        if (kept > 0) {
          r.calls = m->job.scorer_calls;
          r.evaluated = m->job.poses_evaluated;
          r.steps = (int)m->job.launches;
          r.rescored = m->chain_rescored;
        }
      }
      for (int q = 0; q < 3; ++q) r.pose[q] = j.init_pose[q] + dl[q];
      r.prob = out_probs[c];
    }
    if (kept_n) kept_n[c] = kept;
    calls += r.calls;
    evaluated += r.evaluated;
    steps = std::max<long long>(steps, r.steps);
    rescored += r.rescored;
  }
  m->job.scorer_calls = calls;
  m->job.poses_evaluated = evaluated;
  m->job.launches = steps;
  m->chain_launched = b->kernels;
  m->chain_rescored = rescored;
  return SLAMHIP_OK;
}

// ---- the multi-resolution matcher ------------------------------------------------------------------
// BruteForceMultiResolutionScanMatcher::process_scan: the engine's loop on the host, its scores from the pyramid -- the
// root layer in one slamhip_pyramid_score_matches launch, everything below it in expand launches (m3rsm.hip), one per
// super-step.  on_matching_end is the one event the reference's matcher emits.
// what a launch writes back per candidate (score, level) and per slot (rectangle, score, level)
constexpr long long kScoreBack = sizeof(double) + sizeof(int), kSlotBack = 5 * sizeof(double) + sizeof(int);

int m3rsm_process_scan(slamhip_matcher *m, int map_id, const double init_pose[3], double out_delta[3], double *out_prob) {
  if (m->m3->rot_slots)
    return invalid_arg("rotation slots are set (slamhip_matcher_set_m3rsm_rotation_slots): the scan comes from a request's slots, "
                       "slamhip_matcher_m3rsm_match_many / _match_each");
  slamhip_matcher::M3rsm &s = *m->m3;
  slamhip_ctx *ctx = m->ctx;
  // (found before anything is launched or counted: the raw provider's bounds need the scan's angles)
  if (m->cfg.pose_trig == SLAMHIP_POSE_TRIG_RAW_EXACT && ctx->scan_n > 0 && !scan_angles_known(ctx)) {
    set_error("SLAMHIP_POSE_TRIG_RAW_EXACT needs the angles of the current scan's points: slamhip_scan_set_angles (or "
              "slamhip_scan_filter_upload) after the scan upload");
    return SLAMHIP_ERR_STATE;
  }
  m->job.scorer_calls = m->job.poses_evaluated = m->job.launches = 0;
  s.trace.clear();
  s.res = m3rsm::Result{};
  s.copied_back = 0;
  if (std::find(ctx->pyramids.begin(), ctx->pyramids.end(), (void *)s.pyr) == ctx->pyramids.end())
    return invalid_arg("the matcher's pyramid has been destroyed");
  int rc = pyr_check_fresh(s.pyr);
  if (rc) return rc;
  if (map_id != s.pyr->fine_id) return invalid_arg("map_id must be the pyramid's fine map");
  for (int k = 0; k < 3; ++k)
    if (!std::isfinite(init_pose[k])) return invalid_arg("the initial pose is not finite");
  rc = scan_assemble_now(ctx);  // (a raw scan whose block is still to be assembled)
  if (rc) return rc;
  const double t0 = MatchJob::now_us();
  const m3rsm::ScoreFn roots = [&](int n, const double *rot, const double *rect, double *score, int *level) {
    s.copied_back += kScoreBack * n;
    return slamhip_pyramid_score_matches(ctx, s.pyr, &m->cfg, init_pose, n, rot, rect, score, level);
  };
  const m3rsm::ExpandFn expand = [&](int n, const double *rot, const double *rect, int depth, double *slot_rect,
                                     double *slot_score, int *slot_level) {
    s.copied_back += kSlotBack * n * m3rsm::slots_of(depth);
    return slamhip_pyramid_expand_matches(ctx, s.pyr, &m->cfg, init_pose, n, rot, rect, s.cfg.translation_step, depth,
                                          slot_rect, slot_score, slot_level);
  };
  // without the expand kernel (slamhip_matcher_set_m3rsm_speculation(m, 0, 0)): the popped match alone, its children
  // split on the host and bounded by one slamhip_pyramid_score_matches launch -- a round trip per pop
  const m3rsm::ExpandFn per_pop = [&](int n, const double *rot, const double *rect, int, double *slot_rect, double *slot_score,
                                      int *slot_level) {
    const m3rsm::Rect parent{rect[0], rect[1], rect[2], rect[3]};
    m3rsm::Rect kids[m3rsm::kMaxChildren] = {};
    const int nk = n == 1 ? m3rsm::children(parent, s.cfg.translation_step, kids) : 0;
    double k_rot[m3rsm::kMaxChildren], k_rect[4 * m3rsm::kMaxChildren];
    for (int c = 0; c < m3rsm::kMaxChildren; ++c) {
      k_rot[c] = rot[0];
      const m3rsm::Rect &r = kids[c < nk ? c : 0];
      const double nan = std::numeric_limits<double>::quiet_NaN();
      const double v[4] = {c < nk ? r.bot : nan, c < nk ? r.top : nan, c < nk ? r.left : nan, c < nk ? r.right : nan};
      for (int q = 0; q < 4; ++q) k_rect[4 * c + q] = slot_rect[4 * c + q] = v[q];
      slot_score[c] = nan;
      slot_level[c] = -1;
    }
    s.copied_back += kScoreBack * nk;
    return nk ? slamhip_pyramid_score_matches(ctx, s.pyr, &m->cfg, init_pose, nk, k_rot, k_rect, slot_score, slot_level) : 0;
  };
  m3rsm::Config run_cfg = s.cfg;
  if (s.per_pop) run_cfg.width = run_cfg.depth = 1;
  const int erc = m3rsm::run(run_cfg, roots, s.per_pop ? per_pop : expand, &s.res, &s.trace);
  m->t_stage_us = 0;
  m->t_score_us = MatchJob::now_us() - t0;
  m->job.scorer_calls = s.res.scorer_calls;
  m->job.poses_evaluated = s.res.scored;
  m->job.launches = s.res.launches;
  switch (erc) {
    case m3rsm::kOk: break;
    case m3rsm::kErrCallback: return s.res.callback_rc;
    case m3rsm::kErrSuperSteps:
      set_error("the multi-resolution match reached its bound on super-steps");
      return SLAMHIP_ERR_UNSUPPORTED;
    case m3rsm::kErrNoMatch:  // (no candidate left: nothing is accepted, as for a scan with no point)
      out_delta[0] = out_delta[1] = out_delta[2] = 0.0;
      *out_prob = std::numeric_limits<double>::quiet_NaN();
      return SLAMHIP_OK;
    default:
      set_error("internal: the multi-resolution engine failed (an expand launch did not deliver a child)");
      return SLAMHIP_ERR_STATE;
  }
  for (int k = 0; k < 3; ++k) out_delta[k] = s.res.delta[k];
  *out_prob = s.res.prob;
  if (m->has_obs && m->obs.on_matching_end) m->obs.on_matching_end(m->obs.user, out_delta, s.res.prob);
  return SLAMHIP_OK;
}

// slamhip_matcher_set_m3rsm_rotation_slots: scan point weights that depend on the candidate's ROTATION (the reference's
// matcher hands its estimator prerotated scans, and VinySlamSPW weighs a point by its direction in the world).  The
// engine keeps its requests; at the launch boundary candidate (request k, rotation j-th of the root layer) reads entry
// k * n_rot + j of an expanded table, whose scan slot is req[k].scan_slot + j -- the same points, that rotation's weights.
// The kernels see one more request per rotation and nothing else.
struct RotationSlots {
  bool on = false;
  int n_rot = 1;
  std::vector<double> rots;  // the root layer's distinct rotations, in its order
  std::vector<slamhip_m3rsm_request> table;
  std::vector<int> mapped;
  void init(bool enabled, const m3rsm::Config &cfg, int n_requests, const slamhip_m3rsm_request *req) {
    on = enabled;
    if (!on) return;
    std::vector<double> rot;
    std::vector<m3rsm::Rect> rect;
    m3rsm::root_candidates(cfg, &rot, &rect);
    rots.clear();
    for (double r : rot)
      if (index_of(r) < 0) rots.push_back(r);
    n_rot = (int)rots.size();
    table.clear();
    for (int k = 0; k < n_requests; ++k)
      for (int j = 0; j < n_rot; ++j) {
        slamhip_m3rsm_request q = req[k];
        q.scan_slot = req[k].scan_slot + j;
        table.push_back(q);
      }
  }
  int index_of(double r) const {
    for (size_t j = 0; j < rots.size(); ++j)
      if (std::memcmp(&rots[j], &r, sizeof(double)) == 0) return (int)j;
    return -1;
  }
  int n_table(int n_requests) const { return on ? (int)table.size() : n_requests; }
  const slamhip_m3rsm_request *tab(const slamhip_m3rsm_request *req) const { return on ? table.data() : req; }
  // (children carry their parent's rotation bit for bit: every rotation of a launch is one of the root layer's)
  const int *map(int n, const int *rq, const double *rot) {
    if (!on) return rq;
    mapped.resize(n);
    for (int i = 0; i < n; ++i) mapped[i] = rq[i] * n_rot + std::max(0, index_of(rot[i]));
    return mapped.data();
  }
};

// Several requests in one search (m3rsm::run_many): the root layers of all requests in one
// slamhip_pyramid_score_requests launch, every super-step one slamhip_pyramid_expand_requests launch over parents of
// whichever requests the shared queue holds on top.
int m3rsm_match_many(slamhip_matcher *m, int n_requests, const slamhip_m3rsm_request *req, int *out_request, double out_delta[3],
                     double *out_prob) {
  slamhip_matcher::M3rsm &s = *m->m3;
  slamhip_ctx *ctx = m->ctx;
  m->job.scorer_calls = m->job.poses_evaluated = m->job.launches = 0;
  s.trace.clear();
  s.res = m3rsm::Result{};
  s.copied_back = 0;
  RotationSlots rs;
  rs.init(s.rot_slots, s.cfg, n_requests, req);
  const int n_tab = rs.n_table(n_requests);
  const slamhip_m3rsm_request *tab = rs.tab(req);
  {
    std::vector<PyrSource> src;  // (checked before anything runs: the launches check again, they are entry points too)
    const int rc = pyr_many_sources(ctx, &m->cfg, n_tab, tab, &src);
    if (rc) return rc;
  }
  const double t0 = MatchJob::now_us();
  const m3rsm::ScoreManyFn roots = [&](int n, const int *rq, const double *rot, const double *rect, double *score, int *level) {
    s.copied_back += kScoreBack * n;
    return slamhip_pyramid_score_requests(ctx, &m->cfg, n_tab, tab, n, rs.map(n, rq, rot), rot, rect, score, level);
  };
  const m3rsm::ExpandManyFn expand = [&](int n, const int *rq, const double *rot, const double *rect, int depth,
                                         double *slot_rect, double *slot_score, int *slot_level) {
    s.copied_back += kSlotBack * n * m3rsm::slots_of(depth);
    return slamhip_pyramid_expand_requests(ctx, &m->cfg, n_tab, tab, n, rs.map(n, rq, rot), rot, rect, s.cfg.translation_step,
                                           depth, slot_rect, slot_score, slot_level);
  };
  // without the expand kernel (speculation 0, 0): as for the lone match, a bounds launch per popped match
  const m3rsm::ExpandManyFn per_pop = [&](int n, const int *rq, const double *rot, const double *rect, int, double *slot_rect,
                                          double *slot_score, int *slot_level) {
    const m3rsm::Rect parent{rect[0], rect[1], rect[2], rect[3]};
    m3rsm::Rect kids[m3rsm::kMaxChildren] = {};
    const int nk = n == 1 ? m3rsm::children(parent, s.cfg.translation_step, kids) : 0;
    int k_req[m3rsm::kMaxChildren];
    double k_rot[m3rsm::kMaxChildren], k_rect[4 * m3rsm::kMaxChildren];
    for (int c = 0; c < m3rsm::kMaxChildren; ++c) {
      k_req[c] = rq[0];
      k_rot[c] = rot[0];
      const m3rsm::Rect &r = kids[c < nk ? c : 0];
      const double nan = std::numeric_limits<double>::quiet_NaN();
      const double v[4] = {c < nk ? r.bot : nan, c < nk ? r.top : nan, c < nk ? r.left : nan, c < nk ? r.right : nan};
      for (int q = 0; q < 4; ++q) k_rect[4 * c + q] = slot_rect[4 * c + q] = v[q];
      slot_score[c] = nan;
      slot_level[c] = -1;
    }
    s.copied_back += kScoreBack * nk;
    return nk ? slamhip_pyramid_score_requests(ctx, &m->cfg, n_tab, tab, nk, rs.map(nk, k_req, k_rot), k_rot, k_rect, slot_score,
                                               slot_level)
              : 0;
  };
  m3rsm::Config run_cfg = s.cfg;
  if (s.per_pop) run_cfg.width = run_cfg.depth = 1;
  const int erc = m3rsm::run_many(run_cfg, n_requests, roots, s.per_pop ? per_pop : expand, &s.res, &s.trace);
  m->t_stage_us = 0;
  m->t_score_us = MatchJob::now_us() - t0;
  m->job.scorer_calls = s.res.scorer_calls;
  m->job.poses_evaluated = s.res.scored;
  m->job.launches = s.res.launches;
  switch (erc) {
    case m3rsm::kOk: break;
    case m3rsm::kErrCallback: return s.res.callback_rc;
    case m3rsm::kErrSuperSteps:
      set_error("the multi-resolution match reached its bound on super-steps");
      return SLAMHIP_ERR_UNSUPPORTED;
    case m3rsm::kErrNoMatch:
      *out_request = -1;
      out_delta[0] = out_delta[1] = out_delta[2] = 0.0;
      *out_prob = std::numeric_limits<double>::quiet_NaN();
      return SLAMHIP_OK;
    default:
      set_error("internal: the multi-resolution engine failed (an expand launch did not deliver a child)");
      return SLAMHIP_ERR_STATE;
  }
  *out_request = s.res.request;
  for (int k = 0; k < 3; ++k) out_delta[k] = s.res.delta[k];
  *out_prob = s.res.prob;
  if (m->has_obs && m->obs.on_matching_end) m->obs.on_matching_end(m->obs.user, out_delta, s.res.prob);
  return SLAMHIP_OK;
}

// K INDEPENDENT matches advancing in lock-step (m3rsm::run_each): all root layers in one slamhip_pyramid_score_requests
// launch, then per round one slamhip_pyramid_expand_requests launch over the parents of every search that waits for
// one, request = job.  Each search is the lone match's, so request k gets what m3rsm_process_scan gives on its inputs.
constexpr size_t kEachStageLimit = (size_t)256 << 20;  // a launch's strict-mode terms beyond this: consecutive launches

int m3rsm_each_run(slamhip_matcher *m, int n_requests, const std::vector<PyrSource> &src, RotationSlots &rs, int cell_model,
                   double *out_deltas, double *out_probs);

int m3rsm_match_each(slamhip_matcher *m, int n_requests, const slamhip_m3rsm_request *req, double *out_deltas, double *out_probs) {
  slamhip_matcher::M3rsm &s = *m->m3;
  slamhip_ctx *ctx = m->ctx;
  m->job.scorer_calls = m->job.poses_evaluated = m->job.launches = 0;
  s.trace.clear();
  s.res = m3rsm::Result{};
  s.copied_back = 0;
  s.each_res.clear();
  s.each_code.clear();
  s.each_trace.clear();
  if (s.per_pop) return invalid_arg("speculation (0, 0), the per-pop measuring route, has no batched form");
  RotationSlots rs;
  rs.init(s.rot_slots, s.cfg, n_requests, req);
  const int n_tab = rs.n_table(n_requests);
  const slamhip_m3rsm_request *tab = rs.tab(req);
  std::vector<PyrSource> src;  // (checked before anything runs)
  {
    const int rc = pyr_many_sources(ctx, &m->cfg, n_tab, tab, &src);
    if (rc) return rc;
  }
  return m3rsm_each_run(m, n_requests, src, rs, tab[0].pyramid->cell_model, out_deltas, out_probs);
}

// ... below the sources: request k's scan, levels and base pose are src[k * rs.n_rot + rotation slot], wherever the scan
// lies (a stored slot, or a block slamhip_matcher_m3rsm_match_each_raw has assembled).  Resets the last call's state.
int m3rsm_each_run(slamhip_matcher *m, int n_requests, const std::vector<PyrSource> &src, RotationSlots &rs, int cell_model,
                   double *out_deltas, double *out_probs) {
  slamhip_matcher::M3rsm &s = *m->m3;
  slamhip_ctx *ctx = m->ctx;
  m->job.scorer_calls = m->job.poses_evaluated = m->job.launches = 0;
  s.trace.clear();
  s.res = m3rsm::Result{};
  s.copied_back = 0;
  s.each_res.clear();
  s.each_code.clear();
  s.each_trace.clear();
  const double t0 = MatchJob::now_us();
  const bool strict = m->cfg.sum_order == SLAMHIP_SUM_SEQUENTIAL;
  long long launches = 0;
  std::vector<size_t> bytes;
  std::vector<int> first;
  // entries [first[c], first[c + 1]) per launch: one launch, unless strict mode's terms (slots x beams doubles per
  // entry) would outgrow the limit
  const auto cut = [&](int n, const int *rq, size_t slots) {
    if (!strict) {
      first.assign({0, n});
      return;
    }
    bytes.resize(n);
    for (int i = 0; i < n; ++i) bytes[i] = sizeof(double) * slots * (size_t)src[(size_t)rq[i] * rs.n_rot].scan.n;
    m3rsm::split_by_bytes(bytes.data(), n, kEachStageLimit, &first);
  };
  const m3rsm::ScoreManyFn roots = [&](int n, const int *rq, const double *rot, const double *rect, double *score, int *level) {
    cut(n, rq, 1);
    s.copied_back += kScoreBack * n;
    const int *mq = rs.map(n, rq, rot);
    for (size_t c = 0; c + 1 < first.size(); ++c) {
      const int at = first[c];
      const int rc = pyr_score_sources(ctx, &m->cfg, src, cell_model, first[c + 1] - at, mq + at, rot + at,
                                       rect + 4 * (size_t)at, score + at, level + at);
      ++launches;
      if (rc) return rc;
    }
    return 0;
  };
  const m3rsm::ExpandManyFn expand = [&](int n, const int *rq, const double *rot, const double *rect, int depth,
                                         double *slot_rect, double *slot_score, int *slot_level) {
    const size_t slots = (size_t)m3rsm::slots_of(depth);
    cut(n, rq, slots);
    s.copied_back += kSlotBack * n * (long long)slots;
    const int *mq = rs.map(n, rq, rot);
    for (size_t c = 0; c + 1 < first.size(); ++c) {
      const size_t at = (size_t)first[c];
      const int rc = pyr_expand_sources(ctx, &m->cfg, src, cell_model, first[c + 1] - first[c], mq + at, rot + at,
                                        rect + 4 * at, s.cfg.translation_step, depth, slot_rect + 4 * at * slots,
                                        slot_score + at * slots, slot_level + at * slots);
      ++launches;
      if (rc) return rc;
    }
    return 0;
  };
  const std::vector<m3rsm::Config> cfgs((size_t)n_requests, s.cfg);
  s.each_res.resize(n_requests);
  s.each_code.assign(n_requests, m3rsm::kPending);
  s.each_trace.resize(n_requests);
  const int threads = std::min(s.each_threads ? s.each_threads : m3rsm::each_default_threads(n_requests), n_requests);
  if (!s.each_pool || s.each_pool->threads() != threads) s.each_pool = std::make_unique<m3rsm::Pool>(threads);
  const int erc = m3rsm::run_each(cfgs.data(), n_requests, roots, expand, s.each_res.data(), s.each_code.data(),
                                  s.each_trace.data(), s.each_pool.get());
  m->t_stage_us = 0;
  m->t_score_us = MatchJob::now_us() - t0;
  for (const m3rsm::Result &r : s.each_res) {
    m->job.scorer_calls += r.scorer_calls;
    m->job.poses_evaluated += r.scored;
  }
  m->job.launches = launches;
  switch (erc) {
    case m3rsm::kOk: break;
    case m3rsm::kErrCallback:
      for (const m3rsm::Result &r : s.each_res)
        if (r.callback_rc) return r.callback_rc;
      set_error("internal: the multi-resolution engine lost a launch's error");
      return SLAMHIP_ERR_STATE;
    case m3rsm::kErrSuperSteps:
      set_error("a multi-resolution match reached its bound on super-steps");
      return SLAMHIP_ERR_UNSUPPORTED;
    case m3rsm::kErrInvalid: return invalid_arg("more candidates than one launch takes");
    default:
      set_error("internal: the multi-resolution engine failed (an expand launch did not deliver a child)");
      return SLAMHIP_ERR_STATE;
  }
  for (int k = 0; k < n_requests; ++k) {
    double *d = out_deltas + 3 * (size_t)k;
    if (s.each_code[k] != m3rsm::kOk) {  // (no candidate left: nothing is accepted, as the lone match has it)
      d[0] = d[1] = d[2] = 0.0;
      out_probs[k] = std::numeric_limits<double>::quiet_NaN();
      continue;
    }
    for (int q = 0; q < 3; ++q) d[q] = s.each_res[k].delta[q];
    out_probs[k] = s.each_res[k].prob;
  }
  if (m->has_obs && m->obs.on_matching_end)
    for (int k = 0; k < n_requests; ++k)
      if (s.each_code[k] == m3rsm::kOk) m->obs.on_matching_end(m->obs.user, out_deltas + 3 * (size_t)k, s.each_res[k].prob);
  return SLAMHIP_OK;
}

// What the launches of a raw-scan call left per live place (plan[c].live) -> per job; `none` for a job that kept nothing.
template <class T>
void live_to_job(const std::vector<RawBatchPlan> &plan, std::vector<T> &v, const T &none) {
  std::vector<T> by_job(plan.size(), none);
  for (size_t c = 0; c < plan.size(); ++c) {
    const int l = plan[c].live;
    if (l >= 0 && l < (int)v.size()) by_job[c] = std::move(v[l]);
  }
  v = std::move(by_job);
}
// the texts of RawDeviceStage::check_scan's refusals, for a job of the chains' batch and for a fleet request
const char *const kBadRawJob[] = {nullptr, "bad scan in a raw match job", "unknown trig mode in a raw match job", "unknown weighting kind"};
const char *const kBadRawRequest[] = {nullptr, "bad scan in a raw request", "unknown trig mode in a raw request", "unknown weighting kind"};

}  // namespace

extern "C" {

int slamhip_matcher_m3rsm_match_each(slamhip_matcher *m, int n_requests, const slamhip_m3rsm_request *req, double *out_deltas,
                                     double *out_probs) {
  if (!m || !m->is_m3rsm) return invalid_arg("not a multi-resolution matcher");
  if (!out_deltas || !out_probs) return invalid_arg("null outputs");
  return m3rsm_match_each(m, n_requests, req, out_deltas, out_probs);
}

// K raw scans in, K multi-resolution matches.  The host half per request is the lone raw call's; RawDeviceStage (which
// slamhip_matcher_process_raw_scan_batch drives too; the window is the request's pyramid's fine map) writes every live
// request's block -- five rows and the kept angles -- into the matcher's arena in HBM with ONE launch; the lock-step
// searches of m3rsm_match_each run over sources that point at the blocks.  The pinned arena is refilled by the next
// call only: this one returns after the searches, launched on the same stream behind the assembly kernel, have
// delivered their last results.  Every refusal comes before the first launch and before the last call's state goes.
int slamhip_matcher_m3rsm_match_each_raw(slamhip_matcher *m, int n_requests, const slamhip_m3rsm_raw_request *req, double *out_deltas,
                                         double *out_probs, int *kept_n) {
  if (!m || !m->is_m3rsm) return invalid_arg("not a multi-resolution matcher");
  if (n_requests < 1 || !req || !out_deltas || !out_probs) return invalid_arg("at least one request, and room for the results");
  slamhip_matcher::M3rsm &s = *m->m3;
  slamhip_ctx *ctx = m->ctx;
  if (s.per_pop) return invalid_arg("speculation (0, 0), the per-pop measuring route, has no batched form");
  if (s.rot_slots)
    return invalid_arg("rotation slots are set (slamhip_matcher_set_m3rsm_rotation_slots): rotation-slot scans are not made "
                       "on the device, the scans come from a request's stored slots");
  if (n_requests > 65535) return invalid_arg("more requests than one assembly launch takes");
  std::vector<PyrSource> all(n_requests);
  std::vector<RawBatchJob> in(n_requests);
  const slamhip_pyramid *first = nullptr;
  for (int k = 0; k < n_requests; ++k) {
    if (const int bad = RawDeviceStage::check_scan(req[k].scan)) return invalid_arg(kBadRawRequest[bad]);
    int rc = pyr_source_begin(ctx, &m->cfg, req[k].pyramid, &first, &all[k]);
    if (rc) return rc;
    rc = pyr_source_pose(req[k].init_pose, &all[k]);
    if (rc) return rc;
    const DeviceMap &dm = ctx->maps[req[k].pyramid->fine_id];  // (bound and the pyramid's: pyr_source_begin has checked)
    in[k] = RawBatchStage::job_of(req[k].scan, req[k].init_pose, ScanWindow{dm.scale, dm.origin_x, dm.origin_y, dm.width, dm.height});
  }
  SLAMHIP_CHECK(hipSetDevice(ctx->device));
  if (!s.raw) s.raw = std::make_unique<RawDeviceStage>();
  RawDeviceStage &w = *s.raw;
  const RawBatchStage &raw = w.host;
  int rc = w.prepare(n_requests, in.data(), sizeof(ScanAssembleEachArgs), 6);
  if (rc) return invalid_arg(scan_error_text(rc));
  if (raw.n_live > 0) {
    rc = w.assemble<ScanAssembleEachArgs>(ctx, in.data());
    if (rc) return rc;
  } else {  // every filter kept nothing: no launch at all
    w.blocks.assign(n_requests, RawDeviceStage::Block{});
  }
  // ---- the last check lies behind: from here on the last call's state goes
  if (kept_n)
    for (int k = 0; k < n_requests; ++k) kept_n[k] = raw.plan[k].k;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  for (int k = 0; k < n_requests; ++k) {
    out_deltas[3 * (size_t)k] = out_deltas[3 * (size_t)k + 1] = out_deltas[3 * (size_t)k + 2] = 0.0;
    out_probs[k] = nan;
  }
  const auto spread = [&] {  // the searches' results by live place -> by request; an empty request: nothing ran
    live_to_job(raw.plan, s.each_res, m3rsm::Result{});
    live_to_job(raw.plan, s.each_code, (int)m3rsm::kErrNoMatch);
    live_to_job(raw.plan, s.each_trace, std::vector<m3rsm::Call>{});
  };
  if (raw.n_live == 0) {
    m->job.scorer_calls = m->job.poses_evaluated = m->job.launches = 0;
    s.trace.clear();
    s.res = m3rsm::Result{};
    s.copied_back = 0;
    s.each_res.clear();
    s.each_code.clear();
    s.each_trace.clear();
    spread();
    return SLAMHIP_OK;
  }
  // ---- the sources: a live request's scan is its block
  std::vector<PyrSource> src(raw.n_live);
  const bool exact = m->cfg.pose_trig == SLAMHIP_POSE_TRIG_RAW_EXACT;
  for (int k = 0; k < n_requests; ++k) {
    const RawBatchPlan &p = raw.plan[k];
    if (p.live < 0) continue;
    const double *d = w.blocks[k].d;
    src[p.live] = all[k];
    pyr_source_block(d, p.stride, p.k, p.tot_w, exact ? d + 5 * p.stride : nullptr, &src[p.live]);
  }
  RotationSlots rs;  // (off)
  std::vector<double> deltas(3 * (size_t)raw.n_live), probs(raw.n_live);
  rc = m3rsm_each_run(m, raw.n_live, src, rs, first->cell_model, deltas.data(), probs.data());
  m->job.launches += 1;  // (k_scan_assemble_table in front of the searches' launches)
  spread();
  if (rc) return rc;
  for (int k = 0; k < n_requests; ++k) {
    const int l = raw.plan[k].live;
    if (l < 0) continue;
    for (int q = 0; q < 3; ++q) out_deltas[3 * (size_t)k + q] = deltas[3 * (size_t)l + q];
    out_probs[k] = probs[l];
  }
  return SLAMHIP_OK;
}

int slamhip_matcher_m3rsm_each_scan_download(slamhip_matcher *m, int request, int cap, double *out5, double *angle_out, int *n) {
  if (!m || !m->is_m3rsm) return invalid_arg("not a multi-resolution matcher");
  if (!n || cap < 0 || (cap > 0 && !out5)) return invalid_arg("bad arguments");
  const RawDeviceStage *w = m->m3->raw.get();
  if (!w || request < 0 || request >= (int)w->blocks.size()) return invalid_arg("no such request in the last match_each_raw");
  return w->download(m->ctx, request, cap, out5, angle_out, n,
                     "slamhip_matcher_m3rsm_each_scan_download: room for fewer points than the request's scan has");
}

int slamhip_matcher_m3rsm_trace_each(slamhip_matcher *m, int request, int cap, double *rows, int *n) {
  if (!m || !m->is_m3rsm) return invalid_arg("not a multi-resolution matcher");
  if (request < 0 || request >= (int)m->m3->each_trace.size()) return invalid_arg("no such request in the last match_each");
  if (cap < 0 || (cap > 0 && !rows)) return invalid_arg("bad trace buffer");
  const std::vector<m3rsm::Call> &t = m->m3->each_trace[request];
  if (n) *n = (int)t.size();
  for (size_t i = 0; i < std::min((size_t)cap, t.size()); ++i) {
    double *r = rows + 7 * i;
    r[0] = t[i].rotation;
    r[1] = t[i].rect.bot;
    r[2] = t[i].rect.top;
    r[3] = t[i].rect.left;
    r[4] = t[i].rect.right;
    r[5] = t[i].score;
    r[6] = (double)t[i].level;
  }
  return SLAMHIP_OK;
}

int slamhip_matcher_m3rsm_each_stats(slamhip_matcher *m, int request, long long *scorer_calls, long long *poses_evaluated,
                                     long long *super_steps, long long *branching_pops) {
  if (!m || !m->is_m3rsm) return invalid_arg("not a multi-resolution matcher");
  if (request < 0 || request >= (int)m->m3->each_res.size()) return invalid_arg("no such request in the last match_each");
  const m3rsm::Result &r = m->m3->each_res[request];
  if (scorer_calls) *scorer_calls = r.scorer_calls;
  if (poses_evaluated) *poses_evaluated = r.scored;
  if (super_steps) *super_steps = r.super_steps;
  if (branching_pops) *branching_pops = r.branching_pops;
  return SLAMHIP_OK;
}

int slamhip_matcher_m3rsm_copied_back(slamhip_matcher *m, long long *bytes) {
  if (!m || !m->is_m3rsm || !bytes) return invalid_arg("not a multi-resolution matcher");
  *bytes = m->m3->copied_back;
  return SLAMHIP_OK;
}

int slamhip_matcher_set_m3rsm_rotation_slots(slamhip_matcher *m, int on) {
  if (!m || !m->is_m3rsm) return invalid_arg("not a multi-resolution matcher");
  m->m3->rot_slots = on != 0;
  return SLAMHIP_OK;
}

int slamhip_matcher_m3rsm_rotations(slamhip_matcher *m, int cap, double *rotation, int *n) {
  if (!m || !m->is_m3rsm) return invalid_arg("not a multi-resolution matcher");
  if (cap < 0 || !n || (cap > 0 && !rotation)) return invalid_arg("null outputs");
  RotationSlots rs;
  rs.init(true, m->m3->cfg, 0, nullptr);
  *n = rs.n_rot;
  for (int j = 0; j < std::min(cap, rs.n_rot); ++j) rotation[j] = rs.rots[j];
  return SLAMHIP_OK;
}

int slamhip_matcher_set_m3rsm_threads(slamhip_matcher *m, int threads) {
  if (!m || !m->is_m3rsm) return invalid_arg("not a multi-resolution matcher");
  if (threads < 0 || threads > m3rsm::kEachMaxThreads) return invalid_arg("threads: 1 .. 16, or 0 for the default");
  m->m3->each_threads = threads;
  return SLAMHIP_OK;
}

int slamhip_matcher_m3rsm_match_many(slamhip_matcher *m, int n_requests, const slamhip_m3rsm_request *req, int *out_request,
                                     double out_delta[3], double *out_prob) {
  if (!m || !m->is_m3rsm) return invalid_arg("not a multi-resolution matcher");
  if (!out_request || !out_delta || !out_prob) return invalid_arg("null outputs");
  return m3rsm_match_many(m, n_requests, req, out_request, out_delta, out_prob);
}

int slamhip_matcher_m3rsm_trace_many(slamhip_matcher *m, int cap, double *rows, int *n) {
  if (!m || !m->is_m3rsm) return invalid_arg("not a multi-resolution matcher");
  if (cap < 0 || (cap > 0 && !rows)) return invalid_arg("bad trace buffer");
  const std::vector<m3rsm::Call> &t = m->m3->trace;
  if (n) *n = (int)t.size();
  for (size_t i = 0; i < std::min((size_t)cap, t.size()); ++i) {
    double *r = rows + 8 * i;
    r[0] = (double)t[i].request;
    r[1] = t[i].rotation;
    r[2] = t[i].rect.bot;
    r[3] = t[i].rect.top;
    r[4] = t[i].rect.left;
    r[5] = t[i].rect.right;
    r[6] = t[i].score;
    r[7] = (double)t[i].level;
  }
  return SLAMHIP_OK;
}

int slamhip_matcher_create_m3rsm(slamhip_ctx *ctx, const slamhip_spe_cfg *cfg, slamhip_pyramid *pyramid, double max_x_error,
                                 double max_y_error, double max_th_error, double angle_step, double translation_step,
                                 slamhip_matcher **out) {
  if (!ctx || !cfg || !pyramid || !out) return invalid_arg("null argument");
  *out = nullptr;
  if (pyramid->ctx != ctx) return invalid_arg("the pyramid belongs to another context");
  // (a window OOPE -- not the 1-cell or the GMapping one --, the pyramid's OIE, a known sum order)
  int rc = pyr_check_score_cfg(pyramid, cfg);
  if (rc) return rc;
  if (cfg->pose_trig != SLAMHIP_POSE_TRIG_DEVICE && cfg->pose_trig != SLAMHIP_POSE_TRIG_HOST &&
      cfg->pose_trig != SLAMHIP_POSE_TRIG_RAW_EXACT)
    return invalid_arg("pose_trig: DEVICE, HOST or RAW_EXACT");
  if (!(angle_step > 0) || !(translation_step > 0) || !std::isfinite(angle_step) || !std::isfinite(translation_step))
    return invalid_arg("the rotation and translation steps must be positive and finite");
  if (!(max_x_error >= 0) || !(max_y_error >= 0) || !(max_th_error >= 0) || !std::isfinite(max_x_error) ||
      !std::isfinite(max_y_error) || !std::isfinite(max_th_error))
    return invalid_arg("the lookup limits must be finite and not negative");
  rc = make_matcher(ctx, cfg, nullptr, 0, out);
  if (rc) return rc;
  slamhip_matcher *m = *out;
  m->is_m3rsm = true;
  m->m3 = std::make_unique<slamhip_matcher::M3rsm>();
  m->m3->pyr = pyramid;
  m3rsm::Config &c = m->m3->cfg;
  c.max_x_error = max_x_error;
  c.max_y_error = max_y_error;
  c.max_th_error = max_th_error;
  c.angle_step = angle_step;
  c.translation_step = translation_step;
  return SLAMHIP_OK;
}

int slamhip_matcher_set_m3rsm_speculation(slamhip_matcher *m, int width, int depth) {
  if (!m || !m->is_m3rsm) return invalid_arg("not a multi-resolution matcher");
  if (width == 0 && depth == 0) {  // the route without the expand kernel: what the speculation is measured against
    m->m3->per_pop = true;
    return SLAMHIP_OK;
  }
  if (width < 1 || width > 65536 || depth < 1 || depth > m3rsm::kMaxDepth)
    return invalid_arg("speculation: width in [1, 65536], depth 1, 2 or 3 (or 0, 0)");
  m->m3->per_pop = false;
  m->m3->cfg.width = width;
  m->m3->cfg.depth = depth;
  return SLAMHIP_OK;
}

int slamhip_matcher_m3rsm_trace(slamhip_matcher *m, int cap, double *rows, int *n) {
  if (!m || !m->is_m3rsm) return invalid_arg("not a multi-resolution matcher");
  if (cap < 0 || (cap > 0 && !rows)) return invalid_arg("bad trace buffer");
  const std::vector<m3rsm::Call> &t = m->m3->trace;
  if (n) *n = (int)t.size();
  for (size_t i = 0; i < std::min((size_t)cap, t.size()); ++i) {
    double *r = rows + 7 * i;
    r[0] = t[i].rotation;
    r[1] = t[i].rect.bot;
    r[2] = t[i].rect.top;
    r[3] = t[i].rect.left;
    r[4] = t[i].rect.right;
    r[5] = t[i].score;
    r[6] = (double)t[i].level;
  }
  return SLAMHIP_OK;
}

int slamhip_matcher_create_mc(slamhip_ctx *ctx, const slamhip_spe_cfg *cfg, unsigned seed,
                              double td, double rd, unsigned failed_limit, unsigned attempts_limit,
                              slamhip_matcher **out) {
  int rc = make_matcher(ctx, cfg,
                        std::make_unique<GaussianPoseEnumerator>(seed, td, rd, failed_limit, attempts_limit),
                        1024, out);
  if (rc) return rc;
  (*out)->is_mc = true;
  (*out)->chain_nt = 512;
  (*out)->device = ctx->device;
  return SLAMHIP_OK;
}

int slamhip_matcher_create_hc(slamhip_ctx *ctx, const slamhip_spe_cfg *cfg, unsigned failed_rounds_limit,
                              double dt, double dr, slamhip_matcher **out) {
  int rc = make_matcher(ctx, cfg, std::make_unique<HillClimbingPoseEnumerator>(failed_rounds_limit, dt, dr),
                        1024, out);
  if (rc) return rc;
  (*out)->is_hc = true;
  (*out)->hc.max_failed = failed_rounds_limit;
  (*out)->hc.dt = dt;
  (*out)->hc.dr = dr;
  return SLAMHIP_OK;
}

int slamhip_matcher_create_bf(slamhip_ctx *ctx, const slamhip_spe_cfg *cfg, const double range9[9],
                              slamhip_matcher **out) {
  if (!range9) return invalid_arg("null range");
  if (!(range9[0] <= range9[1] && range9[3] <= range9[4] && range9[6] <= range9[7]) ||
      !(range9[2] > 0 && range9[5] > 0 && range9[8] > 0))
    return invalid_arg("brute-force ranges need from <= to and positive steps");
  const int rc = make_matcher(ctx, cfg, std::make_unique<BruteForcePoseEnumerator>(range9), 8192, out);
  if (rc) return rc;
  (*out)->is_bf = true;
  std::memcpy((*out)->bf.r, range9, sizeof((*out)->bf.r));
  return SLAMHIP_OK;
}

int slamhip_matcher_destroy(slamhip_matcher *m) {
  if (m) {
    if (m->hc.d_chain || m->batch || m->bf.d_poses || m->bf_batch || m->bf_peaks) {
      // run-ahead kernels of the last chain may still read the blocks; the context may already be gone
      // (destroying it synchronised its stream), so wait on the device, not on the context's stream
      hipSetDevice(m->device);
      hipDeviceSynchronize();
    }
  }
  delete m;  // (the blocks go with their owners)
  return SLAMHIP_OK;
}

int slamhip_matcher_reset_state(slamhip_matcher *m) {
  if (!m) return invalid_arg("null matcher");
  if (m->pe) m->pe->reset();  // (the multi-resolution matcher keeps no state between matches)
  for (slamhip_matcher::McStream &k : m->mc_streams) k.pe->reset();  // (the engines' positions stay)
  m->bf_streams.reset();  // (the latched bases stay, as the reference's reset() leaves them)
  return SLAMHIP_OK;
}

int slamhip_matcher_set_observer(slamhip_matcher *m, const slamhip_observer *obs) {
  if (!m) return invalid_arg("null matcher");
  m->has_obs = obs != nullptr;
  if (obs) m->obs = *obs;
  return SLAMHIP_OK;
}

int slamhip_matcher_set_batch(slamhip_matcher *m, int max_batch) {
  if (!m || max_batch < 0) return invalid_arg("bad batch");
  if (max_batch > 0) m->max_batch = max_batch;
  return SLAMHIP_OK;
}

int slamhip_matcher_set_device_chain(slamhip_matcher *m, int mode, int threads) {
  if (!m || mode < 0 || mode > 2 || (threads != 0 && threads != 256 && threads != 512 && threads != 1024))
    return invalid_arg("bad device-chain setting");
  (void)chain_eligible(m);  // defaults first, then the explicit setting
  m->chain_mode = mode;
  m->chain_mode_explicit = true;
  m->resident.reset();
  if (threads) m->chain_nt = threads;
  return SLAMHIP_OK;
}

int slamhip_matcher_set_tie_check(slamhip_matcher *m, int on) {
  if (!m || (on != 0 && on != 1)) return invalid_arg("bad tie-check setting");
  m->tie_check = on;
  return SLAMHIP_OK;
}

#ifdef SLAMHIP_TESTING
// debugging aid, not part of include/slamhip.h: wall-clock stamps (100 MHz) of workgroup 1 inside the
// first 64 super-steps of the following process_scan calls: kernel entry, staged, replayed, pose ready,
// terms ready, score stored, two spare (the co-resident 1-cell chain, spare stamp 6 of the super-steps from the fourth
// on: polls the stamped workgroup's sweep took | granules still missing behind its first poll << 32)
int slamhip_matcher_debug_stamps(slamhip_matcher *m, long long *out512) {
  if (!m) return invalid_arg("null matcher");
  if (!m->d_stamps) {
    SLAMHIP_CHECK(m->d_stamps.alloc(512));
    SLAMHIP_CHECK(hipMemset(m->d_stamps.get(), 0, sizeof(long long) * 512));
    SLAMHIP_CHECK(hipDeviceSynchronize());  // (hipMemset of device memory does not wait: the next match would race it)
    return SLAMHIP_OK;
  }
  SLAMHIP_CHECK(hipDeviceSynchronize());
  if (out512) SLAMHIP_CHECK(hipMemcpy(out512, m->d_stamps.get(), sizeof(long long) * 512, hipMemcpyDeviceToHost));
  return SLAMHIP_OK;
}
#endif  // SLAMHIP_TESTING

int slamhip_matcher_process_scan_batch(slamhip_matcher *m, int n_jobs, const slamhip_match_job *jobs,
                                       double *out_deltas, double *out_probs) {
  if (!m || n_jobs < 0 || (n_jobs > 0 && (!jobs || !out_deltas || !out_probs))) return invalid_arg("null argument");
  if (n_jobs == 0) return SLAMHIP_OK;
  if (m->is_m3rsm) return invalid_arg("multi-resolution matches are not batched");
  slamhip_ctx *ctx = m->ctx;
  for (int c = 0; c < n_jobs; ++c) {
    const slamhip_match_job &j = jobs[c];
    if (j.scan_slot >= 0) {
      if (j.scan_slot >= (int)ctx->scan_slots.size() || !ctx->scan_slots[j.scan_slot].d)
        return invalid_arg("a match job names a scan slot nothing is stored in");
    } else if (j.n <= 0 || !j.range || !j.cos_a || !j.sin_a || !j.weight) {
      return invalid_arg("bad scan in a match job");
    }
  }
  // a Monte-Carlo matcher with engine streams: job c runs on ITS stream, in the shared launches or through the lone
  // path.  Everything that can be refused is refused here, before a stream or the last-batch state is touched.
  // A brute-force matcher with enumerator streams (slamhip_matcher_set_bf_streams) likewise: job c enumerates around ITS
  // stream's base, in the shared sweeps or through the lone path; without streams its jobs run job after job through
  // the lone call on the matcher's own enumerator, as ever.
  const bool mc_streams = m->is_mc && !m->mc_streams.empty();
  const bool bf_streams = m->is_bf && m->bf_streams.any();
  std::vector<int> sid;
  bool chains = n_jobs > 1 && (mc_streams ? mc_batch_eligible(m) : (bf_streams ? bf_batch_eligible(m) : batch_chain_eligible(m)));
  if (m->is_bf && !bf_streams) chains = false;
  // the jobs the shared launches take.  The chains take all or none; of a brute-force batch a job above 4096 beams
  // leaves alone (dev_of[c] < 0: the lone call on its stream) and the others stay.
  std::vector<int> dev_of;
  int n_dev = n_jobs;
  if (chains && bf_streams) {
    dev_of.assign(n_jobs, -1);
    n_dev = 0;
    for (int c = 0; c < n_jobs; ++c)
      if ((jobs[c].scan_slot >= 0 ? ctx->scan_slots[jobs[c].scan_slot].n : jobs[c].n) <= kBfBatchMaxBeams) dev_of[c] = n_dev++;
    chains = n_dev > 1;
  }
  for (int c = 0; c < n_jobs && chains && !bf_streams; ++c)
    chains = (jobs[c].scan_slot >= 0 ? ctx->scan_slots[jobs[c].scan_slot].n : jobs[c].n) <= 4096;
  int cell_model = -1;
  if (mc_streams) {
    const int rc = mc_job_streams_of(m, n_jobs, &sid);
    if (rc) return rc;
  }
  if (bf_streams) {
    const int rc = bf_job_streams_of(m, n_jobs, &sid);
    if (rc) return rc;
  }
  if (chains || mc_streams || bf_streams) {  // (the lone route of a hill-climbing or brute-force job checks its map for itself)
    const int rc = batch_maps_check(ctx, n_jobs, jobs, chains ? &cell_model : nullptr);
    if (rc) return rc;
  }
  SLAMHIP_CHECK(hipSetDevice(ctx->device));
  if (chains && bf_streams) {  // (the offsets made, K x n within the scratch budget: else every job alone)
    const int rc = bf_batch_fits(m, n_dev, &chains);
    if (rc) return rc;
  }
  if (!m->batch) m->batch = std::make_unique<HcBatch>();
  HcBatch *b = m->batch.get();
  if (chains && bf_streams) {
    std::vector<slamhip_match_job> dj(n_dev);
    std::vector<int> dsid(n_dev);
    for (int c = 0; c < n_jobs; ++c)
      if (dev_of[c] >= 0) {
        dj[dev_of[c]] = jobs[c];
        dsid[dev_of[c]] = sid[c];
      }
    std::vector<BatchScanBlock> blocks(n_dev);
    int rc = hc_batch_stage_scans(m, n_dev, dj.data(), blocks.data());
    if (rc) return rc;
    b->res.assign(n_jobs, BatchJobResult{});
    b->kernels = 0;
    rc = bf_batch_run(m, n_dev, dj.data(), blocks.data(), dsid.data());
    if (rc) return rc;
    // (the sweeps' results by their place in the launch -> by job)
    std::vector<BatchJobResult> by_dev(b->res.begin(), b->res.begin() + n_dev);
    b->res.assign(n_jobs, BatchJobResult{});
    for (int c = 0; c < n_jobs; ++c)
      if (dev_of[c] >= 0) b->res[c] = by_dev[dev_of[c]];
    chains = false;  // (done)
  } else {
    dev_of.clear();
    b->res.assign(n_jobs, BatchJobResult{});
    b->kernels = 0;
  }
  if (chains) {
    std::vector<BatchScanBlock> blocks(n_jobs);
    int rc = hc_batch_stage_scans(m, n_jobs, jobs, blocks.data());
    if (rc) return rc;
    rc = mc_streams ? mc_batch_run(m, n_jobs, jobs, blocks.data(), sid.data(), cell_model)
                    : hc_batch_run(m, n_jobs, jobs, blocks.data(), cell_model);
    if (rc) return rc;
  }
  // a job the chains did not take or did not settle: its scan selected or uploaded as the current one, process_scan
  return batch_hand_over(
      m, n_jobs, jobs, sid, [&](int c) { return dev_of.empty() ? c : std::max(dev_of[c], 0); }, out_deltas, out_probs, nullptr,
      [&](const slamhip_match_job &j, ScanKeeper &keep, double *delta, double *prob, int *kept) -> int {
        keep.upload_overwritten = keep.upload_overwritten || j.scan_slot < 0;
        const int rc = j.scan_slot >= 0 ? slamhip_scan_select(ctx, j.scan_slot)
                                        : slamhip_scan_upload(ctx, j.n, j.range, j.cos_a, j.sin_a, j.weight, j.factor);
        if (rc) return rc;
        *kept = ctx->scan_n;
        return slamhip_matcher_process_scan(m, j.map_id, j.init_pose, delta, prob);
      });
}

int slamhip_matcher_batch_stats(slamhip_matcher *m, int job, long long *scorer_calls, long long *poses_evaluated,
                                long long *super_steps, int *on_device_chain) {
  if (!m || !m->batch || job < 0 || job >= (int)m->batch->res.size()) return invalid_arg("no such job in the last batch");
  const BatchJobResult &r = m->batch->res[job];
  if (scorer_calls) *scorer_calls = r.calls;
  if (poses_evaluated) *poses_evaluated = r.evaluated;
  if (super_steps) *super_steps = r.steps;
  if (on_device_chain) *on_device_chain = r.on_chain ? 1 : 0;
  return SLAMHIP_OK;
}

int slamhip_matcher_set_mc_streams(slamhip_matcher *m, int n_streams, const unsigned *seeds) {
  if (!m || n_streams < 0 || (n_streams > 0 && !seeds)) return invalid_arg("bad engine streams");
  if (!m->is_mc) return invalid_arg("engine streams belong to a Monte-Carlo matcher");
  const auto *own = static_cast<const GaussianPoseEnumerator *>(m->pe.get());
  std::vector<slamhip_matcher::McStream> streams(n_streams);
  for (int k = 0; k < n_streams; ++k)
    streams[k].pe = std::make_unique<GaussianPoseEnumerator>(seeds[k], own->base_td(), own->base_rd(), own->max_failed(),
                                                             own->max_poses());
  m->mc_streams.swap(streams);
  m->mc_job_streams.clear();
  m->mc.tape_owner = nullptr;  // (the lone chain's tape window may hold a stream's pairs that is gone now)
  return SLAMHIP_OK;
}

int slamhip_matcher_set_mc_job_streams(slamhip_matcher *m, int n, const int *stream_of_job) {
  if (!m || n < 0) return invalid_arg("bad stream mapping");
  if (!m->is_mc) return invalid_arg("engine streams belong to a Monte-Carlo matcher");
  if (!stream_of_job || n == 0) {
    m->mc_job_streams.clear();
    return SLAMHIP_OK;
  }
  const int ns = (int)m->mc_streams.size();
  if (n > ns) return invalid_arg("more jobs than engine streams (slamhip_matcher_set_mc_streams)");
  std::vector<char> used(ns, 0);
  for (int c = 0; c < n; ++c) {
    const int k = stream_of_job[c];
    if (k < 0 || k >= ns) return invalid_arg("a job's engine stream is out of range");
    if (used[k]) return invalid_arg("two jobs of one batch on the same engine stream");
    used[k] = 1;
  }
  m->mc_job_streams.assign(stream_of_job, stream_of_job + n);
  return SLAMHIP_OK;
}

int slamhip_matcher_mc_stream_info(slamhip_matcher *m, int stream, unsigned long long *pairs_consumed, long long *matches,
                                   double *state5) {
  if (!m || !m->is_mc) return invalid_arg("engine streams belong to a Monte-Carlo matcher");
  if (stream < -1 || stream >= (int)m->mc_streams.size()) return invalid_arg("no such engine stream");
  const auto *pe = static_cast<const GaussianPoseEnumerator *>(stream < 0 ? m->pe.get() : m->mc_streams[stream].pe.get());
  if (pairs_consumed) *pairs_consumed = (unsigned long long)pe->tape_pos();
  if (matches) *matches = stream < 0 ? m->mc_matches : m->mc_streams[stream].matches;
  if (state5) pe->state5(state5);
  return SLAMHIP_OK;
}

int slamhip_matcher_set_bf_streams(slamhip_matcher *m, int n_streams) {
  if (!m || n_streams < 0) return invalid_arg("bad enumerator streams");
  if (!m->is_bf) return invalid_arg("enumerator streams belong to a brute-force matcher");
  m->bf_streams.set(n_streams);  // (every base forgotten, the job mapping dropped)
  return SLAMHIP_OK;
}

int slamhip_matcher_set_bf_job_streams(slamhip_matcher *m, int n, const int *stream_of_job) {
  if (!m || n < 0) return invalid_arg("bad stream mapping");
  if (!m->is_bf) return invalid_arg("enumerator streams belong to a brute-force matcher");
  if (const char *why = m->bf_streams.set_job_streams(n, stream_of_job)) return invalid_arg(why);
  return SLAMHIP_OK;
}

int slamhip_matcher_bf_stream_info(slamhip_matcher *m, int stream, int *base_set, double base[3], long long *matches) {
  if (!m || !m->is_bf) return invalid_arg("enumerator streams belong to a brute-force matcher");
  if (stream < -1 || stream >= (int)m->bf_streams.s.size()) return invalid_arg("no such enumerator stream");
  BfStream own;  // (stream -1: the matcher's own enumerator, the one the lone calls use)
  if (stream < 0) {
    const auto *pe = static_cast<const BruteForcePoseEnumerator *>(m->pe.get());
    own.base_set = pe->base_set();
    own.base[0] = pe->base().x;
    own.base[1] = pe->base().y;
    own.base[2] = pe->base().theta;
    own.matches = m->bf_matches;
  }
  const BfStream &k = stream < 0 ? own : m->bf_streams.s[(size_t)stream];
  if (base_set) *base_set = k.base_set ? 1 : 0;
  if (base)
    for (int q = 0; q < 3; ++q) base[q] = k.base_set ? k.base[q] : 0.0;
  if (matches) *matches = k.matches;
  return SLAMHIP_OK;
}

// ---- the peaks of a sweep's score landscape (bf_peaks.h, bf_peaks.hip) ---------------------------------------------
// The lattice a BruteForcePoseEnumerator with base `centre` hands out, scored as the sweep scores it, and reduced on the
// device to its local maxima above the floors, best first.  Nothing of the matcher's own state takes part: not the
// enumerator or its latch, not the enumerator streams, the observer or a counter of slamhip_matcher_stats.
namespace {

int unsupported(const char *msg) {
  set_error(msg);
  return SLAMHIP_ERR_UNSUPPORTED;
}

// the rule's own arguments (both the host entry and the device calls)
int bf_peaks_rule_args(const int radius[3], double min_ratio, double min_score, int max_peaks) {
  for (int k = 0; k < 3; ++k)
    if (radius[k] < 0 || radius[k] > kBfPeaksMaxRadius) return invalid_arg("a peak window's radius lies in 0 ... 32 on every axis");
  if (max_peaks < 0 || max_peaks > kBfPeaksMaxSurvivors) return invalid_arg("max_peaks lies in 0 ... 8192");
  if (!(min_ratio >= 0.0 && min_ratio <= 1.0)) return invalid_arg("min_ratio lies in [0, 1]");
  if (min_score != min_score) return invalid_arg("min_score is NaN");
  return SLAMHIP_OK;
}

// everything a peaks call is refused for before the device is asked for anything but the matcher's offsets; *bound: B
int bf_peaks_check(slamhip_matcher *m, const int radius[3], double min_ratio, double min_score, int max_peaks, long long *bound) {
  if (!m->is_bf) return invalid_arg("the peaks of a sweep belong to a brute-force matcher");
  int rc = bf_peaks_rule_args(radius, min_ratio, min_score, max_peaks);
  if (rc) return rc;
  if (m->cfg.oope == SLAMHIP_OOPE_GMAPPING) return unsupported("the peaks of a sweep: the GMapping OOPE is not covered");
  if (m->cfg.sum_order != SLAMHIP_SUM_TREE256) return unsupported("the peaks of a sweep: the beam-order sum is not covered");
  if (m->cfg.pose_trig != SLAMHIP_POSE_TRIG_DEVICE) return unsupported("the peaks of a sweep: device pose trigonometry only");
  rc = bf_sweep_offsets(m);
  if (rc == kChainNeedsHost) return unsupported("the peaks of a sweep: an axis of the sweep is too long");
  if (rc) return rc;
  const slamhip_matcher::BfSweep &bf = m->bf;
  if (bf.nx <= 0 || bf.ny <= 0 || bf.nt <= 0) return invalid_arg("the sweep is empty");
  if (1 + (long long)bf.nx * bf.ny * bf.nt > (1ll << 26)) return unsupported("the peaks of a sweep: more than 2^26 poses");
  *bound = bf_peaks_bound(bf.nx, bf.ny, bf.nt, radius);
  if (*bound > kBfPeaksMaxSurvivors)
    return invalid_arg("more than 8192 peaks are possible: widen the radius or narrow the sweep");
  return SLAMHIP_OK;
}

// the scratch of n_jobs volumes of np scores each (lone_poses: a pose array for launch_score as well)
int bf_peaks_room(slamhip_matcher *m, int n_jobs, long long np, long long bound, int max_peaks, bool lone_poses) {
  hipStream_t st = m->ctx->stream;
  if (!m->bf_peaks) m->bf_peaks = std::make_unique<BfPeaksScratch>();
  BfPeaksScratch *s = m->bf_peaks.get();
  int rc = grow_blocks({st}, s->job_cap, (size_t)n_jobs, 8, [&](size_t cap) -> int {
    SLAMHIP_CHECK(s->h_jobs.alloc(cap, hipHostMallocDefault));
    SLAMHIP_CHECK(s->d_jobs.alloc(cap));
    SLAMHIP_CHECK(s->d_job_max.alloc(cap));
    SLAMHIP_CHECK(s->d_job_count.alloc(cap));
    // (zero between calls: k_bf_peaks_order clears what its call used)
    SLAMHIP_CHECK(hipMemsetAsync(s->d_job_max.get(), 0, sizeof(unsigned long long) * cap, st));
    SLAMHIP_CHECK(hipMemsetAsync(s->d_job_count.get(), 0, sizeof(unsigned) * cap, st));
    SLAMHIP_CHECK(s->h_hdr.alloc(cap, kPinnedCoherent));
    return SLAMHIP_OK;
  });
  if (!rc) rc = grow_blocks({st}, s->pose_cap, (size_t)(n_jobs * np), 1 << 14, [&](size_t cap) -> int {
    SLAMHIP_CHECK(s->d_scores.alloc(cap));
    SLAMHIP_CHECK(s->d_plane_s.alloc(cap));
    SLAMHIP_CHECK(s->d_plane_i.alloc(cap));
    return SLAMHIP_OK;
  });
  if (!rc) rc = grow_blocks({st}, s->surv_cap, (size_t)(n_jobs * bound), 1 << 10, [&](size_t cap) -> int {
    SLAMHIP_CHECK(s->d_surv.alloc(cap));
    return SLAMHIP_OK;
  });
  if (!rc) rc = grow_blocks({st}, s->out_cap, (size_t)n_jobs * (size_t)std::max(max_peaks, 1), 1 << 8, [&](size_t cap) -> int {
    SLAMHIP_CHECK(s->h_out.alloc(cap, kPinnedCoherent));
    return SLAMHIP_OK;
  });
  if (!rc && lone_poses) rc = grow_blocks({st}, s->lone_cap, (size_t)np, 1 << 14, [&](size_t cap) -> int {
    SLAMHIP_CHECK(s->d_poses.alloc(3 * cap));
    return SLAMHIP_OK;
  });
  return rc;
}

// Behind the last refusal of a call and in front of its first launch: the stats become this call's, and scratch words a
// failed call left behind are cleared.
int bf_peaks_begin(slamhip_matcher *m, long long bound, bool shared) {
  BfPeaksScratch *s = m->bf_peaks.get();
  if (s->words_unknown) {
    SLAMHIP_CHECK(hipMemsetAsync(s->d_job_max.get(), 0, sizeof(unsigned long long) * (size_t)s->job_cap, m->ctx->stream));
    SLAMHIP_CHECK(hipMemsetAsync(s->d_job_count.get(), 0, sizeof(unsigned) * (size_t)s->job_cap, m->ctx->stream));
    s->words_unknown = false;
  }
  s->launches = 0;
  s->bound = bound;
  s->shared = shared ? 1 : 0;
  return SLAMHIP_OK;
}

// one job's np poses -- the centre, then the lattice around it, by the sweep's own kernel -- scored through launch_score
// into its slab, as bf_device_process_scan scores a sweep
int bf_peaks_score_job(slamhip_matcher *m, ScoreArgs a, int cell_model, int oie_eff, const double centre[3], long long np,
                       double *slab) {
  BfPeaksScratch *s = m->bf_peaks.get();
  BfPoseArgs pa;
  for (int k = 0; k < 3; ++k) pa.init[k] = pa.base[k] = centre[k];
  pa.off = m->bf.d_off.get();
  pa.nx = m->bf.nx;
  pa.ny = m->bf.ny;
  pa.nt = m->bf.nt;
  pa.n = np;
  pa.poses = s->d_poses.get();
  SLAMHIP_CHECK(launch_bf_poses(pa, m->ctx->stream));
  ++s->launches;
  a.poses = s->d_poses.get();
  a.pose_sc = nullptr;
  a.scores = slab;
  a.n_poses = (int)np;
  a.poses_per_block = 0;
  a.oie = oie_eff;
  for (int k = 0; k < 4; ++k) a.area[k] = m->cfg.area[k];
  a.gm.fullness_th = m->cfg.gm_fullness_th;
  a.gm.window = m->cfg.gm_window;
  a.fprints = nullptr;
  SLAMHIP_CHECK(launch_score(a, cell_model, m->cfg.oope, m->cfg.sum_order, m->ctx->stream));
  ++s->launches;
  return SLAMHIP_OK;
}

// the peaks kernels over the n_jobs volumes that lie scored in the scratch, the wait, and the hand-over: per job its
// counts and its first max_peaks peaks, their poses made by the enumerator's additions around the job's centre
int bf_peaks_reduce(slamhip_matcher *m, int n_jobs, long long np, long long bound, const int radius[3], double min_ratio,
                    double min_score, int max_peaks, const double *centres, slamhip_bf_peak *peaks_out, int *n_written,
                    long long *n_found) {
  BfPeaksScratch *s = m->bf_peaks.get();
  const slamhip_matcher::BfSweep &bf = m->bf;
  BfPeaksArgs a;
  std::memset(&a, 0, sizeof(a));
  a.volumes = s->d_scores.get() + 1;  // (score 0 of a slab is the centre's own: not part of the lattice)
  a.job_stride = np;
  a.nx = bf.nx;
  a.ny = bf.ny;
  a.nt = bf.nt;
  a.rx = radius[0];
  a.ry = radius[1];
  a.rt = radius[2];
  a.n_jobs = n_jobs;
  a.max_peaks = max_peaks;
  a.min_ratio = min_ratio;
  a.min_score = min_score;
  a.bound = bound;
  a.plane_s = s->d_plane_s.get();
  a.plane_i = s->d_plane_i.get();
  a.job_max = s->d_job_max.get();
  a.job_count = s->d_job_count.get();
  a.survivors = s->d_surv.get();
  a.out_hdr = s->h_hdr.get();
  a.out = s->h_out.get();
  s->words_unknown = true;
  SLAMHIP_CHECK(launch_bf_peaks(a, m->ctx->stream, &s->launches));
  SLAMHIP_CHECK(hipStreamSynchronize(m->ctx->stream));
  s->words_unknown = false;
  for (int c = 0; c < n_jobs; ++c) {
    const BfPeaksHostOut &h = s->h_hdr.get()[c];
    n_found[c] = h.n_found;
    n_written[c] = (int)h.n_written;
    for (long long q = 0; q < h.n_written; ++q) {
      const BfPeakKey &k = s->h_out.get()[(size_t)c * (size_t)max_peaks + (size_t)q];
      slamhip_bf_peak &p = peaks_out[(size_t)c * (size_t)max_peaks + (size_t)q];
      bf_pose_of_host(bf, centres + 3 * c, centres + 3 * c, k.index + 1, p.pose);
      p.score = k.score;
      p.index = k.index;
    }
  }
  return SLAMHIP_OK;
}

}  // namespace

int slamhip_bf_peaks_host(const double *scores, int nx, int ny, int nt, const int radius[3], double min_ratio, double min_score,
                          int max_peaks, long long *index_out, double *score_out, int *n_written, long long *n_found) {
  if (!scores || !radius || !n_written || !n_found || (max_peaks > 0 && (!index_out || !score_out))) return invalid_arg("null argument");
  if (nx <= 0 || ny <= 0 || nt <= 0 || (long long)nx * ny * nt > (1ll << 26)) return invalid_arg("bad volume shape");
  const int rc = bf_peaks_rule_args(radius, min_ratio, min_score, max_peaks);
  if (rc) return rc;
  if (bf_peaks_bound(nx, ny, nt, radius) > kBfPeaksMaxSurvivors)
    return invalid_arg("more than 8192 peaks are possible: widen the radius or narrow the sweep");
  std::vector<BfPeakKey> kept;
  bf_peaks_separable(scores, nx, ny, nt, radius, min_ratio, min_score, &kept);
  *n_found = (long long)kept.size();
  *n_written = (int)std::min<size_t>(kept.size(), (size_t)max_peaks);
  for (int q = 0; q < *n_written; ++q) {
    index_out[q] = kept[(size_t)q].index;
    score_out[q] = kept[(size_t)q].score;
  }
  return SLAMHIP_OK;
}

int slamhip_matcher_bf_peaks(slamhip_matcher *m, int map_id, const double centre[3], const int radius[3], double min_ratio,
                             double min_score, int max_peaks, slamhip_bf_peak *peaks_out, int *n_written, long long *n_found,
                             int shape_out[3]) {
  if (!m || !centre || !radius || !n_written || !n_found || (max_peaks > 0 && !peaks_out)) return invalid_arg("null argument");
  slamhip_ctx *ctx = m->ctx;
  SLAMHIP_CHECK(hipSetDevice(ctx->device));
  long long bound = 0;
  int rc = bf_peaks_check(m, radius, min_ratio, min_score, max_peaks, &bound);
  if (rc) return rc;
  const long long np = 1 + (long long)m->bf.nx * m->bf.ny * m->bf.nt;
  ScoreArgs a;
  std::memset(&a, 0, sizeof(a));
  int cell_model = 0, oie_eff = m->cfg.oie;
  rc = score_views(ctx, map_id, &m->cfg, &a.map, &a.scan, &cell_model, nullptr, &oie_eff);  // (TBM: through the plane)
  if (rc) return rc;
  rc = bf_peaks_room(m, 1, np, bound, max_peaks, true);
  if (!rc) rc = bf_peaks_begin(m, bound, false);
  if (rc) return rc;
  rc = bf_peaks_score_job(m, a, cell_model, oie_eff, centre, np, m->bf_peaks->d_scores.get());
  if (rc) return rc;
  rc = bf_peaks_reduce(m, 1, np, bound, radius, min_ratio, min_score, max_peaks, centre, peaks_out, n_written, n_found);
  if (rc) return rc;
  if (shape_out) {
    shape_out[0] = m->bf.nx;
    shape_out[1] = m->bf.ny;
    shape_out[2] = m->bf.nt;
  }
  return SLAMHIP_OK;
}

int slamhip_matcher_bf_peaks_batch(slamhip_matcher *m, int n_jobs, const slamhip_match_job *jobs, const int radius[3],
                                   double min_ratio, double min_score, int max_peaks, slamhip_bf_peak *peaks_out, int *n_written,
                                   long long *n_found) {
  if (!m || n_jobs < 0 || !radius || (n_jobs > 0 && (!jobs || !n_written || !n_found || (max_peaks > 0 && !peaks_out))))
    return invalid_arg("null argument");
  if (n_jobs > 65535) return invalid_arg("more than 65535 jobs");
  slamhip_ctx *ctx = m->ctx;
  SLAMHIP_CHECK(hipSetDevice(ctx->device));
  long long bound = 0;
  int rc = bf_peaks_check(m, radius, min_ratio, min_score, max_peaks, &bound);
  if (rc) return rc;
  if (n_jobs == 0) return SLAMHIP_OK;
  const long long np = 1 + (long long)m->bf.nx * m->bf.ny * m->bf.nt;
  if ((long long)n_jobs * np > kBfBatchMaxPoses) return invalid_arg("the batch's sweeps hold more than 2^24 poses");
  int max_n = 0;
  for (int c = 0; c < n_jobs; ++c) {
    const slamhip_match_job &j = jobs[c];
    if (j.scan_slot >= 0) {
      if (j.scan_slot >= (int)ctx->scan_slots.size() || !ctx->scan_slots[j.scan_slot].d)
        return invalid_arg("a match job names a scan slot nothing is stored in");
    } else if (j.n <= 0 || !j.range || !j.cos_a || !j.sin_a || !j.weight) {
      return invalid_arg("bad scan in a match job");
    }
    max_n = std::max(max_n, j.scan_slot >= 0 ? ctx->scan_slots[j.scan_slot].n : j.n);
  }
  rc = batch_maps_check(ctx, n_jobs, jobs, nullptr);
  if (rc) return rc;
  // the views a lone call of each job scores through; ONE launch scores all jobs where k_bf_score_batch covers them: the
  // 1-cell OOPE, one effective cell model and OIE, at most 4096 beams a job
  std::vector<MapView> maps(n_jobs);
  std::vector<int> models(n_jobs), oies(n_jobs);
  std::vector<double> centres(3 * (size_t)n_jobs);
  bool shared = m->cfg.oope == SLAMHIP_OOPE_OBSTACLE && max_n <= kBfBatchMaxBeams;
  for (int c = 0; c < n_jobs; ++c) {
    rc = score_map_view(ctx, jobs[c].map_id, &m->cfg, &maps[c], &models[c], &oies[c]);
    if (rc) return rc;
    if (models[c] != models[0] || oies[c] != oies[0]) shared = false;
    for (int q = 0; q < 3; ++q) centres[3 * (size_t)c + q] = jobs[c].init_pose[q];
  }
  rc = bf_peaks_room(m, n_jobs, np, bound, max_peaks, !shared);
  if (rc) return rc;
  if (!m->batch) m->batch = std::make_unique<HcBatch>();  // (its scan arena: hc_batch_stage_scans)
  std::vector<BatchScanBlock> blocks(n_jobs);
  rc = hc_batch_stage_scans(m, n_jobs, jobs, blocks.data());
  if (rc) return rc;
  BfPeaksScratch *s = m->bf_peaks.get();
  rc = bf_peaks_begin(m, bound, shared);
  if (rc) return rc;
  if (shared) {
    for (int c = 0; c < n_jobs; ++c) {
      BfJobView &v = s->h_jobs.get()[c];
      std::memset(&v, 0, sizeof(v));
      v.map = maps[c];
      v.scan = scan_view_of(blocks[c].d, blocks[c].stride, blocks[c].n, blocks[c].tot_w);
      for (int q = 0; q < 3; ++q) v.init[q] = v.base[q] = centres[3 * (size_t)c + q];
      v.at = (long long)c * np;
    }
    SLAMHIP_CHECK(hipMemcpyAsync(s->d_jobs.get(), s->h_jobs.get(), sizeof(BfJobView) * (size_t)n_jobs, hipMemcpyHostToDevice,
                                 ctx->stream));
    BfBatchArgs a;
    std::memset(&a, 0, sizeof(a));
    a.jobs = s->d_jobs.get();
    a.off = m->bf.d_off.get();
    a.nx = m->bf.nx;
    a.ny = m->bf.ny;
    a.nt = m->bf.nt;
    a.n = (int)np;
    a.n_jobs = n_jobs;
    a.oie = oies[0];
    a.scores = s->d_scores.get();
    SLAMHIP_CHECK(launch_bf_batch_score(a, models[0], max_n, ctx->stream));
    ++s->launches;
  } else {
    for (int c = 0; c < n_jobs; ++c) {
      ScoreArgs a;
      std::memset(&a, 0, sizeof(a));
      a.map = maps[c];
      a.scan = scan_view_of(blocks[c].d, blocks[c].stride, blocks[c].n, blocks[c].tot_w);
      rc = bf_peaks_score_job(m, a, models[c], oies[c], &centres[3 * (size_t)c], np, s->d_scores.get() + (size_t)c * (size_t)np);
      if (rc) return rc;
    }
  }
  rc = bf_peaks_reduce(m, n_jobs, np, bound, radius, min_ratio, min_score, max_peaks, centres.data(), peaks_out, n_written,
                       n_found);
  return rc;
}

int slamhip_matcher_bf_peaks_stats(slamhip_matcher *m, long long *launches, long long *survivors_bound, int *on_shared_launch) {
  if (!m || !m->is_bf) return invalid_arg("the peaks of a sweep belong to a brute-force matcher");
  const BfPeaksScratch none;
  const BfPeaksScratch &s = m->bf_peaks ? *m->bf_peaks : none;
  if (launches) *launches = s.launches;
  if (survivors_bound) *survivors_bound = s.bound;
  if (on_shared_launch) *on_shared_launch = s.shared;
  return SLAMHIP_OK;
}

#ifdef SLAMHIP_TESTING
// testing aid, not part of include/slamhip.h: the shared Monte-Carlo launches speculate on `slots` candidates per job
// and super-step instead of what mc_batch_slots picks (0: the rule again) -- the results must not depend on it
// (named *_testing_*: the list of *debug* hooks of the testing library is pinned by tests/test_host_abi.py)
int slamhip_matcher_testing_mc_batch_slots(slamhip_matcher *m, int slots) {
  if (!m || slots < 0) return invalid_arg("bad slot count");
  m->debug_mc_batch_slots = slots;
  return SLAMHIP_OK;
}
// testing aid, not part of include/slamhip.h: the hill-climbing chain treats its observer trace buffer as `cap`
// entries long (0 = its real size), so that the overflow path -- the match redone by the host-driven matcher --
// can be exercised without a 65536-call match
int slamhip_matcher_debug_trace_cap(slamhip_matcher *m, int cap) {
  if (!m || cap < 0) return invalid_arg("bad trace cap");
  m->debug_trace_cap = cap;
  return SLAMHIP_OK;
}
#endif  // SLAMHIP_TESTING

int slamhip_matcher_stats(slamhip_matcher *m, long long *scorer_calls, long long *poses_evaluated,
                          long long *launches) {
  if (!m) return invalid_arg("null matcher");
  if (scorer_calls) *scorer_calls = m->job.scorer_calls;
  if (poses_evaluated) *poses_evaluated = m->job.poses_evaluated;
  if (launches) *launches = m->job.launches;
  return SLAMHIP_OK;
}

int slamhip_matcher_process_raw_scan(slamhip_matcher *m, int map_id, const slamhip_raw_scan *scan, const double init_pose[3],
                                     double out_delta[3], double *out_prob, int *kept_n) {
  if (!m || !scan || !init_pose || !out_delta || !out_prob) return invalid_arg("null argument");
  int kept = 0;
  SLAMHIP_MATCH_END(m, 0);
  // the first half of slamhip_scan_filter_upload: filter and staging.  Who writes the scan block is decided where the
  // match is launched: the lone co-resident hill-climbing chain does it itself (chain_process_scan), every other path
  // goes through scan_assemble_now before its first kernel.
  int rc = scan_filter_stage(m->ctx, map_id, scan->n, scan->range, scan->angle, scan->is_occ, scan->factor, scan->trig_mode,
                             scan->a_min, scan->a_max, scan->a_inc, init_pose, scan->skip_rate, scan->max_range,
                             scan->bounded, scan->weighting, &kept, nullptr);
  SLAMHIP_MATCH_END(m, 1);
  if (kept_n) *kept_n = kept;
  if (rc) return rc;
  if (kept == 0) {  // 0 / 0 for every candidate (weighted_mean_point_probability_spe.h:126-132): nothing is accepted
    if (m->is_m3rsm) m->job.scorer_calls = m->job.poses_evaluated = m->job.launches = 0;  // (its stats are per match)
    out_delta[0] = out_delta[1] = out_delta[2] = 0.0;
    *out_prob = std::numeric_limits<double>::quiet_NaN();
    return SLAMHIP_OK;
  }
  rc = slamhip_matcher_process_scan(m, map_id, init_pose, out_delta, out_prob);
#ifdef SLAMHIP_TESTING
  if (!rc && m->is_hc && !m->has_obs && m->debug_ends[2] > m->debug_ends[1]) {
    m->job.t_build_us = m->debug_ends[1] - m->debug_ends[0];
    m->t_stage_us = m->debug_ends[2] - m->debug_ends[1];
    m->job.t_replay_us = m->debug_ends[4] - m->debug_ends[3];
  }
#endif
  // (a match that failed before it launched anything: the scan is the current one all the same, its block gets written)
  const int arc = scan_assemble_now(m->ctx);
  return rc ? rc : arc;
}

// K raw scans, K matches in the shared launches.  The host half per job is the lone call's (scan_filter.h); the scans
// reach HBM through RawDeviceStage's ONE assembly launch in front of the chains' launch, which reads the call's pinned
// arena: kept ranges, kept indices, factors, ahr weights and the table of per-job ScanAssembleArgs.  The arena is
// refilled by the next call only: this one returns after its chains have reported their results, the chains were
// launched on the same stream behind the assembly kernel, so the kernel has read the arena by then -- no flag.
int slamhip_matcher_process_raw_scan_batch(slamhip_matcher *m, int n_jobs, const slamhip_raw_match_job *jobs,
                                           double *out_deltas, double *out_probs, int *kept_n) {
  if (!m || n_jobs < 0 || (n_jobs > 0 && (!jobs || !out_deltas || !out_probs))) return invalid_arg("null argument");
  if (n_jobs == 0) return SLAMHIP_OK;
  if (m->is_m3rsm) return invalid_arg("multi-resolution matches are not batched");
  slamhip_ctx *ctx = m->ctx;
  // ---- every check in front of the first launch: the arguments, the maps, the scanners' tables (prepare)
  for (int c = 0; c < n_jobs; ++c) {
    if (const int bad = RawDeviceStage::check_scan(jobs[c].scan)) return invalid_arg(kBadRawJob[bad]);
    if (jobs[c].map_id < 0 || jobs[c].map_id >= (int)ctx->maps.size() || !ctx->maps[jobs[c].map_id].bound)
      return invalid_arg("unknown map id in a match job");
  }
  const bool mc_streams = m->is_mc && !m->mc_streams.empty();
  const bool bf_streams = m->is_bf && m->bf_streams.any();
  const bool streams = mc_streams || bf_streams;
  std::vector<int> sid;
  if (mc_streams) {  // (refused before a stream or the last-batch state is touched)
    const int rc = mc_job_streams_of(m, n_jobs, &sid);
    if (rc) return rc;
  }
  if (bf_streams) {
    const int rc = bf_job_streams_of(m, n_jobs, &sid);
    if (rc) return rc;
  }
  SLAMHIP_CHECK(hipSetDevice(ctx->device));
  if (!m->batch) m->batch = std::make_unique<HcBatch>();
  HcBatch *b = m->batch.get();
  RawDeviceStage &stage = b->raw;
  const RawBatchStage &raw = stage.host;
  const bool planned = n_jobs > 1;  // (a batch of one is the lone call, which checks for itself)
  bool on_chains = false;
  if (planned) {
    std::vector<RawBatchJob> in(n_jobs);
    for (int c = 0; c < n_jobs; ++c) {
      const DeviceMap &dm = ctx->maps[jobs[c].map_id];
      in[c] = RawBatchStage::job_of(jobs[c].scan, jobs[c].init_pose, ScanWindow{dm.scale, dm.origin_x, dm.origin_y, dm.width, dm.height});
    }
    int rc = stage.prepare(n_jobs, in.data(), sizeof(ScanAssembleArgs), 5);
    if (rc) return invalid_arg(scan_error_text(rc));
    // the jobs that kept something, and whether the shared launches take them
    struct LiveJob {
      int map_id;
      double init_pose[3];
    };
    std::vector<LiveJob> live(raw.n_live);
    for (int c = 0; c < n_jobs; ++c) {
      if (raw.plan[c].live < 0) continue;
      LiveJob &l = live[raw.plan[c].live];
      l.map_id = jobs[c].map_id;
      for (int q = 0; q < 3; ++q) l.init_pose[q] = jobs[c].init_pose[q];
    }
    std::vector<int> live_sid(streams ? raw.n_live : 0);
    for (int c = 0; c < n_jobs && streams; ++c)
      if (raw.plan[c].live >= 0) live_sid[raw.plan[c].live] = sid[c];
    // (a brute-force matcher without streams: job after job through the lone call.  With streams a raw batch goes
    // through the shared sweeps whole or not at all: one job above 4096 kept beams sends every job to its lone call)
    bool chains = raw.n_live > 1 && raw.n_live <= 65535 && raw.max_k <= 4096 && (!m->is_bf || bf_streams) &&
                  (mc_streams ? mc_batch_eligible(m) : (bf_streams ? bf_batch_eligible(m) : batch_chain_eligible(m)));
    int cell_model = -1;
    if (chains) {
      rc = batch_maps_check(ctx, raw.n_live, live.data(), &cell_model);
      if (rc) return rc;
      if (bf_streams) {
        rc = bf_batch_fits(m, raw.n_live, &chains);
        if (rc) return rc;
      }
    }
    if (chains) {
      // (the arena is filled only now that the shared launches take the jobs; the stream is idle: the batch before
      // returned after its chains had ended)
      rc = stage.assemble<ScanAssembleArgs>(ctx, in.data());
      if (rc) return rc;
      std::vector<BatchScanBlock> blocks(raw.n_live);
      for (int c = 0; c < n_jobs; ++c) {
        const RawBatchPlan &p = raw.plan[c];
        if (p.live >= 0) blocks[p.live] = BatchScanBlock{stage.blocks[c].d, p.stride, p.k, p.tot_w};
      }
      b->res.assign(n_jobs, BatchJobResult{});
      b->kernels = 0;
      rc = mc_streams ? mc_batch_run(m, raw.n_live, live.data(), blocks.data(), live_sid.data(), cell_model)
                      : (bf_streams ? bf_batch_run(m, raw.n_live, live.data(), blocks.data(), live_sid.data())
                                    : hc_batch_run(m, raw.n_live, live.data(), blocks.data(), cell_model));
      if (rc) return rc;
      if (bf_streams) ++b->kernels;  // (k_scan_assemble_table in front of the three)
      live_to_job(raw.plan, b->res, BatchJobResult{});  // (the chains' results by live place -> by job)
      on_chains = true;
    }
  }
  if (!on_chains) {  // (every job that kept something goes through the lone call below)
    b->res.assign(n_jobs, BatchJobResult{});
    b->kernels = 0;
    stage.blocks.assign(n_jobs, RawDeviceStage::Block{});
  }
  // a job the chains did not take or did not settle: the lone raw call, which filters its scan into the upload buffer
  return batch_hand_over(
      m, n_jobs, jobs, sid, [&](int c) { return planned ? raw.plan[c].live : 0; }, out_deltas, out_probs, kept_n,
      [&](const slamhip_raw_match_job &j, ScanKeeper &keep, double *delta, double *prob, int *kept) -> int {
        keep.upload_overwritten = true;
        return slamhip_matcher_process_raw_scan(m, j.map_id, &j.scan, j.init_pose, delta, prob, kept);
      });
}

int slamhip_matcher_batch_scan_download(slamhip_matcher *m, int job, int cap, double *out5, int *n) {
  if (!m || !n || cap < 0 || (cap > 0 && !out5)) return invalid_arg("bad arguments");
  if (!m->batch || job < 0 || job >= (int)m->batch->raw.blocks.size()) return invalid_arg("no such job in the last raw batch");
  return m->batch->raw.download(m->ctx, job, cap, out5, nullptr, n,
                                "slamhip_matcher_batch_scan_download: room for fewer points than the job's scan has");
}

int slamhip_matcher_tail_stats(slamhip_matcher *m, long long *calls_closed_form) {
  if (!m || !calls_closed_form) return invalid_arg("null argument");
  *calls_closed_form = m->tail_calls;
  return SLAMHIP_OK;
}

int slamhip_matcher_chain_stats(slamhip_matcher *m, long long *kernels_launched, long long *steps_rescored) {
  if (!m) return invalid_arg("null matcher");
  if (kernels_launched) *kernels_launched = m->chain_launched;
  if (steps_rescored) *steps_rescored = m->chain_rescored;
  return SLAMHIP_OK;
}

#ifdef SLAMHIP_TESTING
// testing aid: the next `n` slamhip_matcher_process_scan calls of this matcher fail with SLAMHIP_ERR_HIP before anything
// is launched -- what a transient device error looks like to the caller (the adapters' failure semantics,
// host/slamhip_reference_adapter.h)
int slamhip_matcher_debug_fail_next(slamhip_matcher *m, int n) {
  if (!m || n < 0) return invalid_arg("bad count");
  m->debug_fail_next = n;
  return SLAMHIP_OK;
}
// testing aid, not part of include/slamhip.h: workgroup `slot_plus_1 - 1` of the following co-resident launches leaves
// at once (0 = none) -- what a workgroup that never became resident looks like to the others.
// A NEGATIVE argument delays instead (the lone and batched 1-cell / window chains, hc_resident.hip):
// -(workgroup + 1 + 65536 (every + 16 phase)), workgroup + 1 == 0xffff for the bookkeeping one: that workgroup is
// ~2 us late with its granule in the super-steps k with k % every == phase; nothing gives up
int slamhip_matcher_debug_resident_mute(slamhip_matcher *m, int slot_plus_1) {
  if (!m) return invalid_arg("null matcher");
  m->debug_resident_mute = slot_plus_1;
  return SLAMHIP_OK;
}
// testing aid: the state of a dense GMAPPING window's neighbourhood masks (MapView) -- *valid: whether the map holds
// masks at all; *mismatches: cells whose stored mask differs from the one the occupancies around them give
int slamhip_map_debug_nbr_masks(slamhip_ctx *ctx, int map_id, int *valid, long long *mismatches) {
  if (!ctx || map_id < 0 || map_id >= (int)ctx->maps.size() || !ctx->maps[map_id].bound) return invalid_arg("unknown map id");
  DeviceMap &dm = ctx->maps[map_id];
  if (valid) *valid = dm.nbr_ok ? 1 : 0;
  if (mismatches) *mismatches = 0;
  if (!dm.nbr_ok || !mismatches) return SLAMHIP_OK;
  SLAMHIP_CHECK(hipSetDevice(ctx->device));
  DeviceBuf<unsigned long long> d_count;
  unsigned long long h_count = 0;
  SLAMHIP_CHECK(d_count.alloc(1));
  SLAMHIP_CHECK(hipMemsetAsync(d_count.get(), 0, sizeof(unsigned long long), ctx->stream));
  SLAMHIP_CHECK(launch_nbr_check(dm.d_payload, dm.width, dm.height, dm.pitch, dm.nbr_th, d_count.get(), ctx->stream));
  SLAMHIP_CHECK(hipMemcpyAsync(&h_count, d_count.get(), sizeof(h_count), hipMemcpyDeviceToHost, ctx->stream));
  SLAMHIP_CHECK(hipStreamSynchronize(ctx->stream));
  *mismatches = (long long)h_count;
  return SLAMHIP_OK;
}
// testing aid: the state of a TBM map's probability plane (DeviceMap::d_prob) -- *valid: whether the map holds one;
// *mismatches: cells whose stored probability is not, bit for bit, the one their four belief masses give
int slamhip_map_debug_prob_plane(slamhip_ctx *ctx, int map_id, int *valid, long long *mismatches) {
  if (!ctx || map_id < 0 || map_id >= (int)ctx->maps.size() || !ctx->maps[map_id].bound) return invalid_arg("unknown map id");
  DeviceMap &dm = ctx->maps[map_id];
  if (valid) *valid = dm.prob_ok ? 1 : 0;
  if (mismatches) *mismatches = 0;
  if (!dm.prob_ok || !mismatches) return SLAMHIP_OK;
  DeviceBuf<unsigned long long> d_count;
  unsigned long long h_count = 0;
  SLAMHIP_CHECK(d_count.alloc(1));
  SLAMHIP_CHECK(hipMemsetAsync(d_count.get(), 0, sizeof(unsigned long long), ctx->stream));
  SLAMHIP_CHECK(launch_prob_check(dm.cell_model, dm.d_payload, dm.d_prob, dm.width, dm.height, dm.pitch, d_count.get(), ctx->stream));
  SLAMHIP_CHECK(hipMemcpyAsync(&h_count, d_count.get(), sizeof(h_count), hipMemcpyDeviceToHost, ctx->stream));
  SLAMHIP_CHECK(hipStreamSynchronize(ctx->stream));
  *mismatches = (long long)h_count;
  return SLAMHIP_OK;
}
#endif  // SLAMHIP_TESTING

int slamhip_matcher_resident_stats(slamhip_matcher *m, long long *matches, long long *gave_up) {
  if (!m) return invalid_arg("null matcher");
  if (matches) *matches = m->resident.matches;
  if (gave_up) *gave_up = m->resident.gave_up;
  return SLAMHIP_OK;
}

int slamhip_matcher_timing(slamhip_matcher *m, double *build_us, double *stage_us, double *score_us,
                           double *replay_us) {
  if (!m) return invalid_arg("null matcher");
  if (build_us) *build_us = m->job.t_build_us;
  if (stage_us) *stage_us = m->t_stage_us;
  if (score_us) *score_us = m->t_score_us;
  if (replay_us) *replay_us = m->job.t_replay_us;
  return SLAMHIP_OK;
}

static int process_scan_body(slamhip_matcher *m, int map_id, const double init_pose[3], double out_delta[3],
                             double *out_prob);

int slamhip_matcher_process_scan(slamhip_matcher *m, int map_id, const double init_pose[3],
                                 double out_delta[3], double *out_prob) {
  if (!m || !init_pose || !out_delta || !out_prob) return invalid_arg("null argument");
  const int rc = process_scan_body(m, map_id, init_pose, out_delta, out_prob);
  if (!rc && m->is_mc) ++m->mc_matches;  // (slamhip_matcher_mc_stream_info)
  if (!rc && m->is_bf) ++m->bf_matches;  // (slamhip_matcher_bf_stream_info)
  return rc;
}

static int process_scan_body(slamhip_matcher *m, int map_id, const double init_pose[3], double out_delta[3],
                             double *out_prob) {
  slamhip_ctx *ctx = m->ctx;
  SLAMHIP_CHECK(hipSetDevice(ctx->device));
#ifdef SLAMHIP_TESTING
  if (m->debug_fail_next > 0) {
    --m->debug_fail_next;
    set_error("injected failure (slamhip_matcher_debug_fail_next)");
    return SLAMHIP_ERR_HIP;
  }
#endif
  if (m->is_m3rsm) return m3rsm_process_scan(m, map_id, init_pose, out_delta, out_prob);
  // (r06) the GMapping OOPE's checked default mode: a chain that met a comparison its sums cannot settle reports it
  // before anything has been shown to an observer; the match is then redone below in the exact mode
  bool force_exact = false;
  if (chain_eligible(m)) {
    // (one co-resident launch where that is asked for and fits; else, or when it gives up, the chain of kernels)
    const int crc = chain_process_scan(m, map_id, init_pose, out_delta, out_prob, hc_resident_asked(m));
    if (crc == kChainUnsettled) force_exact = true;
    else if (crc != kChainNeedsHost) return crc;
  }
  {
    // (a raw scan whose block is still to be assembled, slamhip_matcher_process_raw_scan: everything below reads it)
    const int arc = scan_assemble_now(ctx);
    if (arc) return arc;
  }
  if (!force_exact && mc_chain_eligible(m)) {
    const int crc = mc_chain_process_scan(m, map_id, init_pose, out_delta, out_prob);
    if (crc != kChainNeedsHost) return crc;
  }
  if (!force_exact && !m->bf.skip_device && bf_device_eligible(m)) {
    const int crc = bf_device_process_scan(m, map_id, init_pose, out_delta, out_prob);
    if (crc != kChainNeedsHost) return crc;
  }
  // The GMapping OOPE in its exact mode (beam-order sum and / or the raw provider's per-beam trig: exact_kernels.hip) keeps
  // the reference's ONE cache object on the device and applies it pose after pose in CALL order -- so the poses have to be
  // scored in call order: one certain candidate per batch, no speculation, no replayed side outputs (the job runs as a
  // plain one; ctx->gm_* is kept by the scoring call itself).  Slow by design: the mode results are checked against.
  const bool gm_cfg = m->cfg.oope == SLAMHIP_OOPE_GMAPPING;
  const bool gm_exact_cfg = gm_cfg && (m->cfg.sum_order == SLAMHIP_SUM_SEQUENTIAL || m->cfg.pose_trig == SLAMHIP_POSE_TRIG_RAW_EXACT);
  // ... and its CHECKED default mode on the host-driven batches: a comparison on the walked path whose two scores lie
  // within 2^-40 of each other (the canonical sum with the device's exp against the reference's beam-order sum with
  // glibc's) ends the speculative run -- the enumerator and the cache go back to where the match started and the match
  // is redone in the exact mode.  An observer's events of the speculative run are held back until it is known to stand
  // (the device chains report their trace at the end of a match as well), so a redone match shows it ONE trace: the exact one
  const bool gm_checked = gm_cfg && !gm_exact_cfg && tie_check_default(m);
  std::unique_ptr<PoseEnumerator> pe_at_start;
  if (gm_checked && !force_exact) pe_at_start = m->pe->clone();
  const GmCarry carry_at_start{ctx->gm_cx, ctx->gm_cy, ctx->gm_prob};
  struct BufferingObserver {  // holds a speculative run's events back until the run is known to stand
    const slamhip_observer *to;
    bool hold;
    struct Ev {
      int kind;
      double p[3], s;
    };
    std::vector<Ev> held;
    static void test(void *u, const double p[3], double s) {
      auto *o = static_cast<BufferingObserver *>(u);
      if (o->hold) o->held.push_back(Ev{0, {p[0], p[1], p[2]}, s});
      else if (o->to->on_scan_test) o->to->on_scan_test(o->to->user, p, s);
    }
    static void update(void *u, const double p[3], double s) {
      auto *o = static_cast<BufferingObserver *>(u);
      if (o->hold) o->held.push_back(Ev{1, {p[0], p[1], p[2]}, s});
      else if (o->to->on_pose_update) o->to->on_pose_update(o->to->user, p, s);
    }
    void flush() {
      for (const Ev &e : held) {
        if (e.kind == 0 && to->on_scan_test) to->on_scan_test(to->user, e.p, e.s);
        if (e.kind == 1 && to->on_pose_update) to->on_pose_update(to->user, e.p, e.s);
      }
      held.clear();
    }
  } buffering{&m->obs, false, {}};
  const slamhip_observer obs_wrap{&buffering, &BufferingObserver::test, &BufferingObserver::update, nullptr};
  m->chain_rescored = 0;
  m->tail_calls = 0;
  m->t_stage_us = m->t_score_us = 0;
  for (;;) {
    const bool gm_exact = gm_exact_cfg || force_exact;
    const bool gm = gm_cfg && !gm_exact;
    slamhip_spe_cfg run_cfg = m->cfg;
    if (force_exact) {
      // the redo decides the way the REFERENCE would: beam-order sums, glibc's exp, and the reference's trigonometry --
      // its default RawTrigonometryProvider (cos / sin(theta + a) per beam, restated) where the scan's angles are known
      // to the context (slamhip_scan_set_angles / slamhip_scan_filter_upload), else the cached provider's angle addition
      // with the host's sincos of the heading
      run_cfg.sum_order = SLAMHIP_SUM_SEQUENTIAL;
      run_cfg.pose_trig = scan_angles_known(ctx) ? SLAMHIP_POSE_TRIG_RAW_EXACT : SLAMHIP_POSE_TRIG_HOST;
    }
    const int budget = gm_exact ? 1 : (m->max_batch > 0 ? m->max_batch : 256);
    int rc = ensure_pose_capacity(ctx, budget + 2);  // + the initial pose, + the best pose of a batch scored twice
    if (rc) return rc;
    // the checked default mode of the host-driven batches (the device chain has its own, csrc/hc_chain.hip)
    (void)tie_check_default(m);
    const bool checked = m->tie_check == 1 && !gm_cfg && m->cfg.sum_order == SLAMHIP_SUM_TREE256 && ctx->low_latency &&
                         !ctx->stage_poses;
    GmCarry carry;
    carry.cx = ctx->gm_cx;
    carry.cy = ctx->gm_cy;
    carry.prob = ctx->gm_prob;
    MatchJob &job = m->job;
    buffering.hold = gm && gm_checked && pe_at_start != nullptr;
    job.start(m->pe.get(), Pose{init_pose[0], init_pose[1], init_pose[2]}, gm, m->has_obs ? &obs_wrap : nullptr,
              carry, m->p_accept0);
    bool redo = false;
    while (!job.done) {
      const int n = job.plan(budget, ctx->h_poses.get());
      if (n == 0) break;
      const double t0 = MatchJob::now_us();
      unsigned seq = 0;
      ctx->want_fprints = checked;
      rc = score_staged(ctx, map_id, &run_cfg, n, nullptr, 0, &seq);
      ctx->want_fprints = false;
      if (rc) return rc;
      m->pe->idle_work();  // outcome-independent host work while the batch is on the GPU (MC: polar pairs)
      rc = score_wait(ctx, seq);
      if (rc) return rc;
      m->t_score_us += MatchJob::now_us() - t0;
      if (gm && gm_checked && pe_at_start && job.gm_unsettled(ctx->h_scores.get(), ctx->h_gm_info.get(), ctx)) {
        redo = true;
        break;
      }
      if (checked && job.ambiguous(ctx->h_scores.get(), ctx->h_fprints.get())) {
        // a comparison the tree sums cannot settle: the same batch (and the pose that is the best so far) once more,
        // summed in the reference's beam order; those sums decide, the canonical sums stay what is reported
        m->keep_scores.assign(ctx->h_scores.get(), ctx->h_scores.get() + n);
        m->keep_fprints.assign(ctx->h_fprints.get(), ctx->h_fprints.get() + n);
        ctx->h_poses.get()[3 * n] = job.best.x;
        ctx->h_poses.get()[3 * n + 1] = job.best.y;
        ctx->h_poses.get()[3 * n + 2] = job.best.theta;
        slamhip_spe_cfg seq_cfg = m->cfg;
        seq_cfg.sum_order = SLAMHIP_SUM_SEQUENTIAL;
        rc = score_staged(ctx, map_id, &seq_cfg, n + 1, nullptr, 0, &seq);
        if (rc) return rc;
        rc = score_wait(ctx, seq);
        if (rc) return rc;
        ++m->chain_rescored;
        m->rescored_poses += n + 1;
        rc = job.consume(m->keep_scores.data(), ctx->h_gm_info.get(), ctx, m->keep_fprints.data(), ctx->h_scores.get(), ctx->h_scores.get()[n]);
      } else {
        rc = job.consume(ctx->h_scores.get(), ctx->h_gm_info.get(), ctx, checked ? ctx->h_fprints.get() : nullptr);
      }
      if (rc) return rc;
    }
    if (redo) {
      // back to the start of the match, in the exact mode; the observer has been shown nothing yet
      m->pe->assign(*pe_at_start);
      pe_at_start.reset();
      ctx->gm_cx = carry_at_start.cx;
      ctx->gm_cy = carry_at_start.cy;
      ctx->gm_prob = carry_at_start.prob;
      buffering.held.clear();
      force_exact = true;
      continue;
    }
    buffering.flush();
    if (force_exact) ++m->chain_rescored;  // (GMapping OOPE: matches redone in the exact mode)
    if (gm) {
      ctx->gm_cx = job.carry.cx;
      ctx->gm_cy = job.carry.cy;
      ctx->gm_prob = job.carry.prob;
    }
    job.delta(out_delta);
    *out_prob = job.best_prob;
    if (m->has_obs && m->obs.on_matching_end) m->obs.on_matching_end(m->obs.user, out_delta, job.best_prob);
    return SLAMHIP_OK;
  }
}

}  // extern "C"
