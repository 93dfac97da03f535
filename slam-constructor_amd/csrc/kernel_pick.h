// kernel_pick.h -- which template instantiation of a kernel family runs, said ONCE per family: the dispatchers every
// launcher (and every capacity query) picks its kernel through, the one launch, and the normalisation of a co-resident
// hill-climbing variant.  Host-only, and free of device code: tests/native/kernel_pick_test.cpp compiles it with a
// plain host compiler.
#pragma once

#include <hip/hip_runtime_api.h>

#include <type_traits>

#include "slamhip.h"

// (hip/hip_ext.h's declaration, repeated: that header's templates need the HIP compiler)
extern "C" hipError_t hipExtLaunchKernel(const void *function_address, dim3 numBlocks, dim3 dimBlocks, void **args,
                                         size_t sharedMemBytes, hipStream_t stream, hipEvent_t startEvent,
                                         hipEvent_t stopEvent, int flags);

namespace slamhip {

template <int V>
using int_c = std::integral_constant<int, V>;

// ---- run-time value -> compile-time constant.  `f` is a generic lambda that returns a kernel pointer.
// The 1-cell models.  Anything else (SLAMHIP_CELL_GMAPPING included) is "no kernel": null, never another model's.
template <class F>
auto pick_cell_model(int model, F &&f) -> decltype(f(int_c<SLAMHIP_CELL_OCC>{})) {
  switch (model) {
    case SLAMHIP_CELL_OCC: return f(int_c<SLAMHIP_CELL_OCC>{});
    case SLAMHIP_CELL_TBM: return f(int_c<SLAMHIP_CELL_TBM>{});
    case SLAMHIP_CELL_CREDIBILIST: return f(int_c<SLAMHIP_CELL_CREDIBILIST>{});
    default: return nullptr;
  }
}
// ... and the two whose cells are beliefs (the probability plane)
template <class F>
auto pick_belief_model(int model, F &&f) -> decltype(f(int_c<SLAMHIP_CELL_TBM>{})) {
  switch (model) {
    case SLAMHIP_CELL_TBM: return f(int_c<SLAMHIP_CELL_TBM>{});
    case SLAMHIP_CELL_CREDIBILIST: return f(int_c<SLAMHIP_CELL_CREDIBILIST>{});
    default: return nullptr;
  }
}
template <class F>
auto pick_bool(bool b, F &&f) -> decltype(f(std::false_type{})) {
  return b ? f(std::true_type{}) : f(std::false_type{});
}
// threads per workgroup.  Hill climbing: 256, 1024, anything else is 512; Monte Carlo: 512, anything else is 1024
constexpr int hc_nt_of(int nt) { return nt == 256 || nt == 1024 ? nt : 512; }
constexpr int mc_nt_of(int nt) { return nt == 512 ? 512 : 1024; }
template <class F>
auto pick_hc_nt(int nt, F &&f) -> decltype(f(int_c<512>{})) {
  switch (hc_nt_of(nt)) {
    case 256: return f(int_c<256>{});
    case 1024: return f(int_c<1024>{});
    default: return f(int_c<512>{});
  }
}
template <class F>
auto pick_mc_nt(int nt, F &&f) -> decltype(f(int_c<512>{})) {
  return mc_nt_of(nt) == 512 ? f(int_c<512>{}) : f(int_c<1024>{});
}

// poses per workgroup of the 1-cell scorers (k_score_point, k_bf_score_batch) for a launch of n_poses: enough workgroups
// to fill 256 CUs several times over, while amortising the per-workgroup beam-constant loads (40 B/beam) over several
// poses once there are plenty of poses.  Results do not depend on it.
inline int pick_poses_per_block(long long n_poses) {
  if (n_poses >= 8192) return 8;
  if (n_poses >= 2048) return 4;
  if (n_poses >= 1024) return 2;
  return 1;
}

// ---- the one launch.  Scoring and chain launches go through hipExtLaunchKernel when an event is given, so that
// slamhip_profile_* can attach its HIP events to the dispatch itself: the elapsed time is then the kernel's own
// begin..end (what rocprofv3 --kernel-trace reports), not record-to-record on an idle stream which adds ~4 us of
// queue processing per isolated launch (tools/event_probe.hip).  Without events the ordinary launch is used.
// A null kernel -- a dispatcher above found none -- is hipErrorInvalidValue.
template <class... P>
hipError_t launch_kernel(void (*kernel)(P...), dim3 grid, dim3 block, size_t lds_bytes, hipStream_t stream, hipEvent_t e0,
                         hipEvent_t e1, typename std::common_type<P>::type... args) {
  if (!kernel) return hipErrorInvalidValue;
  void *argv[] = {(void *)&args..., nullptr};
  if (e0 || e1) hipExtLaunchKernel((const void *)kernel, grid, block, argv, lds_bytes, stream, e0, e1, 0);
  else hipLaunchKernel((const void *)kernel, grid, block, argv, lds_bytes, stream);
  return hipGetLastError();
}

// ---- the co-resident hill-climbing chain (hc_resident.hip): which variants exist
// granules per sweeping lane for a grid of `grid` workgroups
constexpr int hc_gran_per_lane(int grid) { return grid <= 128 ? 2 : (grid <= 256 ? 4 : 7); }

// What a caller asks for.  `pair` only means something in a batch; `window`: a window OOPE in place of the 1-cell one.
struct HcResidentKey {
  int nt, max_inst;
  bool seq, batch, pair, window;
  bool raw = false;  // the workgroups assemble the raw scan's beams themselves (HcChainArgs::raw)
};
// ... and what is instantiated for it: workgroup size and sweep width; false: no such kernel.
//   window  256 / 512 / 1024 threads, lone chains of at most 256 workgroups in the default sum order, G = 4
//   pair    512 threads, G = 2 / 4 / 7
//   plain   256 / 512 / 1024 threads, the default or the beam-order sum or a batch, G = 2 / 4 / 7 -- but 385 workgroups
//           of 1024 threads are not resident together
//   raw     the plain form's lone chains in the default sum order, G = 4
inline bool hc_resident_variant(const HcResidentKey &k, int *nt, int *g) {
  const int slots = 6 * k.max_inst + 1;
  *nt = hc_nt_of(k.nt);
  *g = k.window ? 4 : hc_gran_per_lane(slots);
  if (k.seq && k.batch) return false;
  if (k.raw && (k.seq || k.batch || k.window || *g != 4)) return false;
  if (k.window) return !k.seq && !k.batch && slots <= 256;
  if (k.batch && k.pair) return k.nt == 512;
  return !(*nt == 1024 && *g == 7);
}

// ---- how many workgroups of a co-resident kernel the device keeps resident at once.
// The occupancy query of `kernel` (workgroups of `nt` threads with `lds_bytes` of dynamic LDS), the register-file rule
// of MI355X_MICROARCH.md ("Residency and cooperative launch": the API can be one block per CU high above 80 SGPRs; the
// 1-cell kernel's waves also need <= 128 VGPRs at 1024 threads) as the caller's two bounds -- `by_waves` workgroups per
// CU from the waves' VGPRs, `per_cu_cap` (0: none) from their SGPRs --, minus ONE CU's worth of workgroups of margin:
// a grid that needs every slot of the chip waits for any other kernel's last workgroup to leave.
inline hipError_t resident_capacity_of(const void *kernel, int nt, size_t lds_bytes, int by_waves, int per_cu_cap,
                                       int *out_wgs, int *out_per_cu) {
  if (!kernel) return hipErrorInvalidValue;
  int dev = 0, cus = 0, per_cu = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  if (e != hipSuccess) return e;
  e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, nt, lds_bytes);
  if (e != hipSuccess) return e;
  per_cu = per_cu < by_waves ? per_cu : by_waves;
  if (per_cu_cap > 0 && per_cu > per_cu_cap) per_cu = per_cu_cap;
  *out_wgs = per_cu * (cus - 1);
  if (out_per_cu) *out_per_cu = per_cu;
  return hipSuccess;
}

}  // namespace slamhip
