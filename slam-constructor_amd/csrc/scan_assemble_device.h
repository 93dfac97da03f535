// scan_assemble_device.h -- one point of the scan block from the RAW scan's staged arrays and the resident per-beam
// tables (ScanAssembleArgs, slamhip_internal.h).  The ONE statement of that arithmetic (scan_point_of): k_scan_assemble
// (score_kernels.hip) writes its five values to the scan block, the lone co-resident hill-climbing chain
// (hc_resident.hip, RAW) keeps them in registers / LDS -- the same operations on the same operands, the same bits.
// Two ways of getting the operands: scan_assemble_point loads and computes in one go; scan_assemble_issue /
// scan_assemble_wait / scan_assemble_finish keep the staged loads -- a PCIe round trip -- in flight across whatever the
// caller puts between the first and the second.
#pragma once

#include <hip/hip_runtime.h>

#include "slamhip_internal.h"

namespace slamhip {

struct ScanPoint {
  double range, cos_a, sin_a, weight, factor;
};

// the arithmetic.  weighting 0: the host's 1.0 / k; 1: the host's own product, operand for operand (f64 sqrt is
// correctly rounded on both sides, the one multiplication has nothing to contract with); 2: made on the host
// (viny: the table's factor of the point's beam -- read only where there is a table and no host weight; h_weight,
// h_factor: the host's values, read only where there are any)
__device__ __forceinline__ ScanPoint scan_point_of(const ScanAssembleArgs &a, double range, double cos_a, double sin_a,
                                                   double viny, double h_weight, double h_factor) {
  ScanPoint p;
  p.range = range;
  p.cos_a = cos_a;
  p.sin_a = sin_a;
  p.weight = a.h_weight ? h_weight : (a.tab_viny ? viny * sqrt(p.range) : a.w_even);
  p.factor = a.h_factor ? h_factor : 1.0;
  return p;
}

// point q < a.n of the scan
__device__ __forceinline__ ScanPoint scan_assemble_point(const ScanAssembleArgs &a, int q) {
  const double range = a.h_range[q];
  const int i = a.h_kept ? a.h_kept[q] : q;
  const double cos_a = a.tab_cos[i], sin_a = a.tab_sin[i];
  const double h_weight = a.h_weight ? a.h_weight[q] : 0.0;
  const double viny = !a.h_weight && a.tab_viny ? a.tab_viny[i] : 0.0;
  const double h_factor = a.h_factor ? a.h_factor[q] : 1.0;
  return scan_point_of(a, range, cos_a, sin_a, viny, h_weight, h_factor);
}

// ---- the same point with its loads in flight.  The compiler's wait-count pass puts a vmcnt(0) behind the first
// staged load it sees as soon as a branch or a dependent load follows; these loads it does not see (inline asm), and
// the one wait is the caller's: scan_assemble_wait names every destination register as an in/out operand, so nothing
// reads one between its load and the wait.  Loads the compiler DOES see and that were issued earlier are waited for
// with counts that are at worst too strict (a wave's loads return in order); a load it sees and that is issued while
// these are in flight would wait for them too -- the caller keeps such loads out of the window.
struct ScanInFlight {
  double range, cos_a, sin_a;  // (cosine and sine: with no index row only)
  double wv;                   // the host's weight, or -- no index row, no host weight -- the table's viny factor
  double h_factor;
  int kept;                    // the index row's entry
};
__device__ __forceinline__ void staged_load(double &dst, const double *p) {
  asm volatile("global_load_dwordx2 %0, %1, off" : "+v"(dst) : "v"(p));
}
__device__ __forceinline__ void staged_load(int &dst, const int *p) {
  asm volatile("global_load_dword %0, %1, off" : "+v"(dst) : "v"(p));
}
// everything of point q < a.n that depends on no loaded value
__device__ __forceinline__ void scan_assemble_issue(const ScanAssembleArgs &a, int q, ScanInFlight &s) {
  s.range = s.cos_a = s.sin_a = s.wv = 0.0;
  s.h_factor = 1.0;
  s.kept = q;
  staged_load(s.range, a.h_range + q);
  if (a.h_kept) staged_load(s.kept, a.h_kept + q);
  if (a.h_weight) staged_load(s.wv, a.h_weight + q);
  if (a.h_factor) staged_load(s.h_factor, a.h_factor + q);
  if (!a.h_kept) {
    staged_load(s.cos_a, a.tab_cos + q);
    staged_load(s.sin_a, a.tab_sin + q);
    if (!a.h_weight && a.tab_viny) staged_load(s.wv, a.tab_viny + q);
  }
}
// the ONE wait of two points issued together
__device__ __forceinline__ void scan_assemble_wait(ScanInFlight &s, ScanInFlight &u) {
  asm volatile("s_waitcnt vmcnt(0)"
               : "+v"(s.range), "+v"(s.cos_a), "+v"(s.sin_a), "+v"(s.wv), "+v"(s.h_factor), "+v"(s.kept), "+v"(u.range),
                 "+v"(u.cos_a), "+v"(u.sin_a), "+v"(u.wv), "+v"(u.h_factor), "+v"(u.kept)
               :
               : "memory");
}
// behind the wait: two points' table entries where an index row says which (asked for together), and the arithmetic
__device__ __forceinline__ void scan_assemble_finish(const ScanAssembleArgs &a, const ScanInFlight &s,
                                                     const ScanInFlight &u, ScanPoint &ps, ScanPoint &pu) {
  double cs = s.cos_a, ss = s.sin_a, vs = s.wv, cu = u.cos_a, su = u.sin_a, vu = u.wv;
  if (a.h_kept) {
    cs = a.tab_cos[s.kept];
    cu = a.tab_cos[u.kept];
    ss = a.tab_sin[s.kept];
    su = a.tab_sin[u.kept];
    if (!a.h_weight && a.tab_viny) {
      vs = a.tab_viny[s.kept];
      vu = a.tab_viny[u.kept];
    }
    // (consumed HERE on every path: a table load whose value a caller uses on some lanes' path only stays pending in the
    // compiler's books, and its wait would land behind the NEXT points' issue, in front of their wait)
    asm volatile("" ::"v"(cs), "v"(ss), "v"(vs), "v"(cu), "v"(su), "v"(vu));
  }
  ps = scan_point_of(a, s.range, cs, ss, vs, s.wv, s.h_factor);
  pu = scan_point_of(a, u.range, cu, su, vu, u.wv, u.h_factor);
}

}  // namespace slamhip
