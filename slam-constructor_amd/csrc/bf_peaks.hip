// bf_peaks.hip -- the local maxima of K brute-force score landscapes (slamhip_matcher_bf_peaks and its batch form): the
// rule of bf_peaks.h in three launches behind the scoring launch, grid.y = job (the lone call is K = 1).
//
//   k_bf_peaks_plane    the in-plane half of the separable window maximum.  A workgroup takes a tile of one theta layer
//                       with its halo into LDS (TX + 2 rx by TY + 2 ry scores, absent outside the volume), runs the x
//                       pass over every row of it into a second LDS array of (score, x) pairs and the y pass over that,
//                       and stores the best key of every output's in-plane window.  Two instantiations: 32 x 8 outputs
//                       for rx, ry <= 8 (18 KB of LDS), 16 x 8 for radii up to 32 (59 KB).  It also folds the scores it
//                       loaded into the job's lattice maximum: one 64-bit atomic max per wave on an order-preserving
//                       key, which gives the same word in whatever order the waves arrive.
//   k_bf_peaks_theta    one thread per lattice point: the theta pass over 2 rt + 1 in-plane keys (rows of x: coalesced),
//                       "the box maximum's index is mine", the floors, and a wave-aggregated append of the survivors --
//                       one atomic add per wave -- into the job's slab of B records.
//   k_bf_peaks_order    one workgroup per job ranks the at most 8192 survivors by key (a rank is the number of
//                       survivors that beat a record: the key order is total, so ranks are a permutation) through LDS
//                       chunks of 2048 records, writes n_found, n_written and the first max_peaks records into pinned
//                       memory and clears the job's two scratch words for the next call.
// The survivors arrive in any order; the result's order comes from the ranks alone.  No kernel waits on another
// workgroup.  All arithmetic on scores is comparison, and the one multiplication of the floor (bf_peak_kept).
#include <hip/hip_runtime.h>

#include "bf_peaks_device.h"
#include "kernel_pick.h"

namespace slamhip {

namespace {

constexpr int kPlaneBlock = 256;
constexpr int kThetaBlock = 256;
constexpr int kOrderBlock = 1024;
constexpr int kOrderChunk = 2048;
constexpr int kOrderPerThread = (int)(kBfPeaksMaxSurvivors / kOrderBlock);

// an order-preserving 64-bit key of a non-NaN double; no score maps to 0
__device__ inline unsigned long long peaks_max_key(double s) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(s);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ inline double peaks_max_value(unsigned long long k) {
  const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  return __longlong_as_double((long long)b);
}

}  // namespace

template <int HALO, int TX, int TY>
__global__ __launch_bounds__(kPlaneBlock) void k_bf_peaks_plane(BfPeaksArgs a, int tiles_x, int tiles_y) {
  constexpr int MAXW = TX + 2 * HALO, MAXH = TY + 2 * HALO;
  __shared__ double s_in[MAXH][MAXW];
  __shared__ double s_xs[MAXH][TX];
  __shared__ int s_xi[MAXH][TX];
  const int t = threadIdx.x;
  const int job = blockIdx.y;
  const unsigned tile = blockIdx.x;
  const int tile_x = (int)(tile % (unsigned)tiles_x);
  const unsigned rest = tile / (unsigned)tiles_x;
  const int tile_y = (int)(rest % (unsigned)tiles_y);
  const int it = (int)(rest / (unsigned)tiles_y);
  if (it >= a.nt) return;  // (never: the grid is tiles_x tiles_y nt)
  const int rx = a.rx, ry = a.ry;
  const int x0 = tile_x * TX, y0 = tile_y * TY;
  const int W = TX + 2 * rx, H = TY + 2 * ry;
  const long long plane = (long long)a.nx * a.ny;
  const double *vol = a.volumes + (long long)job * a.job_stride + plane * it;
  const double absent = __longlong_as_double(0x7ff8000000000000ll);
  // ---- the tile and its halo; what lies outside the volume is absent
  unsigned long long my_max = 0;
  for (int e = t; e < W * H; e += kPlaneBlock) {
    const int r = e / W, c = e - r * W;
    const int gx = x0 - rx + c, gy = y0 - ry + r;
    double s = absent;
    if (gx >= 0 && gx < a.nx && gy >= 0 && gy < a.ny) s = vol[gx + (long long)a.nx * gy];
    s_in[r][c] = s;
    if (!bf_peak_isnan(s)) {
      const unsigned long long k = peaks_max_key(s);
      my_max = k > my_max ? k : my_max;
    }
  }
  // the lattice maximum: wave reduction, one atomic per wave that saw a score
  for (int d = 32; d >= 1; d >>= 1) {
    const unsigned long long o = __shfl_xor(my_max, d);
    my_max = o > my_max ? o : my_max;
  }
  if ((t & 63) == 0 && my_max != 0) atomicMax(a.job_max + job, my_max);
  __syncthreads();
  // ---- x pass over every row of the tile and its y halo
  for (int e = t; e < H * TX; e += kPlaneBlock) {
    const int r = e / TX, c = e - r * TX;
    BfPeakKey best{0.0, -1};
    for (int k = 0; k <= 2 * rx; ++k) {
      const double s = s_in[r][c + k];
      best = bf_peak_better(best, BfPeakKey{s, bf_peak_isnan(s) ? -1ll : (long long)(x0 - rx + c + k)});
    }
    s_xs[r][c] = best.score;
    s_xi[r][c] = (int)best.index;
  }
  __syncthreads();
  // ---- y pass: one output per thread
  const int c = t % TX, r = t / TX;
  const int ox = x0 + c, oy = y0 + r;
  if (r < TY && ox < a.nx && oy < a.ny) {
    BfPeakKey best{0.0, -1};
    for (int k = 0; k <= 2 * ry; ++k) {
      const int wx = s_xi[r + k][c];
      const int gy = y0 - ry + r + k;
      // (a present key lies inside the volume: the loads above made everything else absent)
      const long long idx = wx < 0 ? -1ll : wx + (long long)a.nx * gy + plane * it;
      best = bf_peak_better(best, BfPeakKey{s_xs[r + k][c], idx});
    }
    const long long o = (long long)job * plane * a.nt + plane * it + ox + (long long)a.nx * oy;
    a.plane_s[o] = best.score;
    a.plane_i[o] = (int)best.index;
  }
}

__global__ __launch_bounds__(kThetaBlock) void k_bf_peaks_theta(BfPeaksArgs a) {
  const int job = blockIdx.y;
  const long long plane = (long long)a.nx * a.ny;
  const long long n = plane * a.nt;
  const long long i = (long long)blockIdx.x * kThetaBlock + threadIdx.x;
  bool kept = false;
  double s = 0.0;
  if (i < n) {
    const int it = (int)(i / plane);
    const long long in_plane = i - plane * it;
    const int lo = it - a.rt < 0 ? 0 : it - a.rt, hi = it + a.rt > a.nt - 1 ? a.nt - 1 : it + a.rt;
    BfPeakKey best{0.0, -1};
    for (int jt = lo; jt <= hi; ++jt) {
      const long long o = (long long)job * n + plane * jt + in_plane;
      best = bf_peak_better(best, BfPeakKey{a.plane_s[o], (long long)a.plane_i[o]});
    }
    const unsigned long long mk = a.job_max[job];
    if (best.index == i && mk != 0) {
      s = a.volumes[(long long)job * a.job_stride + i];
      kept = bf_peak_kept(s, peaks_max_value(mk), a.min_ratio, a.min_score);
    }
  }
  // the survivors of a wave take consecutive records behind ONE atomic add
  const unsigned long long mask = __ballot(kept);
  if (mask == 0) return;  // (wave-uniform)
  const int lane = (int)(threadIdx.x & 63);
  const int leader = __ffsll((long long)mask) - 1;
  unsigned base = 0;
  if (lane == leader) base = atomicAdd(a.job_count + job, (unsigned)__popcll(mask));
  base = __shfl(base, leader);
  if (kept) {
    const long long slot = (long long)base + __popcll(mask & ((1ull << lane) - 1ull));
    if (slot < a.bound) a.survivors[(long long)job * a.bound + slot] = BfPeakKey{s, i};  // (the bound holds: bf_peaks.h)
  }
}

__global__ __launch_bounds__(kOrderBlock) void k_bf_peaks_order(BfPeaksArgs a) {
  __shared__ BfPeakKey s_rec[kOrderChunk];
  const int t = threadIdx.x;
  const int job = blockIdx.x;
  const long long found = a.job_count[job];
  const int c = (int)(found < a.bound ? found : a.bound);
  const BfPeakKey *surv = a.survivors + (long long)job * a.bound;
  BfPeakKey mine[kOrderPerThread];
  int rank[kOrderPerThread];
#pragma unroll
  for (int k = 0; k < kOrderPerThread; ++k) {
    const int q = t + k * kOrderBlock;
    mine[k] = q < c ? surv[q] : BfPeakKey{0.0, -1};
    rank[k] = 0;
  }
  for (int c0 = 0; c0 < c; c0 += kOrderChunk) {
    const int len = c - c0 < kOrderChunk ? c - c0 : kOrderChunk;
    __syncthreads();
    for (int e = t; e < len; e += kOrderBlock) s_rec[e] = surv[c0 + e];
    __syncthreads();
    for (int e = 0; e < len; ++e) {
      const BfPeakKey o = s_rec[e];
#pragma unroll
      for (int k = 0; k < kOrderPerThread; ++k)
        if (mine[k].index >= 0 && o.index != mine[k].index && bf_peak_beats(o.score, o.index, mine[k].score, mine[k].index)) ++rank[k];
    }
  }
#pragma unroll
  for (int k = 0; k < kOrderPerThread; ++k)
    if (mine[k].index >= 0 && rank[k] < a.max_peaks) a.out[(long long)job * a.max_peaks + rank[k]] = mine[k];
  __syncthreads();  // (every thread has read the job's count)
  if (t == 0) {
    a.out_hdr[job].n_found = c;
    a.out_hdr[job].n_written = c < a.max_peaks ? c : a.max_peaks;
    a.job_count[job] = 0;
    a.job_max[job] = 0;
  }
}

template <int HALO, int TX, int TY>
static hipError_t launch_plane(const BfPeaksArgs &a, hipStream_t stream) {
  const int tiles_x = (a.nx + TX - 1) / TX, tiles_y = (a.ny + TY - 1) / TY;
  const long long tiles = (long long)tiles_x * tiles_y * a.nt;
  if (tiles <= 0 || tiles > 0x7fffffffll) return hipErrorInvalidValue;
  return launch_kernel(k_bf_peaks_plane<HALO, TX, TY>, dim3((unsigned)tiles, (unsigned)a.n_jobs), dim3(kPlaneBlock), 0, stream, nullptr,
                       nullptr, a, tiles_x, tiles_y);
}

hipError_t launch_bf_peaks(const BfPeaksArgs &a, hipStream_t stream, long long *launched) {
  const int radius[3] = {a.rx, a.ry, a.rt};
  if (a.n_jobs <= 0 || a.n_jobs > 65535 || !bf_peaks_shape_ok(a.nx, a.ny, a.nt, radius)) return hipErrorInvalidValue;
  const long long n = (long long)a.nx * a.ny * a.nt;
  if (n > (1ll << 26) || a.bound != bf_peaks_bound(a.nx, a.ny, a.nt, radius) || a.bound > kBfPeaksMaxSurvivors) return hipErrorInvalidValue;
  if (a.max_peaks < 0 || a.max_peaks > kBfPeaksMaxSurvivors) return hipErrorInvalidValue;
  hipError_t e = (a.rx <= kBfPeaksSmallHalo && a.ry <= kBfPeaksSmallHalo)
                     ? launch_plane<kBfPeaksSmallHalo, kBfPeaksSmallTx, kBfPeaksSmallTy>(a, stream)
                     : launch_plane<kBfPeaksLargeHalo, kBfPeaksLargeTx, kBfPeaksLargeTy>(a, stream);
  if (e != hipSuccess) return e;
  ++*launched;
  e = launch_kernel(k_bf_peaks_theta, dim3((unsigned)((n + kThetaBlock - 1) / kThetaBlock), (unsigned)a.n_jobs), dim3(kThetaBlock), 0,
                    stream, nullptr, nullptr, a);
  if (e != hipSuccess) return e;
  ++*launched;
  e = launch_kernel(k_bf_peaks_order, dim3((unsigned)a.n_jobs), dim3(kOrderBlock), 0, stream, nullptr, nullptr, a);
  if (e == hipSuccess) ++*launched;
  return e;
}

}  // namespace slamhip
