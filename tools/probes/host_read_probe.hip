// tools/probes/host_read_probe.hip -- what does it cost when EVERY workgroup of a chain-sized launch (253 x 1024) reads
// the same 1080 doubles with plain global loads, from (a) a pinned mapped host block written by the host just before the
// launch (hipHostMallocMapped, as the scan's staging block is allocated) or (b) HBM?  The question behind folding the
// raw scan's assembly into the chain kernel's prologue: are the host reads of the workgroups of one XCD shared in its
// L2 (about 8 x 8.6 KB over PCIe) or does each workgroup fetch for itself (253 x 8.6 KB)?
//   span      : HIP events attached to the dispatch (hipExtLaunchKernelGGL), us
//   load2use  : per workgroup, wall_clock64 (100 MHz) from before the load to after the workgroup's barrier behind the
//               first use of every loaded value, us: median / max over the workgroups, then median over the launches
// 50 launches per source, new contents before each; every workgroup checks the values it read (a stale value counts).
// Build: hipcc -O3 --offload-arch=gfx950 -o host_read_probe tools/probes/host_read_probe.hip
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <vector>

#define CK(x)                                                                      \
  do {                                                                             \
    hipError_t e = (x);                                                            \
    if (e != hipSuccess) {                                                         \
      printf("%s -> %s\n", #x, hipGetErrorString(e));                              \
      return 1;                                                                    \
    }                                                                              \
  } while (0)

constexpr int kBeams = 1080, kWgs = 253, kThreads = 1024, kReps = 50;

// value of element i in launch `gen`: exact in a double, different in every launch
__host__ __device__ inline double probe_value(int i, unsigned gen) { return (double)(gen * 4096u + (unsigned)i); }

__global__ __launch_bounds__(1024) void k_read(const double *__restrict__ src, int n, unsigned gen,
                                               unsigned *__restrict__ ticks, unsigned *__restrict__ bad) {
  __shared__ unsigned s_bad;
  const int t = threadIdx.x;
  if (t == 0) s_bad = 0;
  __syncthreads();
  const unsigned long long t0 = wall_clock64();
  double v = 0.0, v2 = 0.0;
  if (t < n) v = src[t];
  if (t + 1024 < n) v2 = src[t + 1024];  // the surplus beams of 1080 on 1024 threads
  unsigned wrong = 0;
  if (t < n && v != probe_value(t, gen)) wrong = 1;
  if (t + 1024 < n && v2 != probe_value(t + 1024, gen)) wrong += 1;
  if (wrong) atomicAdd(&s_bad, wrong);
  __syncthreads();
  const unsigned long long t1 = wall_clock64();
  if (t == 0) {
    ticks[blockIdx.x] = (unsigned)(t1 - t0);
    if (s_bad) atomicAdd(bad, s_bad);
  }
}

static float med(std::vector<float> v) {
  std::sort(v.begin(), v.end());
  return v[v.size() / 2];
}

int main() {
  hipStream_t st;
  CK(hipStreamCreate(&st));
  double *h_block = nullptr, *d_block = nullptr;
  CK(hipHostMalloc(&h_block, sizeof(double) * 5 * 2048, hipHostMallocMapped));
  CK(hipMalloc(&d_block, sizeof(double) * 5 * 2048));
  unsigned *d_ticks = nullptr, *d_bad = nullptr;
  CK(hipMalloc(&d_ticks, sizeof(unsigned) * 4096));
  CK(hipMalloc(&d_bad, sizeof(unsigned)));
  CK(hipMemset(d_bad, 0, sizeof(unsigned)));
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  std::vector<double> fresh(kBeams);
  std::vector<unsigned> ticks(4096);
  unsigned gen = 0;
  for (int wgs : {1, 8, 32, kWgs}) {
    for (int src = 0; src < 2; ++src) {
      std::vector<float> span, l2u_med, l2u_max;
      for (int r = 0; r < kReps + 3; ++r) {
        ++gen;
        for (int i = 0; i < kBeams; ++i) fresh[i] = probe_value(i, gen);
        if (src == 0) {
          std::copy(fresh.begin(), fresh.end(), h_block);  // the host writes the pinned block, the launch follows
        } else {
          CK(hipMemcpyAsync(d_block, fresh.data(), sizeof(double) * kBeams, hipMemcpyHostToDevice, st));
          CK(hipStreamSynchronize(st));
        }
        hipExtLaunchKernelGGL(k_read, dim3(wgs), dim3(kThreads), 0, st, e0, e1, 0,
                              (const double *)(src == 0 ? h_block : d_block), kBeams, gen, d_ticks, d_bad);
        CK(hipGetLastError());
        CK(hipEventSynchronize(e1));
        float ms = 0;
        CK(hipEventElapsedTime(&ms, e0, e1));
        CK(hipMemcpy(ticks.data(), d_ticks, sizeof(unsigned) * wgs, hipMemcpyDeviceToHost));
        if (r < 3) continue;  // warm-up
        std::vector<float> t(wgs);
        for (int k = 0; k < wgs; ++k) t[k] = ticks[k] / 100.0f;
        std::sort(t.begin(), t.end());
        span.push_back(ms * 1e3f);
        l2u_med.push_back(t[wgs / 2]);
        l2u_max.push_back(t[wgs - 1]);
      }
      unsigned bad = 0;
      CK(hipMemcpy(&bad, d_bad, sizeof(unsigned), hipMemcpyDeviceToHost));
      printf("%4d wgs x %d, %s: span %7.2f us (max %7.2f) | load-to-use median wg %6.2f us, slowest wg %6.2f us (max %6.2f) | wrong values %u\n",
             wgs, kThreads, src == 0 ? "pinned host" : "HBM        ", med(span),
             *std::max_element(span.begin(), span.end()), med(l2u_med), med(l2u_max),
             *std::max_element(l2u_max.begin(), l2u_max.end()), bad);
      if (bad) return 2;
    }
  }
  return 0;
}
