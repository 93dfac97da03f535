// map_render.hip -- a resident map as the bytes its consumers take (include/slamhip.h "map render").
//
// The reference's two map consumers walk the map cell by cell: OccupancyGridPublisher::on_map_update
// (src/ros/occupancy_grid_publisher.h:40-46) writes one int8 per cell, GridMapToPgmDumber::dump_map
// (src/utils/map_dumpers.h:78-87) one grey byte.  Both bytes are pure functions of the cell (slamhip_internal.h:
// cell_occupancy, render_occgrid, render_pgm), so the conversion runs where the map lives: read 8 (OCC) or 32 (TBM,
// CREDIBILIST; GMAPPING tiles: the 8 of prob_occ) bytes per cell from HBM, write 1, and copy 1 byte per cell to the host
// in one piece.  Bandwidth bound; no LDS, no atomics.
//
// Output layout: w * h bytes, row r of the output at r * w; OCCGRID rows go bottom-up (output row r = map row y0 + r),
// PGM rows top-down (output row r = map row y0 + h - 1 - r).  The output buffer is cut into PACKS of kPack bytes at
// multiples of kPack from its (256-byte aligned) start; a thread owns the part of one pack that lies in one row.  A
// pack wholly inside a row is assembled in a register and leaves as ONE 4- or 8-byte store; what is left of a pack at
// the ragged ends of a row (a row start that is no multiple of the pack, its last w % kPack bytes, a row shorter than a
// pack) leaves byte by byte -- two rows that share a pack write disjoint bytes of it.
#include <algorithm>
#include <cstdint>

#include "slamhip_internal.h"
#include "tile_pool.h"

namespace slamhip {
namespace {

constexpr int kRenderThreads = 256;
constexpr int kMaxGridY = 65535;

// bytes per thread: 8 one-double cells (64 bytes read) or 4 four-double cells (128 bytes read)
template <int CD>
struct RenderPack {
  static constexpr int n = CD == 1 ? 8 : 4;
};

template <int CD>
__device__ inline unsigned char render_cell(const double *c, int model, int occ_kind, int format) {
  if (CD == 1) return render_byte(format, cell_occupancy(model, occ_kind, c[0], 0.0, 0.0));
  const double2 a = reinterpret_cast<const double2 *>(c)[0], b = reinterpret_cast<const double2 *>(c)[1];
  return render_byte(format, cell_occupancy(model, occ_kind, a.x, a.y, b.x));
}

// the part [lo, hi) of pack `p` of the output that lies in the row starting at output byte `o` (w bytes long)
template <int P>
__device__ inline bool pack_span(size_t o, int w, size_t p, size_t *lo, size_t *hi) {
  *lo = p * P;
  *hi = *lo + P;
  if (*lo < o) *lo = o;
  if (*hi > o + (size_t)w) *hi = o + (size_t)w;
  return *lo < *hi;
}

// dense window [x0, x0 + w) x [y0, y0 + h) of a bound map (the caller has checked it against the map): cells of CD
// doubles at `pitch` cells per row
template <int CD>
__global__ __launch_bounds__(kRenderThreads) void k_render_dense(const double *__restrict__ payload, int pitch, int model,
                                                                 int occ_kind, int format, int x0, int y0, int w, int h,
                                                                 unsigned char *__restrict__ out) {
  constexpr int P = RenderPack<CD>::n;
  const size_t t = (size_t)blockIdx.x * kRenderThreads + threadIdx.x;
  for (int r = blockIdx.y; r < h; r += gridDim.y) {
    const int sy = format == SLAMHIP_RENDER_PGM ? y0 + (h - 1 - r) : y0 + r;
    const size_t o = (size_t)r * w;
    size_t lo, hi;
    if (!pack_span<P>(o, w, o / P + t, &lo, &hi)) continue;
    const double *src = payload + ((size_t)sy * pitch + (size_t)x0 + (lo - o)) * CD;
    if (hi - lo == (size_t)P) {
      if (CD == 1) {
        double v[P];
        if ((reinterpret_cast<uintptr_t>(src) & 15) == 0) {  // (the same answer for every whole pack of a row)
#pragma unroll
          for (int k = 0; k < P; k += 2) {
            const double2 d = *reinterpret_cast<const double2 *>(src + k);
            v[k] = d.x;
            v[k + 1] = d.y;
          }
        } else {
#pragma unroll
          for (int k = 0; k < P; ++k) v[k] = src[k];
        }
        unsigned q[2] = {0u, 0u};
#pragma unroll
        for (int k = 0; k < P; ++k)
          q[k >> 2] |= (unsigned)render_byte(format, cell_occupancy(model, occ_kind, v[k], 0.0, 0.0)) << (8 * (k & 3));
        *reinterpret_cast<uint2 *>(out + lo) = make_uint2(q[0], q[1]);
      } else {
        unsigned q = 0u;
#pragma unroll
        for (int k = 0; k < P; ++k) q |= (unsigned)render_cell<CD>(src + (size_t)k * CD, model, occ_kind, format) << (8 * k);
        *reinterpret_cast<unsigned *>(out + lo) = q;
      }
    } else {
      const int n = (int)(hi - lo);
      for (int k = 0; k < n; ++k) out[lo + k] = render_cell<CD>(src + (size_t)k * CD, model, occ_kind, format);
    }
  }
}

// one slot of a tile pool (tile_pool.h): window at VIRTUAL cell (vx0, vy0) = external + the pool's origin; `table` is
// the slot's tile table.  Only prob_occ (the first double of the 4-double cell) is read; cells outside the extent read u0.
constexpr int kTiledPack = 8;
__device__ inline unsigned char render_tiled_cell(const double *__restrict__ pool, const int *__restrict__ table, int tiles_x,
                                                  int tiles_y, long long vx, long long vy, int format, double u0) {
  double v = u0;
  if (vx >= 0 && vx < (long long)tiles_x * kTileSide && vy >= 0 && vy < (long long)tiles_y * kTileSide) {
    const int ix = (int)vx, iy = (int)vy;
    const int tile = table[(iy >> kTileShift) * tiles_x + (ix >> kTileShift)];
    v = pool[((size_t)tile * kTileCells + ((size_t)(iy & kTileMask) << kTileShift) + (ix & kTileMask)) * 4];
  }
  return render_byte(format, cell_occupancy(SLAMHIP_CELL_GMAPPING, 0, v, 0.0, 0.0));
}
__global__ __launch_bounds__(kRenderThreads) void k_render_tiled(const double *__restrict__ pool, const int *__restrict__ table,
                                                                 int tiles_x, int tiles_y, long long vx0, long long vy0, int w,
                                                                 int h, int format, double u0, unsigned char *__restrict__ out) {
  constexpr int P = kTiledPack;
  const size_t t = (size_t)blockIdx.x * kRenderThreads + threadIdx.x;
  for (int r = blockIdx.y; r < h; r += gridDim.y) {
    const long long vy = format == SLAMHIP_RENDER_PGM ? vy0 + (h - 1 - r) : vy0 + r;
    const size_t o = (size_t)r * w;
    size_t lo, hi;
    if (!pack_span<P>(o, w, o / P + t, &lo, &hi)) continue;
    const long long vx = vx0 + (long long)(lo - o);
    if (hi - lo == (size_t)P) {
      unsigned q[2] = {0u, 0u};
#pragma unroll
      for (int k = 0; k < P; ++k)
        q[k >> 2] |= (unsigned)render_tiled_cell(pool, table, tiles_x, tiles_y, vx + k, vy, format, u0) << (8 * (k & 3));
      *reinterpret_cast<uint2 *>(out + lo) = make_uint2(q[0], q[1]);
    } else {
      const int n = (int)(hi - lo);
      for (int k = 0; k < n; ++k) out[lo + k] = render_tiled_cell(pool, table, tiles_x, tiles_y, vx + k, vy, format, u0);
    }
  }
}

int render_invalid(const char *msg) {
  set_error(msg);
  return SLAMHIP_ERR_INVALID;
}

bool format_ok(int format) { return format == SLAMHIP_RENDER_OCCGRID || format == SLAMHIP_RENDER_PGM; }

// room for `bytes` in the context's render buffer (kept between calls; a larger request replaces it)
int render_reserve(slamhip_ctx *ctx, size_t bytes) {
  // (whole 64 KiB: the floor is the rounded size itself)
  return grow_block(ctx->stream, ctx->d_render, ctx->render_cap, bytes, (bytes + 65535) & ~(size_t)65535);
}

dim3 render_grid(int w, int h, int pack) {
  const int packs = w / pack + 2;  // a row of w bytes touches at most that many packs of the output
  return dim3((packs + kRenderThreads - 1) / kRenderThreads, std::min(h, kMaxGridY));
}

// the kernel has been queued (between the profiling pair e0, e1 if there is one): bytes to the caller, one wait
int render_fetch(slamhip_ctx *ctx, hipEvent_t e1, size_t bytes, void *out) {
  SLAMHIP_CHECK(hipGetLastError());
  if (e1) SLAMHIP_CHECK(hipEventRecord(e1, ctx->stream));
  SLAMHIP_CHECK(hipMemcpyAsync(out, ctx->d_render.get(), bytes, hipMemcpyDeviceToHost, ctx->stream));
  SLAMHIP_CHECK(hipStreamSynchronize(ctx->stream));
  return SLAMHIP_OK;
}

}  // namespace

int tile_pool_render(TilePool *tp, int slot, int format, int x0, int y0, int w, int h, void *out) {
  if (!tp || slot < 0 || slot >= tp->n_slots) return render_invalid("bad slot");
  if (!out) return render_invalid("null output");
  if (!format_ok(format)) return render_invalid("unknown render format");
  if (w <= 0 || h <= 0) return render_invalid("empty window");
  slamhip_ctx *ctx = tp->ctx;
  SLAMHIP_CHECK(hipSetDevice(ctx->device));
  const size_t bytes = (size_t)w * h;
  int rc = render_reserve(ctx, bytes);
  if (rc) return rc;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  rc = profile_event_pair(ctx, &e0, &e1);
  if (rc) return rc;
  if (e0) SLAMHIP_CHECK(hipEventRecord(e0, ctx->stream));
  hipLaunchKernelGGL(k_render_tiled, render_grid(w, h, kTiledPack), dim3(kRenderThreads), 0, ctx->stream, tp->d_pool,
                     tp->d_table() + (size_t)slot * tp->table_stride(), tp->tiles_x, tp->tiles_y,
                     (long long)x0 + tp->origin_x, (long long)y0 + tp->origin_y, w, h, format, tp->unknown[0], ctx->d_render.get());
  return render_fetch(ctx, e1, bytes, out);
}

}  // namespace slamhip

using namespace slamhip;

int slamhip_map_render(slamhip_ctx *ctx, int map_id, int format, int occ_kind, int x0, int y0, int w, int h, void *out) {
  if (!ctx || map_id < 0 || map_id >= (int)ctx->maps.size() || !ctx->maps[map_id].bound) return render_invalid("unknown map id");
  const DeviceMap &m = ctx->maps[map_id];
  if (!out) return render_invalid("null output");
  if (!format_ok(format)) return render_invalid("unknown render format");
  if (!occ_kind_ok(m.cell_model, occ_kind))
    return render_invalid("occ_kind names a TBM cell class: 0 or 1 on a TBM map, 0 on every other");
  if (w <= 0 || h <= 0 || x0 < 0 || y0 < 0 || (long long)x0 + w > m.width || (long long)y0 + h > m.height)
    return render_invalid("window outside the bound map");
  SLAMHIP_CHECK(hipSetDevice(ctx->device));
  const size_t bytes = (size_t)w * h;
  int rc = render_reserve(ctx, bytes);
  if (rc) return rc;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  rc = profile_event_pair(ctx, &e0, &e1);
  if (rc) return rc;
  if (e0) SLAMHIP_CHECK(hipEventRecord(e0, ctx->stream));
  if (cell_doubles(m.cell_model) == 1)
    hipLaunchKernelGGL(k_render_dense<1>, render_grid(w, h, RenderPack<1>::n), dim3(kRenderThreads), 0, ctx->stream, m.d_payload,
                       m.pitch, m.cell_model, occ_kind, format, x0, y0, w, h, ctx->d_render.get());
  else
    hipLaunchKernelGGL(k_render_dense<4>, render_grid(w, h, RenderPack<4>::n), dim3(kRenderThreads), 0, ctx->stream, m.d_payload,
                       m.pitch, m.cell_model, occ_kind, format, x0, y0, w, h, ctx->d_render.get());
  return render_fetch(ctx, e1, bytes, out);
}

int slamhip_render_cells(int cell_model, int occ_kind, int format, int n, const double *payload, void *out) {
  if (cell_model < SLAMHIP_CELL_OCC || cell_model > SLAMHIP_CELL_CREDIBILIST) return render_invalid("unknown cell model");
  if (!format_ok(format)) return render_invalid("unknown render format");
  if (!occ_kind_ok(cell_model, occ_kind))
    return render_invalid("occ_kind names a TBM cell class: 0 or 1 for TBM cells, 0 for every other model");
  if (n < 0 || (n > 0 && (!payload || !out))) return render_invalid("bad arguments");
  const int sh = cell_stride_host(cell_model);
  unsigned char *o = static_cast<unsigned char *>(out);
  for (int i = 0; i < n; ++i) {
    const double *c = payload + (size_t)i * sh;
    o[i] = render_byte(format, cell_occupancy(cell_model, occ_kind, c[0], sh > 1 ? c[1] : 0.0, sh > 2 ? c[2] : 0.0));
  }
  return SLAMHIP_OK;
}
