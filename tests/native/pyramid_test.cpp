// tests/native/pyramid_test.cpp -- the level definition of the map pyramid (slam-constructor_amd/csrc/map_pyramid_device.h)
// on the host under -fsanitize=address,undefined: maps and levels whose buffers are EXACTLY width * height * stride
// doubles on the heap (a read or write one cell outside a window is a heap overflow the sanitizer reports), windows of
// every small shape and origin -- far off centre, external (0, 0) outside the window --, few distinct impacts (ties
// everywhere), cells bit-equal to the unknown payload.  Checked while it runs:
//   * the levels made one from the other (pyr::reduce_cell with the carried fine coordinates) equal, bit for bit, a
//     direct scan of every block of the fine map under the same order -- the result does not depend on the reduction;
//   * every fine cell falls into exactly one block of every level, and that block lies inside the planned window;
//   * the last level is 1 x 1 of infinite scale, the one before it at most 2 x 2, scales double;
//   * refreshing the cells pyr::level_window names after changing fine cells equals building anew.
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include
//       -I<repo>/include -I<repo>/slam-constructor_amd/csrc pyramid_test.cpp
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "map_pyramid_device.h"

using namespace slamhip;

static int fails = 0;
#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
      if (++fails > 20) std::exit(1);                         \
    }                                                         \
  } while (0)

struct HostLevel {
  double *payload;
  int *coord;
  int w, h, ox, oy;
  pyr::Level view() const { return pyr::Level{payload, coord, w, h, w, ox, oy}; }
};

template <int CD>
static void reduce_window(const pyr::Level &src, const pyr::Level &dst, bool top, int model, int oie, const double *unknown, int cx0,
                          int cy0, int cx1, int cy1) {
  const int bx = top ? 0 : src.origin_x - 2 * dst.origin_x, by = top ? 0 : src.origin_y - 2 * dst.origin_y;
  for (int iy = cy0; iy <= cy1; ++iy)
    for (int ix = cx0; ix <= cx1; ++ix) pyr::reduce_cell<CD>(src, dst, bx, by, model, oie, unknown, ix, iy);
}

template <int CD>
static long run_case(std::mt19937 &rng, int model, int oie, bool far = false) {
  std::uniform_int_distribution<int> dim(1, 41), off(-9, 50), val(0, 5), coin(0, 3);
  // far: the window stands 10^4 ... 2^21 cells from external (0, 0), in any quadrant, now and then exactly a power of two
  // out (the window then starts, or ends, on the border of the last finite level's block)
  std::uniform_int_distribution<int> far_off(10000, 1 << 21), pow2(14, 21);
  auto far_origin = [&]() {
    const int d = coin(rng) == 0 ? (1 << pow2(rng)) + coin(rng) - 1 : far_off(rng);
    return (rng() & 1) ? d : -d;
  };
  const int w = dim(rng), h = dim(rng), ox = far ? far_origin() : off(rng), oy = far ? far_origin() : off(rng);
  double unknown[4] = {0.5, 0, 0, 0};
  if (CD == 4) unknown[0] = 1.0, unknown[1] = unknown[2] = unknown[3] = 0.0;
  auto fill_cell = [&](double *p) {
    if (coin(rng) == 0) {
      for (int k = 0; k < CD; ++k) p[k] = unknown[k];
      return;
    }
    if (CD == 1) {
      // 0.75 and 1.25 have the same impact under the discrepancy OIE and different payloads
      static const double v[6] = {0.0, 0.25, 0.75, 1.25, 1.0, 0.625};
      p[0] = v[val(rng)];
    } else {
      const double o = 0.125 * val(rng), e = 0.125 * coin(rng);
      p[0] = 1.0 - o - e > 0 ? 1.0 - o - e : 0.0;
      p[1] = e;
      p[2] = o;
      p[3] = 0.0;
    }
  };
  double *fine = (double *)std::malloc(sizeof(double) * w * h * CD);
  for (int i = 0; i < w * h; ++i) fill_cell(fine + (size_t)i * CD);
  pyr::Plan pl;
  CHECK(pyr::plan_levels(w, h, ox, oy, 0.05, &pl));
  CHECK(pl.n >= 1 && pl.n < pyr::kMaxLevels);
  if (far) {
    // one level per doubling: ceil(log2(extent)) + 1, and the fine window's origin far outside every finite level
    long long extent = std::max(std::max((long long)ox, (long long)w - ox), std::max((long long)oy, (long long)h - oy));
    int want = 1;
    while ((1ll << (want - 1)) < extent) ++want;
    CHECK(pl.n == want && pl.n >= 15 && pl.n <= 23);
    CHECK(pl.origin_x[0] < 0 || pl.origin_x[0] >= pl.width[0]);
  }
  CHECK(pl.width[pl.n - 1] == 1 && pl.height[pl.n - 1] == 1 && std::isinf(pl.scale[pl.n - 1]));
  if (pl.n >= 2) CHECK(pl.width[pl.n - 2] <= 2 && pl.height[pl.n - 2] <= 2);
  else CHECK(w <= 2 && h <= 2);
  std::vector<HostLevel> lv(pl.n);
  for (int k = 0; k < pl.n; ++k) {
    lv[k] = HostLevel{(double *)std::malloc(sizeof(double) * pl.width[k] * pl.height[k] * CD),
                      (int *)std::malloc(sizeof(int) * 2 * pl.width[k] * pl.height[k]), pl.width[k], pl.height[k], pl.origin_x[k],
                      pl.origin_y[k]};
    if (k + 1 < pl.n) CHECK(pl.scale[k] == 0.05 * std::ldexp(1.0, k + 1));
  }
  const pyr::Level fine_view{fine, nullptr, w, h, w, ox, oy};
  auto build = [&](std::vector<HostLevel> &L, int x0, int y0, int ww, int hh) {
    for (int k = 1; k <= pl.n; ++k) {
      int cx0, cy0, cx1, cy1;
      pyr::level_window(pl, ox, oy, k, x0, y0, ww, hh, &cx0, &cy0, &cx1, &cy1);
      CHECK(cx0 >= 0 && cy0 >= 0 && cx1 < L[k - 1].w && cy1 < L[k - 1].h && cx0 <= cx1 && cy0 <= cy1);
      reduce_window<CD>(k == 1 ? fine_view : L[k - 2].view(), L[k - 1].view(), k == pl.n, model, oie, unknown, cx0, cy0, cx1, cy1);
    }
  };
  build(lv, 0, 0, w, h);
  // a direct scan of every block of the fine map
  auto check_direct = [&](const std::vector<HostLevel> &L) {
    for (int k = 1; k <= pl.n; ++k) {
      const HostLevel &l = L[k - 1];
      std::vector<int> hits((size_t)l.w * l.h, 0);
      for (int iy = 0; iy < l.h; ++iy)
        for (int ix = 0; ix < l.w; ++ix) {
          const double *best = nullptr;
          long long bk = 0;
          int bfx = 0, bfy = 0;
          for (int fy = 0; fy < h; ++fy)
            for (int fx = 0; fx < w; ++fx) {
              const int ex = fx - ox, ey = fy - oy;
              const bool in = k == pl.n ? true : (pyr::floor_shift(ex, k) == ix - l.ox && pyr::floor_shift(ey, k) == iy - l.oy);
              if (!in) continue;
              hits[(size_t)iy * l.w + ix]++;
              const double *p = fine + ((size_t)fy * w + fx) * CD;
              if (!pyr::known<CD>(p, unknown)) continue;
              const long long kk = pyr::key(pyr::impact(model, oie, p));
              if (!best || pyr::better(kk, ex, ey, bk, bfx, bfy)) best = p, bk = kk, bfx = ex, bfy = ey;
            }
          const double *got = l.payload + ((size_t)iy * l.w + ix) * CD;
          CHECK(std::memcmp(got, best ? best : unknown, sizeof(double) * CD) == 0);
          if (best) CHECK(l.coord[2 * ((size_t)iy * l.w + ix)] == bfx && l.coord[2 * ((size_t)iy * l.w + ix) + 1] == bfy);
        }
      long total = 0;
      for (int v : hits) total += v;
      CHECK(total == (long)w * h);  // every fine cell in exactly one block inside the window
      if (k < pl.n)
        for (int v : hits) CHECK(v > 0);  // a tight window: no column or row of blocks without a fine cell ... per cell
    }
  };
  check_direct(lv);
  // change a few cells, refresh their bounding window, compare with the direct scan again
  std::uniform_int_distribution<int> px(0, w - 1), py(0, h - 1);
  int x0 = w, y0 = h, x1 = -1, y1 = -1;
  for (int i = 0; i < 4; ++i) {
    const int x = px(rng), y = py(rng);
    fill_cell(fine + ((size_t)y * w + x) * CD);
    x0 = x < x0 ? x : x0, y0 = y < y0 ? y : y0, x1 = x > x1 ? x : x1, y1 = y > y1 ? y : y1;
  }
  build(lv, x0, y0, x1 - x0 + 1, y1 - y0 + 1);
  check_direct(lv);
  for (auto &l : lv) std::free(l.payload), std::free(l.coord);
  std::free(fine);
  return (long)w * h;
}

int main() {
  std::mt19937 rng(20261018u);
  long cells = 0;
  for (int i = 0; i < 300; ++i) {
    cells += run_case<1>(rng, SLAMHIP_CELL_OCC, SLAMHIP_OIE_DISCREPANCY);
    cells += run_case<1>(rng, SLAMHIP_CELL_OCC, SLAMHIP_OIE_OCCUPANCY);
    cells += run_case<4>(rng, SLAMHIP_CELL_TBM, SLAMHIP_OIE_DISCREPANCY);
    cells += run_case<4>(rng, SLAMHIP_CELL_CREDIBILIST, SLAMHIP_OIE_DISCREPANCY);
  }
  for (int i = 0; i < 100; ++i) {  // the same checks, window origins out to +-2^21 cells
    cells += run_case<1>(rng, SLAMHIP_CELL_OCC, SLAMHIP_OIE_DISCREPANCY, true);
    cells += run_case<1>(rng, SLAMHIP_CELL_OCC, SLAMHIP_OIE_OCCUPANCY, true);
    cells += run_case<4>(rng, SLAMHIP_CELL_TBM, SLAMHIP_OIE_DISCREPANCY, true);
    cells += run_case<4>(rng, SLAMHIP_CELL_CREDIBILIST, SLAMHIP_OIE_DISCREPANCY, true);
  }
  // the order of impacts: numbers, -0 below +0
  CHECK(pyr::key(-0.0) < pyr::key(0.0) && pyr::key(-1.0) < pyr::key(-0.5) && pyr::key(0.5) < pyr::key(1.0) &&
        pyr::key(-1e-300) < pyr::key(0.0));
  CHECK(!pyr::check_oie(SLAMHIP_CELL_TBM, SLAMHIP_OIE_OCCUPANCY) && pyr::check_oie(SLAMHIP_CELL_OCC, SLAMHIP_OIE_OCCUPANCY));
  pyr::Plan pl;
  CHECK(!pyr::plan_levels(0, 3, 0, 0, 1.0, &pl) && !pyr::plan_levels(4, 4, (1 << 30) + 1, 0, 1.0, &pl) && !pyr::plan_levels(4, 4, -(1 << 30), 0, 1.0, &pl));
  if (fails) return 1;
  std::printf("ok %ld cells in 1600 maps (400 of them 10^4 ... 2^21 cells from the origin)\n", cells);
  return 0;
}
