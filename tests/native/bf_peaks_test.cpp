// The peaks rule of csrc/bf_peaks.h on the host, as a stand-alone program (tests/test_bf_peaks_host.py builds it plainly
// and under -fsanitize=address,undefined): the separable form against the triple-loop form on volumes drawn from four
// numbers and NaN -- ties and plateaus everywhere --, floors that cut at exact equality, an all-NaN volume, and the bound B as an upper
// bound on every case.  (The cut at max_peaks is the entry point's: tests/test_bf_peaks_host.py holds it, through
// slamhip_bf_peaks_host, with max_peaks of 0, 1 and more than n_found.)
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "bf_peaks.h"

using namespace slamhip;

namespace {

int g_cases = 0;

#define REQUIRE(cond)                                                        \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);          \
      std::exit(1);                                                          \
    }                                                                        \
  } while (0)

std::uint64_t g_state = 0x9e3779b97f4a7c15ull;
unsigned next_u32() {  // (splitmix64: the same volumes on every host)
  g_state += 0x9e3779b97f4a7c15ull;
  std::uint64_t z = g_state;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return (unsigned)((z ^ (z >> 31)) >> 32);
}

bool same(const std::vector<BfPeakKey> &a, const std::vector<BfPeakKey> &b) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); ++i)
    if (a[i].index != b[i].index || std::memcmp(&a[i].score, &b[i].score, 8) != 0) return false;
  return true;
}

void check_case(const std::vector<double> &v, int nx, int ny, int nt, const int r[3], double min_ratio, double min_score) {
  ++g_cases;
  REQUIRE(bf_peaks_shape_ok(nx, ny, nt, r));
  std::vector<BfPeakKey> sep, brute;
  bf_peaks_separable(v.data(), nx, ny, nt, r, min_ratio, min_score, &sep);
  bf_peaks_brute(v.data(), nx, ny, nt, r, min_ratio, min_score, &brute);
  REQUIRE(same(sep, brute));
  REQUIRE((long long)sep.size() <= bf_peaks_bound(nx, ny, nt, r));
  for (size_t i = 0; i + 1 < sep.size(); ++i) {  // ordered, and no two inside each other's window
    REQUIRE(bf_peak_beats(sep[i].score, sep[i].index, sep[i + 1].score, sep[i + 1].index));
  }
  for (size_t i = 0; i < sep.size(); ++i)
    for (size_t j = i + 1; j < sep.size(); ++j) {
      const long long a = sep[i].index, b = sep[j].index;
      const long long dx = std::llabs(a % nx - b % nx), dy = std::llabs((a / nx) % ny - (b / nx) % ny),
                      dt = std::llabs(a / ((long long)nx * ny) - b / ((long long)nx * ny));
      REQUIRE(dx > r[0] || dy > r[1] || dt > r[2]);
    }
}

}  // namespace

int main() {
  const double nan = std::numeric_limits<double>::quiet_NaN();
  const double values[5] = {0.25, 0.5, 1.0, 2.0, nan};  // powers of two: ratio 0.5 keeps the floor's product exact
  const int shapes[4][3] = {{1, 1, 1}, {9, 7, 1}, {3, 683, 2}, {17, 5, 9}};
  const int radii[4][3] = {{0, 0, 0}, {1, 1, 1}, {3, 2, 1}, {32, 32, 32}};
  const double floors[4][2] = {{0.0, -std::numeric_limits<double>::infinity()}, {0.5, 0.0}, {1.0, 0.0}, {0.0, 1.0}};
  for (const auto &sh : shapes)
    for (int fill = 0; fill < 3; ++fill) {
      const int nx = sh[0], ny = sh[1], nt = sh[2];
      std::vector<double> v((size_t)nx * ny * nt);
      // fill 0: all five values alike; 1: mostly one value (plateaus) with few others; 2: NaN-heavy
      for (double &s : v) {
        const unsigned u = next_u32();
        s = fill == 0 ? values[u % 5] : (fill == 1 ? (u % 16 ? 1.0 : values[(u >> 8) % 5]) : (u % 3 ? nan : values[(u >> 8) % 4]));
      }
      for (const auto &r : radii)
        for (const auto &f : floors) check_case(v, nx, ny, nt, r, f[0], f[1]);
    }
  {  // floors at exact equality: 1.0 is exactly 0.5 x 2.0 and stays; below it everything goes
    const int r[3] = {0, 0, 0};
    const std::vector<double> v = {2.0, 1.0, 0.5, nan, 1.0};
    std::vector<BfPeakKey> k;
    bf_peaks_separable(v.data(), 5, 1, 1, r, 0.5, 0.0, &k);
    REQUIRE(k.size() == 3 && k[0].index == 0 && k[1].index == 1 && k[2].index == 4);
    bf_peaks_separable(v.data(), 5, 1, 1, r, 0.0, 1.0, &k);
    REQUIRE(k.size() == 3 && k[1].index == 1 && k[2].index == 4);
    bf_peaks_separable(v.data(), 5, 1, 1, r, 1.0, 0.0, &k);
    REQUIRE(k.size() == 1 && k[0].index == 0);
    const int r1[3] = {1, 0, 0};  // two equal neighbours: the lower index only
    const std::vector<double> w = {1.0, 1.0, 0.5, 1.0, 1.0};
    bf_peaks_separable(w.data(), 5, 1, 1, r1, 0.0, 0.0, &k);
    REQUIRE(k.size() == 2 && k[0].index == 0 && k[1].index == 3);
    ++g_cases;
  }
  {  // an all-NaN volume: nothing found, under every radius
    const std::vector<double> v(9 * 7 * 2, nan);
    for (const auto &r : radii) {
      std::vector<BfPeakKey> a, b;
      bf_peaks_separable(v.data(), 9, 7, 2, r, 0.0, -1.0, &a);
      bf_peaks_brute(v.data(), 9, 7, 2, r, 0.0, -1.0, &b);
      REQUIRE(a.empty() && b.empty());
      ++g_cases;
    }
  }
  {  // shapes and radii the rule refuses
    const int ok[3] = {1, 1, 1}, neg[3] = {0, -1, 0}, wide[3] = {33, 0, 0};
    REQUIRE(bf_peaks_shape_ok(2, 2, 2, ok) && !bf_peaks_shape_ok(2, 2, 2, neg) && !bf_peaks_shape_ok(2, 2, 2, wide));
    REQUIRE(!bf_peaks_shape_ok(0, 2, 2, ok) && !bf_peaks_shape_ok(2, 2, 0, ok));
    REQUIRE(bf_peaks_bound(9, 7, 5, ok) == 5 * 4 * 3);
    const int zero[3] = {0, 0, 0};
    REQUIRE(bf_peaks_bound(9, 7, 5, zero) == 9 * 7 * 5);
  }
  std::printf("%d cases\nok bf peaks\n", g_cases);
  return 0;
}
