// scan_filter_test.cpp -- csrc/scan_filter.cpp (keep-mask pass + compaction pass, baseline and AVX2 clones) against
// the ONE-loop filter it replaced, which is kept here verbatim as the yardstick: the kept list, its length, the staged
// range / factor / weight rows and the total weight, compared with memcmp.  Random scans (argv[1] of them, default
// 24 000: n 1..1200, both trig modes, bounded 0 / 1, skip_rate 0 / 1 / 3, with and without is_occ / factor, ranges
// salted with NaN, +-inf, 0, negatives and 1e300, max_range 0 and negative among the usable ones) and swept ones: end
// points exactly on the map's first and last cell edges and a few ulps either side, nothing kept, everything kept.
// Prints "ok ..." or the first mismatch (exit status 1).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "scan_filter.h"

namespace {

struct MapGeom {
  double scale;
  int origin_x, origin_y, width, height;
};

struct Scan {
  int n = 0;
  std::vector<double> range, angle, cos_a, sin_a, factor, viny_f;
  std::vector<int> is_occ;
  bool has_occ = false, has_factor = false;
  bool trig_cached = true;
  int bounded = 1;
  unsigned skip_rate = 0;
  double max_range = 0;
  double pose[3] = {0, 0, 0};
  MapGeom map{0.1, 0, 0, 1, 1};
};

struct Rows {
  std::vector<int> kept;
  std::vector<double> r, f, w;
  double tot_w = 0;
};

// ---- the yardstick: the filter loop of scan_filter_stage as it was (csrc/slamhip_api.cpp), statement for statement
// (its int conversion of a NaN / an infinite / a huge quotient is what the hardware makes of it: not for the sanitizer)
__attribute__((no_sanitize("undefined"))) void yardstick(const Scan &sc, Rows *out) {
  const int n = sc.n;
  const double *range = sc.range.data(), *angle = sc.angle.data(), *pose = sc.pose;
  const int *is_occ = sc.has_occ ? sc.is_occ.data() : nullptr;
  const unsigned skip_rate = sc.skip_rate;
  const double max_range = sc.max_range;
  const int bounded = sc.bounded;
  const bool trig_cached = sc.trig_cached;
  const MapGeom *m = &sc.map;
  const Scan &sp = sc;
  constexpr double eps = std::numeric_limits<double>::epsilon();
  std::vector<int> &kept = out->kept;
  kept.clear();
  const bool cut = 0.0 < max_range + eps;  // (a usable range is set at all)
  double sb = 0, cb = 1;
  if (bounded) ::sincos(pose[2], &sb, &cb);
  for (int i = 0; i < n; ++i) {
    if (skip_rate && (unsigned(i) % skip_rate)) continue;
    if (is_occ && !is_occ[i]) continue;
    const bool too_far = cut && (max_range < range[i] + eps);
    if (too_far) continue;
    if (bounded) {
      double c, s;
      if (trig_cached) {
        c = cb * sp.cos_a[i] - sb * sp.sin_a[i];
        s = sb * sp.cos_a[i] + cb * sp.sin_a[i];
      } else {
        ::sincos(pose[2] + angle[i], &s, &c);
      }
      const double wx = pose[0] + range[i] * c, wy = pose[1] + range[i] * s;
      const int ix = (int)std::floor(wx / m->scale) + m->origin_x, iy = (int)std::floor(wy / m->scale) + m->origin_y;
      if (!(0 <= ix && ix < m->width && 0 <= iy && iy < m->height)) continue;
    }
    kept.push_back(i);
  }
  const int k = (int)kept.size();
  out->r.assign(k, 0.0);
  out->f.assign(k, 0.0);
  out->w.assign(k, 0.0);
  for (int q = 0; q < k; ++q) out->r[q] = range[kept[q]];
  for (int q = 0; q < k; ++q) out->w[q] = sc.viny_f[kept[q]] * std::sqrt(out->r[q]);
  if (sc.has_factor)
    for (int q = 0; q < k; ++q) out->f[q] = sc.factor[kept[q]];
  double tot_w = 0;
  for (int i = 0; i < k; ++i) tot_w += out->w[i];
  out->tot_w = tot_w;
}

void two_pass(const Scan &sc, int variant, Rows *out, int *mask_count) {
  slamhip::ScanFilterArgs a{};
  a.n = sc.n;
  a.range = sc.range.data();
  a.angle = sc.angle.data();
  a.is_occ = sc.has_occ ? sc.is_occ.data() : nullptr;
  a.skip_rate = sc.skip_rate;
  a.max_range = sc.max_range;
  a.bounded = sc.bounded;
  a.trig_raw = sc.trig_cached ? 0 : 1;
  a.cos_a = sc.cos_a.data();
  a.sin_a = sc.sin_a.data();
  for (int q = 0; q < 3; ++q) a.pose[q] = sc.pose[q];
  a.scale = sc.map.scale;
  a.origin_x = sc.map.origin_x;
  a.origin_y = sc.map.origin_y;
  a.width = sc.map.width;
  a.height = sc.map.height;
  // (exactly-sized heap blocks: the address sanitizer sees a store one past the end)
  std::vector<unsigned char> mask(sc.n);
  std::vector<double> tmp(sc.bounded && a.trig_raw ? 2 * (size_t)sc.n : 0);
  *mask_count = slamhip::scan_filter_mask(a, mask.data(), tmp.data(), variant);
  std::vector<int> kept(sc.n);
  const int k = slamhip::scan_filter_compact(mask.data(), sc.n, kept.data());
  out->kept.assign(kept.begin(), kept.begin() + k);
  out->r.assign(k, 0.0);
  out->f.assign(k, 0.0);
  out->w.assign(k, 0.0);
  out->tot_w = slamhip::scan_filter_fill(k, out->kept.data(), sc.range.data(), sc.has_factor ? sc.factor.data() : nullptr,
                                         sc.viny_f.data(), out->r.data(), sc.has_factor ? out->f.data() : nullptr,
                                         out->w.data(), variant);
}

// the total weight: the same bits -- unless both are NaN (a kept range that is NaN or negative makes its weight one):
// the NaN a sum of several NaNs carries on is that of whichever operand the compiler put first in the addition, which
// the source does not say
bool same_total(double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0 || (std::isnan(a) && std::isnan(b)); }

bool same_doubles(const std::vector<double> &a, const std::vector<double> &b) {
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), sizeof(double) * a.size()) == 0);
}

long long g_checked = 0, g_kept = 0, g_dropped = 0;
int g_all = 0, g_none = 0;

bool check(const Scan &sc, const char *what, long long id) {
  Rows want;
  yardstick(sc, &want);
  const int k = (int)want.kept.size();
  g_kept += k;
  g_dropped += sc.n - k;
  g_all += k == sc.n;
  g_none += k == 0;
  const int variants = slamhip::scan_filter_has_avx2() ? 2 : 1;
  for (int v = 0; v < variants; ++v) {
    Rows got;
    int count = -1;
    two_pass(sc, v, &got, &count);
    const bool ok_list = got.kept.size() == want.kept.size() &&
                         (k == 0 || std::memcmp(got.kept.data(), want.kept.data(), sizeof(int) * k) == 0);
    const bool ok = ok_list && count == k && same_doubles(got.r, want.r) && same_doubles(got.f, want.f) &&
                    same_doubles(got.w, want.w) && same_total(got.tot_w, want.tot_w);
    if (!ok) {
      int first = -1;
      for (size_t q = 0; q < std::min(got.kept.size(), want.kept.size()) && first < 0; ++q)
        if (got.kept[q] != want.kept[q]) first = (int)q;
      std::printf("mismatch: %s %lld, clone %d: n %d, kept %d (mask pass says %d) against %d, first differing entry %d; "
                  "bounded %d, cached trig %d, skip_rate %u, max_range %g, scale %.17g\n",
                  what, id, v, sc.n, (int)got.kept.size(), count, k, first, sc.bounded, (int)sc.trig_cached, sc.skip_rate,
                  sc.max_range, sc.map.scale);
      return false;
    }
    // the weights alone, as a scan with every point kept is staged (its ranges go by memcpy)
    std::vector<double> w2(k);
    const double tot2 = slamhip::scan_filter_fill(k, want.kept.data(), sc.range.data(), nullptr, sc.viny_f.data(), nullptr,
                                                  nullptr, w2.data(), v);
    if (!same_doubles(w2, want.w) || !same_total(tot2, want.tot_w)) {
      std::printf("mismatch: %s %lld, clone %d: the weight row alone\n", what, id, v);
      return false;
    }
  }
  ++g_checked;
  return true;
}

void set_trig(Scan *sc) {
  sc->cos_a.resize(sc->n);
  sc->sin_a.resize(sc->n);
  for (int i = 0; i < sc->n; ++i) {
    sc->cos_a[i] = std::cos(sc->angle[i]);
    sc->sin_a[i] = std::sin(sc->angle[i]);
  }
}

Scan random_scan(std::mt19937_64 &g, long long id) {
  auto u = [&](double lo, double hi) { return lo + (hi - lo) * std::generate_canonical<double, 53>(g); };
  auto pick = [&](int m) { return (int)(g() % (unsigned long long)m); };
  Scan sc;
  // (every width class of the vector loops and their tails: 1 .. 1200, the short ones more often)
  sc.n = pick(4) == 0 ? 1 + pick(40) : 1 + pick(1200);
  sc.trig_cached = (id & 1) == 0;
  sc.bounded = pick(5) != 0;
  const unsigned skips[3] = {0u, 1u, 3u};
  sc.skip_rate = skips[pick(3)];
  sc.has_occ = pick(2) == 0;
  sc.has_factor = pick(2) == 0;
  const double scales[4] = {0.1, 0.05, 0.25, u(0.01, 1.0)};
  sc.map.scale = scales[pick(4)];
  sc.map.width = 20 + pick(400);
  sc.map.height = 20 + pick(400);
  sc.map.origin_x = pick(8) == 0 ? -pick(50) : pick(sc.map.width + 20);
  sc.map.origin_y = pick(8) == 0 ? sc.map.height + pick(50) : pick(sc.map.height + 20);
  const double ext = sc.map.scale * std::max(sc.map.width, sc.map.height);
  sc.pose[0] = (u(0, 1) * sc.map.width - sc.map.origin_x) * sc.map.scale;
  sc.pose[1] = (u(0, 1) * sc.map.height - sc.map.origin_y) * sc.map.scale;
  sc.pose[2] = u(-4, 4);
  const int mr = pick(6);
  sc.max_range = mr == 0 ? 0.0 : mr == 1 ? -1.0 : mr == 2 ? -std::numeric_limits<double>::epsilon() : u(0.1, 1.2) * ext;
  const double reach = u(0.2, 1.5) * ext;
  const int salt = pick(3) == 0 ? 0 : 10 + pick(90);  // one point in `salt` is a special value
  sc.range.resize(sc.n);
  sc.angle.resize(sc.n);
  sc.viny_f.resize(sc.n);
  sc.factor.resize(sc.n);
  sc.is_occ.resize(sc.n);
  const double specials[8] = {std::numeric_limits<double>::quiet_NaN(),
                              std::numeric_limits<double>::infinity(),
                              -std::numeric_limits<double>::infinity(),
                              0.0,
                              -0.0,
                              -u(0, 1) * ext,
                              1e300,
                              -1e300};
  for (int i = 0; i < sc.n; ++i) {
    sc.range[i] = u(0, reach);
    if (salt && pick(salt) == 0) sc.range[i] = specials[pick(8)];
    sc.angle[i] = u(-3.2, 3.2);
    sc.viny_f[i] = u(1, 3);
    sc.factor[i] = u(0.5, 1.5);
    sc.is_occ[i] = pick(10) != 0;
  }
  set_trig(&sc);
  return sc;
}

// End points on the rims: beams along +x and +y from the origin (cosine / sine exactly 1 and 0), whose end point is
// the range itself -- at edge * scale for the first and the one-past-the-last cell edge, and up to 6 ulps either side
Scan edge_scan(double scale, int origin, int extent, int tail) {
  Scan sc;
  sc.trig_cached = true;
  sc.bounded = 1;
  sc.max_range = -1.0;
  sc.map = MapGeom{scale, origin, origin, extent, extent};
  const double edges[4] = {-(double)origin * scale, (double)(extent - origin) * scale, -(double)origin / (1.0 / scale),
                           (double)(extent - origin) / (1.0 / scale)};
  for (int axis = 0; axis < 2; ++axis)
    for (int e = 0; e < 4; ++e)
      for (int d = -6; d <= 6; ++d) {
        double v = edges[e];
        for (int s = 0; s < std::abs(d); ++s) v = std::nextafter(v, d < 0 ? -1e308 : 1e308);
        sc.range.push_back(v);
        sc.cos_a.push_back(axis == 0 ? 1.0 : 0.0);
        sc.sin_a.push_back(axis == 0 ? 0.0 : 1.0);
        sc.angle.push_back(axis == 0 ? 0.0 : 1.5707963267948966);
      }
  for (int i = 0; i < tail; ++i) {  // (so that the swept points fall on every lane of a vector and into its tail)
    sc.range.insert(sc.range.begin(), 0.0);
    sc.cos_a.insert(sc.cos_a.begin(), 1.0);
    sc.sin_a.insert(sc.sin_a.begin(), 0.0);
    sc.angle.insert(sc.angle.begin(), 0.0);
  }
  sc.n = (int)sc.range.size();
  sc.viny_f.assign(sc.n, 1.5);
  sc.factor.assign(sc.n, 1.0);
  sc.is_occ.assign(sc.n, 1);
  return sc;
}

}  // namespace

int main(int argc, char **argv) {
  const long long n_random = argc > 1 ? std::atoll(argv[1]) : 24000;
  std::mt19937_64 g(20261019);
  for (long long id = 0; id < n_random; ++id)
    if (!check(random_scan(g, id), "random scan", id)) return 1;
  // ---- the rims
  long long id = 0;
  std::mt19937_64 ge(7);
  for (int rep = 0; rep < 400; ++rep) {
    const double fixed[6] = {0.1, 0.05, 0.2, 0.3, 0.025, 1.0 / 3.0};
    const double scale = rep < 6 ? fixed[rep] : 0.01 + 0.99 * std::generate_canonical<double, 53>(ge);
    const int extent = 2 + (int)(ge() % 2000), origin = (int)(ge() % (unsigned)(extent + 1));
    if (!check(edge_scan(scale, origin, extent, rep % 9), "rim sweep", id++)) return 1;
  }
  // ---- nothing kept / everything kept, at every n around the vector widths
  for (int n = 1; n <= 70; ++n)
    for (int all = 0; all < 2; ++all)
      for (int cached = 0; cached < 2; ++cached) {
        Scan sc;
        sc.n = n;
        sc.trig_cached = cached != 0;
        sc.bounded = 1;
        sc.max_range = all ? 50.0 : 0.0;
        sc.map = MapGeom{0.1, 500, 500, 1000, 1000};
        sc.range.assign(n, 3.0);
        sc.angle.resize(n);
        for (int i = 0; i < n; ++i) sc.angle[i] = 0.01 * i;
        set_trig(&sc);
        sc.viny_f.assign(n, 2.0);
        sc.factor.assign(n, 1.0);
        sc.is_occ.assign(n, 1);
        sc.has_occ = (n & 1) != 0;
        if (!check(sc, all ? "everything kept" : "nothing kept", n)) return 1;
      }
  std::printf("ok %lld scans, %lld points kept, %lld dropped, %d scans kept whole, %d kept nothing, avx2 clone %s\n",
              g_checked, g_kept, g_dropped, g_all, g_none, slamhip::scan_filter_has_avx2() ? "run" : "not on this CPU");
  return 0;
}
