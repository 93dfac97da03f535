// tests/native/scan_generate_test.cpp -- the scan generator's per-beam routine (slam-constructor_amd/csrc/
// scan_generate_device.h) on the host under -fsanitize=address,undefined: maps whose payload is EXACTLY width * height *
// stride doubles on the heap (a read one cell outside the window is a heap overflow the sanitizer reports), poses inside
// and outside the window, beams far longer than the window, beams through grid vertices (ties), end points a hair off grid
// corners (walks that go astray: Bresenham's list).  Checks while it runs: a hit's range is positive and at most
// max_dist plus a cell's diagonal, a status is 0 / 1 / 2, the two libm variants give the same STATUS on all but a few
// beams, the angle list has the length the loop gives.
// The WAVE FORM of csrc/scan_generate.hip on the host: wave_emulated() below runs the kernel's rounds with the functions
// the kernel calls (sg_wave_applies, sg_wave_classify, sg_wave_after_tie, sg_cell_occ, sg_test_cell), the 64 lanes one
// after the other, the ballots as loops.  Every beam it settles must equal sg_beam_sequential bit for bit, and it must
// settle most beams: a wave form that always fell back would pass every device-against-device comparison unseen.
// sincos_<FMA> against the RUNNING libm: the variant the probe names must equal ::sincos on every one of 2e6 arguments
// (skipped with a note where the libm is neither build).
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include
//       -I<repo>/include -I<repo>/slam-constructor_amd/csrc scan_generate_test.cpp
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "scan_generate_device.h"

using namespace slamhip;
using namespace slamhip::sg;

// k_scan_generate_wave's sg_beam_wave, lane after lane; false = not settled
static bool wave_emulated(const SgMap &m, const SgBeam &b, double thr, int *status_out, double *range_out) {
  const SgWalkLine L = sg_walk_line(b);
  const int steps_x = std::abs(b.ex - b.bx), steps_y = std::abs(b.ey - b.by);
  const unsigned cap = (unsigned)steps_x + (unsigned)steps_y + 1u;
  if (!sg_wave_applies(L, cap)) return false;
  SgPiece pc{0u, 0, 0, L.e0, L.q0};
  int ties = 0, status = SG_NONE;
  bool found = false;
  double range = 0.0;
  for (unsigned k0 = 0u;;) {
    int i[64], j[64], cls[64], first = 64;
    for (int lane = 0; lane < 64; ++lane) {
      cls[lane] = sg_wave_classify(L, pc, k0 + (unsigned)lane, cap, steps_x, steps_y, &i[lane], &j[lane]);
      if (cls[lane] != 0 && first == 64) first = lane;
    }
    const int fcls = first < 64 ? cls[first] : 0;
    if (fcls == 3 || fcls == 4) return false;
    for (int lane = 0; !found && lane < 64 && lane <= first; ++lane) {
      const int cx = b.bx + L.inc_x * i[lane], cy = b.by + L.inc_y * j[lane];
      if (sg_cell_occ(m, cx, cy) < thr) continue;
      double rg = 0.0;
      const int r = sg_test_cell(b, cx, cy, &rg);
      if (r == SG_TOUCH) continue;
      found = true;
      status = r;
      range = r == SG_HIT ? rg : 0.0;
    }
    if (first == 64) {
      k0 += 64u;
      continue;
    }
    if (fcls == 1) break;
    if (++ties > kSgMaxTies) return false;
    pc = sg_wave_after_tie(L, i[first], j[first], k0 + (unsigned)first, steps_x, steps_y);
    k0 = pc.k_base;
  }
  *status_out = status;
  *range_out = range;
  return true;
}

template <bool FMA>
static long sincos_mismatches(std::mt19937_64 &eng) {
  std::uniform_real_distribution<double> U(-8.0, 8.0);
  long bad = 0;
  void (*volatile p)(double, double *, double *) = ::sincos;
  for (long it = 0; it < 2000000; ++it) {
    double x = U(eng);
    if (it % 8 == 1) x *= 1e-3;
    if (it % 64 == 2) x *= 1e-9;
    if (it % 64 == 3) x *= 1e4;
    double s, c, s1, c1;
    p(x, &s, &c);
    libm_exact::sincos_<FMA>(x, &s1, &c1);
    bad += s != s1 || c != c1;
  }
  return bad;
}

int main() {
  std::mt19937_64 eng(20261018);
  // which build of sincos runs here (the probe of slamhip_scan_gen_libm_variant: either build equal on everything)
  const long bad_fma = sincos_mismatches<true>(eng), bad_plain = sincos_mismatches<false>(eng);
  if (bad_fma != 0 && bad_plain != 0)
    std::fprintf(stderr, "note: this libm's sincos is neither restated build (%ld / %ld mismatches): not checked\n", bad_fma, bad_plain);
  long long settled = 0, wave_bad = 0, long_beams = 0;
  std::uniform_real_distribution<double> U(0.0, 1.0);
  long long beams = 0, hits = 0, asserts = 0, invalid = 0, differ = 0;
  const double tiny[6] = {0.0, 1e-9, -1e-9, 3e-8, -1e-7, 1e-6};
  // calls 600 ...: the same maps and poses at the far stations of tests/placed_scenes.py (shifts in cells), where the
  // relative tolerance of every tie and intersection test is 10^3 ... 10^5 times as wide and sg_pose_ok refuses poses
  static const int station[6][2] = {{20011, 10007}, {-20011, 10007}, {-10007, -20011}, {10007, -20011}, {2097155, -2097157}, {-2097155, 1048577}};
  const int n_near = 600, n_far = 600;
  long long near_settled = 0, near_beams = 0, near_hits = 0, near_differ = 0, near_invalid = 0;
  for (int it = 0; it < n_near + n_far; ++it) {
    if (it == n_near) near_settled = settled, near_beams = beams, near_hits = hits, near_differ = differ, near_invalid = invalid;
    const int kx = it < n_near ? 0 : station[it % 6][0], ky = it < n_near ? 0 : station[it % 6][1];
    const int model = it % 4;
    const int stride = model == SLAMHIP_CELL_OCC ? 1 : (model == SLAMHIP_CELL_GMAPPING ? 3 : 4);
    const int w = 1 + (int)(U(eng) * 40), h = 1 + (int)(U(eng) * 30);
    const double scale = (it % 3 == 0) ? 0.05 : 0.1;
    std::vector<double> payload((size_t)w * h * stride);
    for (size_t c = 0; c < (size_t)w * h; ++c) {
      const bool occ = U(eng) < 0.1;
      double *p = payload.data() + c * stride;
      if (stride == 1) p[0] = occ ? 1.0 : U(eng) * 0.4;
      else if (stride == 3) p[0] = occ ? 0.9 : (U(eng) < 0.5 ? -1.0 : 0.1), p[1] = p[2] = 0.0;
      else p[0] = occ ? 0.0 : 1.0, p[1] = 0.0, p[2] = occ ? 1.0 : 0.0, p[3] = 0.0;
    }
    SgMap m;
    m.payload = payload.data();
    m.width = w;
    m.height = h;
    m.pitch = w;
    m.stride = stride;
    m.origin_x = (int)(U(eng) * w) - kx;
    m.origin_y = (int)(U(eng) * h) - ky;
    m.model = model;
    m.occ_kind = model == SLAMHIP_CELL_TBM ? it / 4 % 2 : 0;
    m.scale = scale;
    m.unknown_occ = model == SLAMHIP_CELL_GMAPPING ? -1.0 : 0.5;
    const double hs = M_PI * (0.25 + 0.75 * U(eng)), inc = hs / (4 + (int)(U(eng) * 20));
    std::vector<double> angles(64);
    const long long na = sg_angles(hs, inc, 64, angles.data());
    if (na < 1 || na > 64) return std::printf("FAIL angle list %lld\n", na), 1;
    angles.resize((size_t)na);
    const int np_ = 4;
    std::vector<double> poses(3 * np_);
    double max_dist = it % 5 == 0 ? 100.0 : 0.3 + U(eng) * 6.0;
    for (int p = 0; p < np_; ++p) {
      // cell centres (ties along the axes and diagonals), centres a hair aside, anywhere; some outside the window
      const int cx = (int)(U(eng) * (w + 8)) - 4 - m.origin_x, cy = (int)(U(eng) * (h + 8)) - 4 - m.origin_y;
      const int kind = (int)(U(eng) * 3);
      poses[3 * p] = (cx + (kind == 2 ? 0.05 + 0.9 * U(eng) : 0.5)) * scale + (kind == 1 ? tiny[(int)(U(eng) * 6)] : 0.0);
      poses[3 * p + 1] = (cy + (kind == 2 ? 0.05 + 0.9 * U(eng) : 0.5)) * scale + (kind == 1 ? tiny[(int)(U(eng) * 6)] : 0.0);
      poses[3 * p + 2] = kind == 2 ? (U(eng) - 0.5) * 7.0 : (U(eng) < 0.5 ? std::atan2(1.0, 1 + (int)(U(eng) * 3)) - angles[0] : -angles[0]);
    }
    if (it % 7 == 0) {
      // aim beam 0 of pose 0 at a point a hair off a grid corner
      const double tx = (kx + (int)(U(eng) * 60) - 30) * scale + tiny[1 + (int)(U(eng) * 5)];
      const double ty = (ky + (int)(U(eng) * 60) - 30) * scale + tiny[1 + (int)(U(eng) * 5)];
      max_dist = std::hypot(tx - poses[0], ty - poses[1]);
      poses[2] = std::atan2(ty - poses[1], tx - poses[0]) - angles[0];
    }
    if (sg_check_beams(scale, np_, poses.data(), (int)na, angles.data(), max_dist)) {
      ++invalid;
      continue;
    }
    const size_t nb = (size_t)np_ * (size_t)na;
    std::vector<double> r0(nb), r1(nb);
    std::vector<unsigned char> s0(nb), s1(nb);
    sg_generate_host<false>(m, np_, poses.data(), (int)na, angles.data(), max_dist, 0.6, r0.data(), s0.data());
    sg_generate_host<true>(m, np_, poses.data(), (int)na, angles.data(), max_dist, 0.6, r1.data(), s1.data());
    for (int p = 0; p < np_; ++p)
      for (int i = 0; i < (int)na; ++i) {
        const SgBeam bm = sg_beam_setup<false>(poses[3 * p], poses[3 * p + 1], poses[3 * p + 2], angles[i], max_dist, scale);
        int st = -1;
        double rg = -1.0;
        long_beams += !sg_wave_applies(sg_walk_line(bm), (unsigned)(std::abs(bm.ex - bm.bx) + std::abs(bm.ey - bm.by) + 1));
        if (!wave_emulated(m, bm, 0.6, &st, &rg)) continue;
        ++settled;
        const size_t at = (size_t)p * na + i;
        wave_bad += st != s0[at] || std::memcmp(&rg, &r0[at], sizeof rg) != 0;
      }
    for (size_t b = 0; b < nb; ++b) {
      ++beams;
      if (s0[b] > 2 || s1[b] > 2) return std::printf("FAIL status\n"), 1;
      hits += s0[b] == 1;
      asserts += s0[b] == 2;
      differ += s0[b] != s1[b];
      if (s0[b] == 1 && !(r0[b] >= 0.0 && r0[b] <= std::fabs(max_dist) + 2 * scale)) return std::printf("FAIL range %g\n", r0[b]), 1;
      if (s0[b] != 1 && r0[b] != 0.0) return std::printf("FAIL range of a beam without a hit\n"), 1;
    }
  }
  if (wave_bad) return std::printf("FAIL %lld beams the wave form settles differ from the sequential routine\n", wave_bad), 1;
  if (near_settled * 10 < near_beams * 8) return std::printf("FAIL the wave form settled %lld of %lld beams only\n", near_settled, near_beams), 1;
  if (near_beams < 10000 || near_hits < 1000 || near_differ * 100 > near_beams)
    return std::printf("FAIL coverage %lld %lld %lld\n", near_beams, near_hits, near_differ), 1;
  // ... and the same bars for the far block alone; out there the opening assertion must have refused some calls
  const long long far_settled = settled - near_settled, far_beams = beams - near_beams, far_hits = hits - near_hits;
  if (far_settled * 10 < far_beams * 8) return std::printf("FAIL far out the wave form settled %lld of %lld beams only\n", far_settled, far_beams), 1;
  if (far_beams < 10000 || far_hits < 1000 || (differ - near_differ) * 100 > far_beams || invalid - near_invalid <= near_invalid)
    return std::printf("FAIL far coverage %lld %lld %lld %lld\n", far_beams, far_hits, differ - near_differ, invalid - near_invalid), 1;
  std::printf("ok wave form settled %lld of %lld beams (%lld too long for it), all equal; sincos mismatches fma %ld plain %ld; ", settled,
              beams, long_beams, bad_fma, bad_plain);
  std::printf("%lld beams, %lld hits, %lld status 2, %lld calls invalid, %lld statuses differ between the libm variants; ", beams,
              hits, asserts, invalid, differ);
  std::printf("at the far stations: settled %lld of %lld beams, %lld hits, %lld of %d calls refused\n", far_settled, far_beams, far_hits,
              invalid - near_invalid, n_far);
  return 0;
}
