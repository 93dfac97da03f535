// oracle/ref_consumers_harness.cpp -- TEST INFRASTRUCTURE ONLY (built where the reference tree exists).
//
// The host adapters that had only ever been compiled, RUN next to the UNMODIFIED reference headers:
//   refc_scan_generator  HipLaserScanGenerator (laser_scan_2D, laser_scans_2D), HipResidentMapView::generate_scans and the
//                        view's operator[] under the reference's own LaserScanGenerator
//   refc_angles          HipLaserScanGenerator::angles() against the list read off the reference's loop
//   refc_observers       HipGridMapToPgmDumper (on_map_update, file_name, dump_map, both branches), hip_occupancy_grid (both
//                        branches), HipResidentMapView::render -- next to GridMapToPgmDumber and the publisher's cell loop
//   refc_spe             HipScanProbabilityEstimator (filter_scan, estimate_scan_probability) next to
//                        WeightedMeanPointProbabilitySPE
//   refc_raw_batch       hip_process_raw_scans / HipRawScanJob next to the owners' own process_scan and the reference's
//   refc_scene_stats, refc_spe / refc_raw_batch with with_hip = 0: the scenes on the reference alone (no device call):
//                        tests/test_adapter_scenes_reference.py
// The scenes are oracle/ref_adapter_scenes.h.  Every entry returns 0 when it ran (-1: no device) and fills counters and
// rows of doubles; the tests assert on them.  Access control is relaxed only to put hand-made beliefs into cells and to
// read the library matcher a HipGridScanMatcher owns.
// Output: oracle/_ref/libslamref_consumers.so (links slam-constructor_amd/libslamhip.so).
#include <algorithm>
#include <array>
#include <cassert>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <functional>
#include <iostream>
#include <iterator>
#include <limits>
#include <map>
#include <memory>
#include <queue>
#include <random>
#include <set>
#include <sstream>
#include <stdexcept>
#include <string>
#include <tuple>
#include <typeinfo>
#include <unordered_map>
#include <unordered_set>
#include <utility>
#include <vector>

#include <unistd.h>

#define private public
#define protected public
#include "utils/init_scan_matching.h"
#include "utils/init_occupancy_mapping.h"
#include "utils/map_dumpers.h"
#include "utils/data_generation/map_primitives.h"
#include "utils/data_generation/grid_map_patcher.h"
#include "utils/data_generation/laser_scan_generator.h"
#include "slams/credibilist/grid_cell.h"
#include "../test/core/mock_grid_cell.h"
#include "slamhip_init_scan_matching.h"
#include "slamhip_scan_generator.h"
#include "slamhip_map_observers.h"
#undef private
#undef protected

#include "ref_adapter_scenes.h"

namespace {

using namespace scn;

bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0; }

slamhip_ctx *make_ctx() {
  slamhip_ctx *ctx = nullptr;
  if (slamhip_ctx_create(0, &ctx) != SLAMHIP_OK) {
    std::cerr << "refc: " << slamhip_last_error() << std::endl;
    return nullptr;
  }
  return ctx;
}

// the map of a cell class: the hand-made cecum or a SLAM-built one (with its hand-made beliefs)
struct Scene {
  std::shared_ptr<UnboundedPlainGridMap> gt = make_cecum_map(), wider = make_wider_world();
  std::unique_ptr<SlamMap> slam;
  std::shared_ptr<UnboundedPlainGridMap> map;
  int cls;
  explicit Scene(int c, bool special = true) : cls{c} {
    if (c == MOCK) {
      map = gt;
    } else {
      slam = std::make_unique<SlamMap>(c);
      slam->build(*gt);
      if (special) put_special_host(c, *slam->map);
      map = slam->map;
    }
  }
  // one more scan into a built map (the reference's side); the scan and pose for the device's side
  void update(int k, LaserScan2D *scan_out = nullptr, RobotPose *pose_out = nullptr) {
    const RobotPose p = extra_pose(k);
    const LaserScan2D s = ref_scan(*wider, p, slam->lsp);
    slam->append(s, p, 0.9);
    if (scan_out) *scan_out = s;
    if (pose_out) *pose_out = p;
  }
};

// A device window that gets every scan of a built map through K6 (slamhip_map_append_scan_raw), from the empty 40 x 30
// window on: what a resident world's map is.  (A MeanProbabilityCell's update count is no part of its payload: a window
// UPLOADED from a host map cannot be updated further as the host map is.)
struct K6Map {
  slamhip_ctx *ctx;
  int id, cls;
  K6Map(slamhip_ctx *c, int map_id, int cell_class) : ctx{c}, id{map_id}, cls{cell_class} {
    double unk[4] = {0, 0, 0, 0};
    payload(cls, *prototype(cls), unk);
    slamhip_or_die(slamhip_map_bind(ctx, id, model(cls), 40, 30, 20, 15, kScale, unk), "map_bind");
    slamhip_or_die(slamhip_map_set_auto_grow(ctx, id, 1), "map_set_auto_grow");
  }
  void append(const LaserScan2D &scan, const RobotPose &pose, double quality) {
    std::vector<double> r, a;
    std::vector<int> occ;
    for (const auto &p : scan.points()) {
      r.push_back(p.range());
      a.push_back(p.angle());
      occ.push_back(p.is_occupied() ? 1 : 0);
    }
    if (r.empty()) return;
    const slamhip_scan_adder_cfg adder = device_adder(cls, quality);
    const double p3[3] = {pose.x, pose.y, pose.theta};
    long long nu = 0;
    slamhip_or_die(slamhip_map_append_scan_raw(ctx, id, &adder, p3, (int)r.size(), r.data(), a.data(), occ.data(), nullptr, &nu),
                   "map_append_scan_raw");
  }
  void build(const GridMap &gt, const LaserScannerParams &lsp) {
    int k = 0;
    for (const auto &p : build_poses()) append(ref_scan(gt, p, lsp), p, build_quality(k++));
  }
  void put_special() {
    if (stride(cls) != 4) return;
    int ox = 0, oy = 0;
    slamhip_or_die(slamhip_map_info(ctx, id, nullptr, nullptr, nullptr, &ox, &oy, nullptr, nullptr), "map_info");
    for (const auto &s : special_cells()) {
      const int xy[2] = {s.x + ox, s.y + oy};
      slamhip_or_die(slamhip_map_apply_dirty(ctx, id, 1, xy, s.tbm), "map_apply_dirty");
    }
  }
};

// ---------------------------------------------------------------------------------------------------------------------
// scan generation

// two scanners, 38 and 90 beams, neither with the default scanner's max_dist of 15 m: 6 m ends some beams short of the far
// walls, 40 m is beyond everything
LaserScannerParams gen_lsp(int cls) { return cls % 2 ? to_lsp(40, 270, 89) : to_lsp(6.0, 270, 37); }

std::vector<double> angle_list(const LaserScannerParams &lsp) {
  std::vector<double> out;
  for (double a = -lsp.h_hsector; a <= lsp.h_hsector; a += lsp.h_angle_inc) {
    if (2 * M_PI <= lsp.h_hsector + a) break;
    out.push_back(a);
  }
  return out;
}

std::vector<RobotPose> gen_poses(const LaserScannerParams &lsp) {
  const auto angles = angle_list(lsp);
  std::vector<RobotPose> p;
  p.push_back(off_boundary({-1.033, -0.448, 0.3}));                   // the middle of the cecum
  p.push_back(off_boundary({-7.137, 1.013, 0.05}));                   // outside the window, looking in
  p.push_back(off_boundary({1.733, -2.148, 2.5}));                    // bottom right, looking at the far corner
  // a cell centre: the middle beam runs down the slope -3, through a grid vertex every third cell, and leaves by the open
  // end, to the right of the trough the updates put into the maps.  (A beam like that must not reach a wall: where the reference's walk ties and goes astray its cell list holds
  // cells the ray never enters, and an occupied one of those fails its "obstacle is not pierced" assertion.  No beam is
  // at a right angle to the middle one: neither 270 / 37 nor 270 / 89 degrees divides 90.)
  p.push_back(RobotPose{0.25, -0.45, std::atan2(-3.0, 1.0) - angles[angles.size() / 2]});
  p.push_back(off_boundary({-1.033, -1.948, -1.57}));                 // out of the open end
  p.push_back(off_boundary({0.667, 1.213, 1.0}));                     // close to the top wall
  p.push_back(off_boundary({-3.533, -1.0512, -0.4}));
  return p;
}

struct GenStats {
  long points = 0, hit_early = 0, hit_late = 0, miss = 0, leaves_window = 0, tie = 0, robot_outside = 0, beams = 0;
};

// what the reference's generator meets on this pose: per beam the cell list it walks
void beam_stats(const GridMap &m, const RobotPose &pose, const LaserScannerParams &lsp, const LaserScan2D &scan, GenStats &st) {
  const auto angles = angle_list(lsp);
  const auto org = m.origin();
  auto inside = [&](const DiscretePoint2D &c) {
    return 0 <= c.x + org.x && c.x + org.x < m.width() && 0 <= c.y + org.y && c.y + org.y < m.height();
  };
  if (!inside(m.world_to_cell(pose.point()))) ++st.robot_outside;
  size_t next = 0;
  for (double a : angles) {
    ++st.beams;
    const Point2D dir{lsp.max_dist * std::cos(a + pose.theta), lsp.max_dist * std::sin(a + pose.theta)};
    const auto cells = m.world_to_cells({pose.point(), pose.point() + dir});
    bool leaves = false, diag = false;
    for (size_t i = 0; i < cells.size(); ++i) {
      if (!inside(cells[i])) leaves = true;
      if (i && cells[i].x != cells[i - 1].x && cells[i].y != cells[i - 1].y) diag = true;
    }
    st.leaves_window += leaves;
    st.tie += diag;
    if (next < scan.points().size() && same_bits(scan.points()[next].angle(), a)) {
      const auto hit = m.world_to_cell(scan.points()[next].move_origin(pose.x, pose.y, pose.theta));
      const size_t at = std::find(cells.begin(), cells.end(), hit) - cells.begin();
      (at < 64 ? st.hit_early : st.hit_late) += 1;
      ++next;
      ++st.points;
    } else {
      ++st.miss;
    }
  }
}

long scan_mismatches(const LaserScan2D &a, const LaserScan2D &b) {
  long mis = 0;
  if (a.points().size() != b.points().size()) return 1000000;
  for (size_t i = 0; i < a.points().size(); ++i) {
    const auto &p = a.points()[i], &q = b.points()[i];
    if (!same_bits(p.range(), q.range()) || !same_bits(p.angle(), q.angle()) || p.is_occupied() != q.is_occupied() ||
        !same_bits(p.factor(), q.factor()))
      ++mis;
  }
  if (!a.trig_provider || !b.trig_provider || typeid(*a.trig_provider) != typeid(*b.trig_provider)) mis += 100000;
  return mis;
}

// a pose on which the library's host routine reports status 2 for some beam (the reference's generator would fail an
// assertion there): searched like tests/golden/make_golden_scan_generate.py searches its touches -- from a cell centre
// pushed a hair aside, along a small rational slope, so that the ray clips cell corners
bool find_assert_pose(const GridMap &m, int cls, const std::vector<double> &angles, double max_dist, double thr, int variant,
                      RobotPose *out, long *tried) {
  const int w = m.width(), h = m.height(), st = stride(cls);
  const auto org = m.origin();
  std::vector<double> cells((size_t)w * h * st);
  double unk[4] = {0, 0, 0, 0};
  payload(cls, *m.new_cell(), unk);
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) payload(cls, m[{x - org.x, y - org.y}], &cells[((size_t)y * w + x) * st]);
  std::mt19937 rs(11);
  const double tiny[] = {3e-8, -3e-8, 5e-8, -5e-8, 1e-9, -1e-9, 0.0};
  const int slope[] = {1, 2, 3, -1, -2, -3};
  std::vector<double> range(angles.size());
  std::vector<unsigned char> status(angles.size());
  for (*tried = 1; *tried <= 200000; ++*tried) {
    const double x0 = ((int)(rs() % 50) - 35 + 0.5) * kScale + tiny[rs() % 7];
    const double y0 = ((int)(rs() % 34) - 20 + 0.5) * kScale + tiny[rs() % 6];
    const int q = slope[rs() % 6], pp = slope[rs() % 6];
    const size_t k = rs() % angles.size();
    const double pose[3] = {x0, y0, std::atan2((double)pp, (double)q) - angles[k]};
    if (slamhip_scan_generate_host(model(cls), model(cls) == SLAMHIP_CELL_TBM ? tbm_kind(cls) : 0, variant, w, h, org.x, org.y, kScale, unk, cells.data(), 1, pose, (int)angles.size(),
                                   angles.data(), max_dist, thr, range.data(), status.data()) != SLAMHIP_OK)
      continue;  // (a robot on a cell boundary: refused)
    if (std::find(status.begin(), status.end(), (unsigned char)2) != status.end()) {
      *out = RobotPose{pose[0], pose[1], pose[2]};
      return true;
    }
  }
  return false;
}

// ---------------------------------------------------------------------------------------------------------------------
// map consumers

std::string read_file(const std::string &path) {
  std::ifstream f(path, std::ios::in | std::ios::binary);
  return std::string((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}
template <typename F>
std::string dumped(const std::string &path, F dump) {
  {
    std::ofstream os(path, std::ios::out | std::ios::binary | std::ios::trunc);
    dump(os);
  }
  return read_file(path);
}
bool file_exists(const std::string &path) { return std::ifstream(path).good(); }

// OccupancyGridPublisher::on_map_update's cell loop (occupancy_grid_publisher.h:37-46) restated -- the ROS headers the
// class includes are not here --: rows bottom-up, value == -1 ? -1 : value * 100 narrowed to int8.  A value that is not
// finite has no defined conversion: -1, as include/slamhip.h says; *not_finite counts them
std::vector<int8_t> publisher_cells(const GridMap &map, long *not_finite) {
  std::vector<int8_t> data;
  const DiscretePoint2D origin = map.origin();
  DiscretePoint2D pnt;
  const DiscretePoint2D end_of_map = DiscretePoint2D(map.width(), map.height()) - origin;
  for (pnt.y = -origin.y; pnt.y < end_of_map.y; ++pnt.y)
    for (pnt.x = -origin.x; pnt.x < end_of_map.x; ++pnt.x) {
      double value = (double)map[pnt];
      if (!std::isfinite(value)) {
        ++*not_finite;
        data.push_back(-1);
        continue;
      }
      int cell_value = value == -1 ? -1 : value * 100;
      data.push_back(cell_value);
    }
  return data;
}

// ---------------------------------------------------------------------------------------------------------------------
// scan probability estimator, raw batch

void hc_props(MapPropertiesProvider &p, int strict, int trig_cache) {
  p.set_property("slam/scmtch/spe/type", "wmpp");
  p.set_property("slam/scmtch/type", "HC");
  p.set_property("slam/scmtch/HC/distortion/translation", "0.1");
  p.set_property("slam/scmtch/HC/distortion/rotation", "0.1");
  p.set_property("slam/scmtch/HC/distortion/failed_attempts_limit", "6");
  p.set_property("slam/scmtch/hip/strict", strict ? "true" : "false");
  p.set_property("slam/scmtch/hip/trig_cache", trig_cache ? "true" : "false");
}

struct Provider {
  LaserScannerParams lsp;
  std::shared_ptr<TrigonometryProvider> make(bool cached) const {
    if (!cached) return std::make_shared<RawTrigonometryProvider>();
    auto p = std::make_shared<CachedTrigonometryProvider>();
    p->update(-lsp.h_hsector, lsp.h_hsector + lsp.h_angle_inc / 2, lsp.h_angle_inc);
    return p;
  }
  HipScanTrig hip(bool cached) const {
    HipScanTrig t;
    if (cached) {
      t.mode = SLAMHIP_TRIG_CACHED;
      t.a_min = -lsp.h_hsector;
      t.a_max = lsp.h_hsector + lsp.h_angle_inc / 2;
      t.a_inc = lsp.h_angle_inc;
    }
    return t;
  }
};

}  // namespace

extern "C" {

// A guard for the entries below, which END THE PROCESS where the reference's generator fails an assertion: the library's
// host routine (no device) over the poses a scene uses.  phase 0: the poses the maps are built and updated from, over the
// cecum (cls is not read); phase 1 -- to be asked only when phase 0 is clean --: the generator poses of the class over
// the class's map at its threshold; phase 2: the same over the map after the first update.  out[i] = beams of pose i with status 2, or -1 where the pose is refused (a robot on
// a cell boundary); returns the number of poses.  (REFC_TRACE in the environment: the status-2 beams go to stderr.)
int refc_pose_check(int cls, int phase, double *out) {
  Scene sc(phase == 0 ? MOCK : cls);
  if (phase == 0) cls = MOCK;
  if (phase == 2 && sc.slam) sc.update(0);
  const size_t n_build = build_poses().size();
  const LaserScannerParams lsp = phase == 0 ? to_lsp(15, 270, 90) : gen_lsp(cls);
  std::vector<RobotPose> poses;
  if (phase == 0) {
    poses = build_poses();
    poses.push_back(extra_pose(0));
    poses.push_back(extra_pose(1));
  } else {
    poses = gen_poses(lsp);
  }
  int variant = -1;
  slamhip_or_die(slamhip_scan_gen_libm_variant(&variant), "scan_gen_libm_variant");
  const auto angles = angle_list(lsp);
  std::vector<double> range(angles.size());
  std::vector<unsigned char> status(angles.size());
  for (size_t i = 0; i < poses.size(); ++i) {
    const GridMap &m = (phase == 0 && i >= n_build) ? *sc.wider : *sc.map;
    const int w = m.width(), h = m.height(), st = stride(cls);
    const auto org = m.origin();
    std::vector<double> cells((size_t)w * h * st);
    double unk[4] = {0, 0, 0, 0};
    payload(cls, *m.new_cell(), unk);
    for (int y = 0; y < h; ++y)
      for (int x = 0; x < w; ++x) payload(cls, m[{x - org.x, y - org.y}], &cells[((size_t)y * w + x) * st]);
    const double p[3] = {poses[i].x, poses[i].y, poses[i].theta};
    if (slamhip_scan_generate_host(model(cls), model(cls) == SLAMHIP_CELL_TBM ? tbm_kind(cls) : 0, variant, w, h, org.x, org.y, kScale, unk,
                                   cells.data(), 1, p, (int)angles.size(), angles.data(), lsp.max_dist, occ_threshold(cls), range.data(),
                                   status.data()) != SLAMHIP_OK)
      out[i] = -1;
    else
      out[i] = (double)std::count(status.begin(), status.end(), (unsigned char)2);
    if (std::getenv("REFC_TRACE"))
      for (size_t b = 0; b < status.size(); ++b)
        if (status[b] == 2) std::fprintf(stderr, "pose %zu beam %zu of %zu angle %.17g heading %.17g\n", i, b, status.size(), angles[b], p[2]);
  }
  return (int)poses.size();
}

// The scene of a cell class on the reference alone.  out (24 doubles):
//  0 width  1 height  2 origin x  3 origin y  4 times the map grew while it was built  5 cells  6 never-observed cells
//  7 distinct PGM grey values  8 scan points  9 hits within 64 cells  10 hits beyond  11 beams without a hit
// 12 beams that leave the window  13 beams with a diagonal step in their cell list (a vertex tie)  14 poses outside the window
// 15 TBM cells with occupied + empty == 0 and unknown < 1  16 cells with conflict  17 cells whose occupancy is not finite
// 18 tries until a pose with an assertion beam was found (0: none)  19 times the map grew in the two updates of the observer scene
// 20 beams
int refc_scene_stats(int cls, double *out) {
  std::memset(out, 0, sizeof(double) * 24);
  Scene sc(cls);
  const GridMap &m = *sc.map;
  const auto org = m.origin();
  out[0] = m.width(); out[1] = m.height(); out[2] = org.x; out[3] = org.y;
  out[4] = sc.slam ? (double)sc.slam->grown : 1.0;  // (the cecum map grew under the patcher)
  out[5] = (double)m.width() * m.height();
  for (int y = 0; y < m.height(); ++y)
    for (int x = 0; x < m.width(); ++x) {
      const GridCell &c = m[{x - org.x, y - org.y}];
      if (c.is_unknown()) out[6] += 1;
      if (!std::isfinite((double)c)) out[17] += 1;
      if (stride(cls) == 4) {
        double p[4];
        payload(cls, c, p);
        if (p[1] + p[2] == 0 && p[0] < 1) out[15] += 1;
        if (p[3] != 0) out[16] += 1;
      }
    }
  {
    char path[] = "/tmp/refc_stats_XXXXXX";
    const int fd = mkstemp(path);
    if (fd < 0) return 3;
    close(fd);
    const std::string bytes = dumped(path, [&](std::ofstream &os) { GridMapToPgmDumber::dump_map(os, m); });
    std::remove(path);
    const std::string header = "P5\n" + std::to_string(m.width()) + "\n" + std::to_string(m.height()) + "\n255\n";
    if (bytes.compare(0, header.size(), header) != 0 || bytes.size() != header.size() + (size_t)m.width() * m.height()) return 4;
    std::set<unsigned char> greys(bytes.begin() + header.size(), bytes.end());
    out[7] = (double)greys.size();
  }
  const LaserScannerParams lsp = gen_lsp(cls);
  GenStats st;
  for (const auto &p : gen_poses(lsp)) beam_stats(m, p, lsp, ref_scan(m, p, lsp, occ_threshold(cls)), st);
  out[8] = (double)st.points; out[9] = (double)st.hit_early; out[10] = (double)st.hit_late; out[11] = (double)st.miss;
  out[12] = (double)st.leaves_window; out[13] = (double)st.tie; out[14] = (double)st.robot_outside; out[20] = (double)st.beams;
  int variant = -1;
  slamhip_or_die(slamhip_scan_gen_libm_variant(&variant), "scan_gen_libm_variant");
  RobotPose bad{0, 0, 0};
  long tried = 0;
  if (variant >= 0 && find_assert_pose(m, cls, angle_list(lsp), lsp.max_dist, occ_threshold(cls), variant, &bad, &tried)) out[18] = (double)tried;
  if (sc.slam) {
    const long g0 = sc.slam->grown;
    sc.update(0);
    sc.update(1);
    out[19] = (double)(sc.slam->grown - g0);
  }
  return 0;
}

// out (16 doubles):
//  0 poses  1 scan points of the reference over the host map  2 mismatches reference over the VIEW against the host map
//  3 mismatches HipLaserScanGenerator::laser_scan_2D against the host map  4 mismatches laser_scans_2D (all poses in one
//  call) against the lone calls  5 the assertion pose was found (tries)  6 it threw std::logic_error from laser_scan_2D
//  7 ... and nothing else was thrown anywhere  8 scan points after the K6 update (reference)  9 mismatches after the update
//  and invalidate() (the device generator, and the reference's generator, over the view of a window K6 built against the
//  reference over its updated map)  10 the view's geometry followed the device window after the update  11 poses whose scan
//  differs between before and after the update (the update is seen at all)  12 mismatches over that view before the update
int refc_scan_generator(int cls, double *out) {
  std::memset(out, 0, sizeof(double) * 16);
  Scene sc(cls);
  slamhip_ctx *ctx = make_ctx();
  if (!ctx) return -1;
  int rc = 0;
  {
    DevMap dev(ctx, 0, cls, *sc.map);
    const LaserScannerParams lsp = gen_lsp(cls);
    const double thr = occ_threshold(cls);
    const auto poses = gen_poses(lsp);
    LaserScanGenerator ref_gen{lsp};
    HipLaserScanGenerator hip_gen{lsp};
    out[0] = (double)poses.size();
    out[7] = 1;
    std::vector<LaserScan2D> lone, before;
    try {
      for (const auto &p : poses) {
        const LaserScan2D a = ref_gen.laser_scan_2D(*sc.map, p, thr);
        const LaserScan2D b = ref_gen.laser_scan_2D(*dev.view, p, thr);
        const LaserScan2D c = hip_gen.laser_scan_2D(*dev.view, p, thr);
        out[1] += (double)a.points().size();
        out[2] += (double)scan_mismatches(a, b);
        out[3] += (double)scan_mismatches(a, c);
        lone.push_back(c);
        before.push_back(a);
      }
      const auto batch = hip_gen.laser_scans_2D(*dev.view, poses, thr);
      if (batch.size() != lone.size()) out[4] = 1000000;
      else
        for (size_t i = 0; i < lone.size(); ++i) out[4] += (double)scan_mismatches(lone[i], batch[i]);
    } catch (const std::exception &e) {
      std::cerr << "refc_scan_generator: " << e.what() << std::endl;
      out[7] = 0;
    }
    // the pose the reference cannot take: only the device generator is run on it
    int variant = -1;
    slamhip_or_die(slamhip_scan_gen_libm_variant(&variant), "scan_gen_libm_variant");
    RobotPose bad{0, 0, 0};
    long tried = 0;
    if (find_assert_pose(*sc.map, cls, hip_gen.angles(), lsp.max_dist, thr, variant, &bad, &tried)) {
      out[5] = (double)tried;
      try {
        hip_gen.laser_scan_2D(*dev.view, bad, thr);
      } catch (const std::logic_error &) {
        out[6] = 1;
      } catch (...) {
        out[7] = 0;
      }
    }
    // one scan more: the reference's adder into the host map, K6 into a device window that K6 built, then invalidate()
    if (sc.slam && out[7] == 1) {
      K6Map k6(ctx, 1, cls);
      k6.build(*sc.gt, sc.slam->lsp);
      k6.put_special();
      HipResidentMapView view(ctx, 1, GridMapParams{40, 30, kScale}, 0.5, tbm_kind(cls));
      try {
        // the view's chunks are filled by a walk of the reference's generator over it, and the window as it is now is
        // the host map as it is now
        for (size_t i = 0; i < poses.size(); ++i) out[12] += (double)scan_mismatches(before[i], ref_gen.laser_scan_2D(view, poses[i], thr));
        LaserScan2D scan;
        RobotPose up{0, 0, 0};
        sc.update(0, &scan, &up);
        k6.append(scan, up, 0.9);
        view.invalidate();
        int w = 0, h = 0, ox = 0, oy = 0;
        slamhip_or_die(slamhip_map_info(ctx, 1, nullptr, &w, &h, &ox, &oy, nullptr, nullptr), "map_info");
        out[10] = (view.width() == w && view.height() == h && view.origin() == DiscretePoint2D{ox, oy} && (w != 40 || h != 30)) ? 1 : 0;
        const auto batch = hip_gen.laser_scans_2D(view, poses, thr);
        for (size_t i = 0; i < poses.size(); ++i) {
          const LaserScan2D a2 = ref_gen.laser_scan_2D(*sc.map, poses[i], thr);
          out[8] += (double)a2.points().size();
          out[9] += (double)scan_mismatches(a2, batch[i]);
          out[9] += (double)scan_mismatches(a2, ref_gen.laser_scan_2D(view, poses[i], thr));
          if (scan_mismatches(a2, before[i])) out[11] += 1;
        }
      } catch (const std::exception &e) {
        std::cerr << "refc_scan_generator: " << e.what() << std::endl;
        out[7] = 0;
      }
    }
  }
  slamhip_ctx_destroy(ctx);
  return rc;
}

// Four scanners: to_lsp(15, 270, 36), to_lsp(15, 270, 89), to_lsp(100, 270, 1000) and the default LaserScannerParams{},
// whose list the 2 pi break cuts short.  The reference's list is read off its own loop: over a map whose every cell is
// occupied each beam hits in the robot's own cell, so the scan's angles ARE the list.
// out: per scanner 3 doubles = length of the reference's list, length of angles(), entries that differ
int refc_angles(double *out) {
  const LaserScannerParams sets[4] = {to_lsp(15, 270, 36), to_lsp(15, 270, 89), to_lsp(100, 270, 1000), LaserScannerParams{}};
  UnboundedPlainGridMap full(std::make_shared<MockGridCell>(1.0), GridMapParams{4, 4, 1.0});
  for (int k = 0; k < 4; ++k) {
    const LaserScan2D s = LaserScanGenerator{sets[k]}.laser_scan_2D(full, RobotPose{0.3, 0.4, 0.0}, 1.0);
    const HipLaserScanGenerator g{sets[k]};
    const auto &a = g.angles();
    out[3 * k] = (double)s.points().size();
    out[3 * k + 1] = (double)a.size();
    long mis = 0;
    for (size_t i = 0; i < std::min(a.size(), s.points().size()); ++i)
      if (!same_bits(a[i], s.points()[i].angle())) ++mis;
    out[3 * k + 2] = (double)mis;
  }
  return 0;
}

// The map consumers.  dir: an empty scratch directory.  out (24 doubles):
//  0 bytes of the reference's dump of the host map  1..3 the three other dumps differ from it (0 / 1): the reference's dumper
//  over the view, HipGridMapToPgmDumper over the view, HipGridMapToPgmDumper over the host map
//  4 + 3 k (k = 0, 1, 2), the k-th on_map_update: the file names are equal and both files exist, the files' bytes are equal,
//  the bytes  13 the three dumps are three different files' worth (the map did change)  14 times the map grew in between
//  15 occupancy-grid cells  16 cells where hip_occupancy_grid over the VIEW differs from the publisher's loop
//  17 ... over the HOST map  18 w, h, ox, oy all equal (both branches)  19 cells whose reference value is not finite
//  20 distinct grey values in the first dump  21 the first update went to "<prefix>_0.pgm"
int refc_observers(int cls, const char *dir, double *out) {
  std::memset(out, 0, sizeof(double) * 24);
  Scene sc(cls);
  slamhip_ctx *ctx = make_ctx();
  if (!ctx) return -1;
  {
    DevMap dev(ctx, 0, cls, *sc.map);
    const std::string d = std::string(dir) + "/";
    const GridMap &host = *sc.map;
    const GridMap &view = *dev.view;
    const std::string want = dumped(d + "a.pgm", [&](std::ofstream &os) { GridMapToPgmDumber::dump_map(os, host); });
    out[0] = (double)want.size();
    out[1] = dumped(d + "b.pgm", [&](std::ofstream &os) { GridMapToPgmDumber::dump_map(os, view); }) != want;
    out[2] = dumped(d + "c.pgm", [&](std::ofstream &os) { HipGridMapToPgmDumper::dump_map(os, view); }) != want;
    out[3] = dumped(d + "d.pgm", [&](std::ofstream &os) { HipGridMapToPgmDumper::dump_map(os, host); }) != want;
    {
      const size_t hdr = want.size() - (size_t)host.width() * host.height();
      std::set<unsigned char> greys(want.begin() + hdr, want.end());
      out[20] = (double)greys.size();
    }
    // the occupancy grid, both branches
    {
      long not_finite = 0;
      const std::vector<int8_t> pub = publisher_cells(host, &not_finite);
      out[15] = (double)pub.size();
      out[19] = (double)not_finite;
      bool geom = true;
      for (int branch = 0; branch < 2; ++branch) {
        std::vector<int8_t> data;
        int w = 0, h = 0, ox = 0, oy = 0;
        hip_occupancy_grid(branch == 0 ? view : host, data, w, h, ox, oy);
        geom = geom && w == host.width() && h == host.height() && ox == host.origin().x && oy == host.origin().y;
        long mis = data.size() == pub.size() ? 0 : 1000000;
        for (size_t i = 0; i < std::min(data.size(), pub.size()); ++i) mis += data[i] != pub[i];
        out[16 + branch] = (double)mis;
      }
      out[18] = geom ? 1 : 0;
    }
    // three updates through the two observers; the map changes (and grows) in between
    GridMapToPgmDumber ref_dumper(d + "ref");
    HipGridMapToPgmDumper hip_dumper(d + "hip");
    std::vector<std::string> seen;
    const long g0 = sc.slam ? sc.slam->grown : 0;
    for (int k = 0; k < 3; ++k) {
      ref_dumper.on_map_update(host);
      hip_dumper.on_map_update(view);
      // (the reference's names: base + "_" + id + ".pgm"; the adapter's own file_name is asked for the same n)
      const std::string ref_name = d + "ref_" + std::to_string(k) + ".pgm", hip_name = hip_dumper.file_name(k);
      const bool names = hip_name == d + "hip_" + std::to_string(k) + ".pgm" && file_exists(ref_name) && file_exists(hip_name) &&
                         !file_exists(d + "hip_" + std::to_string(k + 1) + ".pgm") && !file_exists(d + "ref_" + std::to_string(k + 1) + ".pgm");
      const std::string rb = read_file(ref_name), hb = file_exists(hip_name) ? read_file(hip_name) : std::string();
      out[4 + 3 * k] = names ? 1 : 0;
      out[5 + 3 * k] = (!rb.empty() && rb == hb) ? 1 : 0;
      out[6 + 3 * k] = (double)rb.size();
      seen.push_back(rb);
      if (k == 0) out[21] = file_exists(d + "hip_0.pgm") ? 1 : 0;
      if (k < 2) {
        if (sc.slam) {
          sc.update(k);
        } else {  // the hand-made map: a wall more, beyond the window's right rim, through the patcher
          using C = CecumTextRasterMapPrimitive;
          C c{9 + 4 * k, 7, k ? C::BoundPosition::Bot : C::BoundPosition::Top};
          GridMapPatcher{}.apply_text_raster(*sc.map, c.to_stream(), DiscretePoint2D{27 + 9 * k, 3 - 11 * k}, 1, 1);
        }
        dev.upload(host);
      }
    }
    out[13] = (seen[0] != seen[1] && seen[1] != seen[2] && seen[0] != seen[2]) ? 1 : 0;
    out[14] = sc.slam ? (double)(sc.slam->grown - g0) : (double)(seen[0].size() != seen[2].size());
  }
  slamhip_ctx_destroy(ctx);
  return 0;
}

// HipScanProbabilityEstimator next to WeightedMeanPointProbabilitySPE: one scan, one map, 16 poses.
//   cls      the map's cell class (MEAN .. TBM_UNKNOWN_EVEN)      oope  0 obstacle (the 1-cell one), 1 max, 2 mean, 3 overlap
//   oie      0 discrepancy, 1 occupancy                            weighting 0 even, 1 viny
//   cached   the scan's trig provider                              strict 1: SUM_SEQUENTIAL and the reference's trig bits
//   with_hip 0: the reference alone
// The analysis area of the window OOPEs is NOT square and not centred: bot -0.17, top 0.09, left -0.06, right 0.23.
// out (40 doubles): 0..15 the reference's probabilities, 16..31 the adapter's, 32 points of the filtered scan,
// 33 the adapter's filtered scan differs from the reference's (points), 34 the reference's probability of pose 0 for the
// SECOND scan (two filter_scans in a row), 35 the adapter's, 36 the reference's probability of pose 0 with bot / left
// exchanged in the area (what a permutation would give)
int refc_spe(int cls, int oope, int oie, int weighting, int cached, int strict, int with_hip, double *out) {
  std::memset(out, 0, sizeof(double) * 40);
  Scene sc(cls, false);  // (a scorer meets what scans leave in a map: no hand-made beliefs)
  MapPropertiesProvider props;
  mapping_props(props, cls);
  hc_props(props, strict, cached);
  static const char *oopes[] = {"obstacle", "max", "mean", "overlap"};
  props.set_property("slam/scmtch/oope/type", oopes[oope]);
  props.set_property("slam/scmtch/oie/type", oie ? "occupancy" : "discrepancy");
  props.set_property("slam/scmtch/spe/wmpp/weighting/type", weighting ? "viny" : "even");
  auto ref_spe = std::dynamic_pointer_cast<WeightedMeanPointProbabilitySPE>(init_spe(props));
  const Provider prov{to_lsp(15, 270, 90)};
  const RobotPose truth = off_boundary({-1.233, -0.648, 1.1}), truth2 = off_boundary({-0.433, -1.148, 2.3});
  LaserScan2D raw = ref_scan(*sc.gt, truth, prov.lsp), raw2 = ref_scan(*sc.gt, truth2, prov.lsp);
  raw.trig_provider = prov.make(cached != 0);
  raw2.trig_provider = prov.make(cached != 0);
  using SPEParams = ScanProbabilityEstimator::SPEParams;
  SPEParams params;
  if (oope != 0) params.sp_analysis_area = LightWeightRectangle{-0.17, 0.09, -0.06, 0.23};
  std::vector<RobotPose> poses;
  for (int k = 0; k < 16; ++k)
    poses.push_back(RobotPose{truth.x + 0.07 * std::sin(1.3 * k), truth.y + 0.05 * std::cos(0.7 * k + 0.4), truth.theta + 0.03 * std::sin(2.1 * k + 1)});
  const GridMap &map = *sc.map;
  const LaserScan2D fr = ref_spe->filter_scan(raw, poses[0], map);
  out[32] = (double)fr.points().size();
  for (int k = 0; k < 16; ++k) out[k] = ref_spe->estimate_scan_probability(fr, poses[k], map, params);
  {
    SPEParams sw = params;
    const auto &r = params.sp_analysis_area;
    sw.sp_analysis_area = LightWeightRectangle{r.left(), r.top(), r.bot(), r.right()};
    out[36] = ref_spe->estimate_scan_probability(fr, poses[0], map, sw);
  }
  const LaserScan2D fr2 = ref_spe->filter_scan(raw2, poses[0], map);
  out[34] = ref_spe->estimate_scan_probability(fr2, poses[0], map, params);
  if (!with_hip) return 0;
  slamhip_ctx *ctx = make_ctx();
  if (!ctx) return -1;
  {
    slamhip_spe_cfg cfg{};
    cfg.oope = oope;  // (SLAMHIP_OOPE_* are numbered like this entry's argument)
    cfg.oie = oie ? SLAMHIP_OIE_OCCUPANCY : SLAMHIP_OIE_DISCREPANCY;
    cfg.sum_order = strict ? SLAMHIP_SUM_SEQUENTIAL : SLAMHIP_SUM_TREE256;
    cfg.pose_trig = !strict ? SLAMHIP_POSE_TRIG_DEVICE : (cached ? SLAMHIP_POSE_TRIG_HOST : SLAMHIP_POSE_TRIG_RAW_EXACT);
    // TBM cells score through their masses under the discrepancy OIE, everything else through occupancy().prob_occ
    // (host/slamhip_init_scan_matching.h)
    const int mirror_model = (stride(cls) == 4 && !oie) ? SLAMHIP_CELL_TBM : SLAMHIP_CELL_OCC;
    auto mirror = std::make_shared<HipMapMirror>(ctx, 0, mirror_model, false);
    auto host_spe = std::dynamic_pointer_cast<WeightedMeanPointProbabilitySPE>(init_spe(props));
    HipScanProbabilityEstimator hip_spe(host_spe, ctx, cfg, mirror, weighting, prov.hip(cached != 0));
    const LaserScan2D fh = hip_spe.filter_scan(raw, poses[0], map);
    out[33] = (double)scan_mismatches(fr, fh);
    for (int k = 0; k < 16; ++k) out[16 + k] = hip_spe.estimate_scan_probability(fh, poses[k], map, params);
    const LaserScan2D fh2 = hip_spe.filter_scan(raw2, poses[0], map);
    out[35] = hip_spe.estimate_scan_probability(fh2, poses[0], map, params);
  }
  slamhip_ctx_destroy(ctx);
  return 0;
}

// hip_process_raw_scans: three HipGridScanMatchers on one context, each with its own map, scanner and pose --
//   robot 0  mean_probability, 90 beams          robot 1  affine_quality_merge, 61 beams, viny weights, sp_skip_rate 3 and
//                                                         sp_max_usable_range 3.1
//   robot 2  mean_probability (a map of its own), 45 beams
// Rounds: 0 all three; 1 robot 1's scan has NO points; 2 robot 2's scan filters to nothing (every point unoccupied);
// 3 K = 1 (robot 1 alone).
// out: per round and robot 13 doubles = 0..3 the job's delta and probability, 4..7 the owner's own process_scan (a second,
// identical set of matchers, so that no state is shared), 8..11 the reference's GridScanMatcher::process_scan, 12 the job
// ran in this round; then at 4 * 3 * 13 = 156: the callers' scans and maps were left unchanged (1 / 0)
int refc_raw_batch(int strict, int with_hip, double *out) {
  std::memset(out, 0, sizeof(double) * 160);
  const auto gt = make_cecum_map();
  const int classes[3] = {MEAN, AFFINE, MEAN};  // (two cell classes of ONE cell model: the shared launches ask for that)
  const int beams[3] = {90, 61, 45};
  std::vector<std::unique_ptr<SlamMap>> maps;
  std::vector<MapPropertiesProvider> props(3);
  std::vector<RobotPose> truth, init;
  for (int r = 0; r < 3; ++r) {
    maps.push_back(std::make_unique<SlamMap>(classes[r]));
    maps[r]->build(*gt);
    if (r == 2) maps[r]->append(*make_wider_world(), extra_pose(0), 0.9);  // (a map of its own)
    mapping_props(props[r], classes[r]);
    hc_props(props[r], strict, 0);
    props[r].set_property("slam/scmtch/oope/type", "obstacle");
    props[r].set_property("slam/scmtch/spe/wmpp/weighting/type", r == 1 ? "viny" : "even");
    if (r == 1) {
      props[r].set_property("slam/scmtch/spe/wmpp/sp_skip_rate", "3");
      props[r].set_property("slam/scmtch/spe/wmpp/sp_max_usable_range", "3.1");
    }
    truth.push_back(off_boundary({-1.533 + 0.9 * r, -0.748 + 0.3 * r, 1.3 + 0.5 * r}));
    init.push_back(RobotPose{truth[r].x + 0.06 - 0.05 * r, truth[r].y - 0.04 + 0.03 * r, truth[r].theta + 0.03 - 0.025 * r});
  }
  std::vector<TransformedLaserScan> scans(3);
  for (int r = 0; r < 3; ++r) {
    scans[r].scan = ref_scan(*gt, truth[r], to_lsp(15, 270, beams[r]));
    scans[r].quality = 1.0;
    scans[r].pose_delta = RobotPoseDelta{0, 0, 0};
  }
  TransformedLaserScan none = scans[1], unoccupied = scans[2];
  none.scan.points().clear();
  for (auto &p : unoccupied.scan.points()) p = ScanPoint2D::make_polar(p.range(), p.angle(), false);

  slamhip_ctx *ctx = nullptr;
  std::vector<std::shared_ptr<HipGridScanMatcher>> batch_owner(3), lone_owner(3);
  if (with_hip) {
    ctx = make_ctx();
    if (!ctx) return -1;
    for (int r = 0; r < 3; ++r) {
      batch_owner[r] = std::dynamic_pointer_cast<HipGridScanMatcher>(init_hip_scan_matcher(props[r], ctx, r));
      lone_owner[r] = std::dynamic_pointer_cast<HipGridScanMatcher>(init_hip_scan_matcher(props[r], ctx, 10 + r));
    }
  }
  bool untouched = true;
  for (int round = 0; round < 4; ++round) {
    std::vector<int> robots = round == 3 ? std::vector<int>{1} : std::vector<int>{0, 1, 2};
    std::vector<const TransformedLaserScan *> given(3);
    for (int r = 0; r < 3; ++r) given[r] = (round == 1 && r == 1) ? &none : ((round == 2 && r == 2) ? &unoccupied : &scans[r]);
    std::vector<HipRawScanJob> jobs;
    std::vector<TransformedLaserScan> copies;
    for (int r : robots) copies.push_back(*given[r]);
    for (size_t j = 0; j < robots.size(); ++j) {
      const int r = robots[j];
      double *row = out + (size_t)(round * 3 + r) * 13;
      row[12] = 1;
      // the reference's matcher, made anew (no state carried from round to round)
      if (!given[r]->scan.points().empty()) {
        RobotPoseDelta d{0, 0, 0};
        const double p = init_scan_matcher(props[r])->process_scan(*given[r], init[r], *maps[r]->map, d);
        row[8] = d.x; row[9] = d.y; row[10] = d.theta; row[11] = p;
      } else {
        // (a scan without points: every estimate is the unknown probability, nothing is accepted)
        row[8] = row[9] = row[10] = 0;
        row[11] = std::numeric_limits<double>::quiet_NaN();
      }
      if (with_hip) {
        RobotPoseDelta d{0, 0, 0};
        const double p = lone_owner[r]->process_scan(*given[r], init[r], *maps[r]->map, d);
        row[4] = d.x; row[5] = d.y; row[6] = d.theta; row[7] = p;
        jobs.push_back(HipRawScanJob{batch_owner[r].get(), &copies[j], &init[r], maps[r]->map.get(), RobotPoseDelta{9, 9, 9}, -7.0});
      }
    }
    if (with_hip) {
      std::vector<std::vector<double>> payload_before;
      for (int r : robots) {
        std::vector<double> pl;
        const GridMap &m = *maps[r]->map;
        const auto org = m.origin();
        for (int y = 0; y < m.height(); ++y)
          for (int x = 0; x < m.width(); ++x) {
            double p[4] = {0, 0, 0, 0};
            payload(classes[r], m[{x - org.x, y - org.y}], p);
            pl.insert(pl.end(), p, p + 4);
          }
        payload_before.push_back(pl);
      }
      hip_process_raw_scans(*batch_owner[robots[0]], jobs);
      for (size_t j = 0; j < robots.size(); ++j) {
        const int r = robots[j];
        double *row = out + (size_t)(round * 3 + r) * 13;
        row[0] = jobs[j].pose_delta.x; row[1] = jobs[j].pose_delta.y; row[2] = jobs[j].pose_delta.theta; row[3] = jobs[j].prob;
        if (scan_mismatches(copies[j].scan, given[r]->scan)) untouched = false;
        std::vector<double> pl;
        const GridMap &m = *maps[r]->map;
        const auto org = m.origin();
        for (int y = 0; y < m.height(); ++y)
          for (int x = 0; x < m.width(); ++x) {
            double p[4] = {0, 0, 0, 0};
            payload(classes[r], m[{x - org.x, y - org.y}], p);
            pl.insert(pl.end(), p, p + 4);
          }
        if (pl.size() != payload_before[j].size() || std::memcmp(pl.data(), payload_before[j].data(), pl.size() * sizeof(double)) != 0)
          untouched = false;
      }
    }
  }
  out[156] = untouched ? 1 : 0;
  batch_owner.clear();
  lone_owner.clear();
  if (ctx) slamhip_ctx_destroy(ctx);
  return 0;
}

}  // extern "C"
