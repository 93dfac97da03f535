// oracle/ref_credibilist_harness.cpp -- TEST INFRASTRUCTURE ONLY (built where the reference tree exists).
//
// host/slamhip_credibilist_slam.h RUN next to the UNMODIFIED reference headers.  slams/credibilist/grid_cell.h defines
// non-inline functions, so that header goes into ONE translation unit of a program: this shared object is it.
//   refcred_loop          init_credibilist_slam(props) and init_hip_resident_credibilist_slam(props) over one loop of
//                         generated scans with odometry error, as oracle/ref_world_harness.cpp runs its worlds: poses after
//                         every scan, the scan qualities the worlds chose, the final beliefs mass by mass, world->map()
//                         through the view
//   refcred_host_matcher  init_hip_credibilist_scan_matcher over a HOST map of CredibilistCell (mirrored through
//                         slamhip_credibilist_belief) next to the reference's matcher on the same map
//   refcred_refusal       oie/type = occupancy: the factory prints its message and ends the process (run in a child)
// with_hip = 0: the reference alone, no device call (tests/test_adapter_scenes_reference.py).
// Output: oracle/_ref/libslamref_credibilist.so (links slam-constructor_amd/libslamhip.so).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <limits>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#define private public
#define protected public
#include "utils/init_slam.h"
#include "slams/credibilist/init_slam.h"
#include "utils/data_generation/map_primitives.h"
#include "utils/data_generation/grid_map_patcher.h"
#include "utils/data_generation/laser_scan_generator.h"
#include "../test/core/mock_grid_cell.h"
#include "slamhip_credibilist_slam.h"
#undef private
#undef protected

#include "ref_adapter_scenes.h"

namespace {

using namespace scn;

// matcher 0: MC, 1: HC (the parameters of oracle/ref_world_harness.cpp)
void fill_props(MapPropertiesProvider &p, int matcher, int strict, int trig_cache, const char *oie = "discrepancy") {
  auto S = [&](const char *k, const std::string &v) { p.set_property(k, v); };
  mapping_props(p, CREDIBILIST);
  S("slam/map/height_in_meters", "4");  // 40 x 40 cells to start from: the loop leaves them
  S("slam/map/width_in_meters", "4");
  S("slam/scmtch/spe/type", "wmpp");
  S("slam/scmtch/spe/wmpp/weighting/type", "even");
  S("slam/scmtch/oie/type", oie);
  if (matcher == 0) {
    S("slam/scmtch/type", "MC");
    S("slam/scmtch/MC/dispersion/translation", "0.2");
    S("slam/scmtch/MC/dispersion/rotation", "0.1");
    S("slam/scmtch/MC/dispersion/failed_attempts_limit", "20");
    S("slam/scmtch/MC/attempts_limit", "100");
    S("slam/scmtch/MC/seed", "424242");
  } else {
    S("slam/scmtch/type", "HC");
    S("slam/scmtch/HC/distortion/translation", "0.1");
    S("slam/scmtch/HC/distortion/rotation", "0.1");
    S("slam/scmtch/HC/distortion/failed_attempts_limit", "6");
  }
  S("slam/scmtch/hip/strict", strict ? "true" : "false");
  S("slam/scmtch/hip/trig_cache", trig_cache ? "true" : "false");
}

struct Calls : public GridScanMatcherObserver {
  long tests = 0, updates = 0;
  void on_scan_test(const RobotPose &, const LaserScan2D &, double) override { ++tests; }
  void on_pose_update(const RobotPose &, const LaserScan2D &, double) override { ++updates; }
};

// the room of oracle/ref_world_harness.cpp
std::shared_ptr<GridMap> make_room() {
  auto gt = std::make_shared<UnboundedPlainGridMap>(std::make_shared<MockGridCell>(0.0), GridMapParams{300, 300, kScale});
  using C = CecumTextRasterMapPrimitive;
  C c1{81, 60, C::BoundPosition::Top}, c2{31, 21, C::BoundPosition::Bot};
  GridMapPatcher{}.apply_text_raster(*gt, c1.to_stream(), DiscretePoint2D{-40, 35}, 1, 1);
  GridMapPatcher{}.apply_text_raster(*gt, c2.to_stream(), DiscretePoint2D{-15, -6}, 1, 1);
  return gt;
}

std::shared_ptr<TrigonometryProvider> provider(const LaserScannerParams &lsp, bool cached) {
  if (!cached) return std::make_shared<RawTrigonometryProvider>();
  auto p = std::make_shared<CachedTrigonometryProvider>();
  p->update(-lsp.h_hsector, lsp.h_hsector + lsp.h_angle_inc / 2, lsp.h_angle_inc);
  return p;
}

void belief_of(const GridCell &c, double *p) { payload(CREDIBILIST, c, p); }

}  // namespace

extern "C" {

// poses_out: n_scans x 6 (reference x, y, theta, resident world x, y, theta) after every scan
// quality_out: n_scans x 2, the scan quality the two worlds gave each scan (0.9 localized, 0.6 raw)
// out (16 doubles): 0 poses that differ (bitwise)  1 max |pose difference|  2 cells compared  3 cells whose four masses differ
// (bitwise)  4 max |mass difference|  5, 6 scan tests (reference, resident)  7, 8 accepted poses  9 times the HBM window grew
// 10, 11 the reference map's final width and height  12 cells where world->map() through the view differs from the
// reference map's occupancy()  13 the reference map grew  14 known cells of the reference map
int refcred_loop(int matcher, int strict, int trig_cache, int n_scans, int with_hip, double *poses_out, double *quality_out,
                 double *out) {
  std::memset(out, 0, sizeof(double) * 16);
  std::memset(poses_out, 0, sizeof(double) * 6 * n_scans);
  std::memset(quality_out, 0, sizeof(double) * 2 * n_scans);
  const auto gt = make_room();
  MapPropertiesProvider props;
  fill_props(props, matcher, strict, trig_cache);
  auto ref = init_credibilist_slam(props);
  const int w0 = ref->map().width(), h0 = ref->map().height();
  slamhip_ctx *ctx = nullptr;
  std::shared_ptr<HipResidentWorld> hip;
  auto c_ref = std::make_shared<Calls>(), c_hip = std::make_shared<Calls>();
  ref->add_sm_observer(c_ref);
  if (with_hip) {
    if (slamhip_ctx_create(0, &ctx) != SLAMHIP_OK) {
      std::cerr << "refcred: " << slamhip_last_error() << std::endl;
      return -1;
    }
    hip = init_hip_resident_credibilist_slam(props, ctx, 0);
    hip->add_sm_observer(c_hip);
  }
  const LaserScannerParams lsp = to_lsp(15, 270, 90);
  RobotPose truth{kScale / 2, kScale / 2 - 6 * kScale, deg2rad(90)};
  RobotPose prev_odom{0, 0, 0};
  for (int k = 0; k < n_scans; ++k) {
    TransformedLaserScan ts;
    ts.scan = LaserScanGenerator{lsp}.laser_scan_2D(*gt, truth, 1);
    ts.scan.trig_provider = provider(lsp, trig_cache != 0);
    ts.quality = 1.0;
    const double ex = 0.03 * std::sin(1.7 * k), ey = -0.025 * std::cos(0.9 * k), et = 0.02 * std::sin(0.6 * k + 1);
    RobotPose odom{truth.x + ex, truth.y + ey, truth.theta + et};
    ts.pose_delta = k == 0 ? RobotPoseDelta{truth.x, truth.y, truth.theta}
                           : RobotPoseDelta{odom.x - prev_odom.x, odom.y - prev_odom.y, odom.theta - prev_odom.theta};
    prev_odom = k == 0 ? truth : odom;
    TransformedLaserScan ts_hip = ts;
    ts_hip.scan.trig_provider = provider(lsp, trig_cache != 0);  // (a provider keeps a base angle: one per world)
    ref->handle_sensor_data(ts);
    const RobotPose pr = ref->pose();
    poses_out[6 * k + 0] = pr.x; poses_out[6 * k + 1] = pr.y; poses_out[6 * k + 2] = pr.theta;
    quality_out[2 * k] = ts.quality;
    if (hip) {
      hip->handle_sensor_data(ts_hip);
      const RobotPose ph = hip->pose();
      poses_out[6 * k + 3] = ph.x; poses_out[6 * k + 4] = ph.y; poses_out[6 * k + 5] = ph.theta;
      quality_out[2 * k + 1] = ts_hip.quality;
      if (std::memcmp(&poses_out[6 * k], &poses_out[6 * k + 3], 3 * sizeof(double)) != 0) out[0] += 1;
      out[1] = std::max({out[1], std::fabs(pr.x - ph.x), std::fabs(pr.y - ph.y), std::fabs(pr.theta - ph.theta)});
    }
    truth = RobotPose{truth.x + 0.04 * std::cos(0.35 * k), truth.y + 0.09, truth.theta + 0.015 * std::sin(0.8 * k)};
    truth = off_boundary(truth);
  }
  const GridMap &mr = ref->map();
  const auto org = mr.origin();
  out[5] = (double)c_ref->tests; out[7] = (double)c_ref->updates;
  out[10] = mr.width(); out[11] = mr.height();
  out[13] = (mr.width() != w0 || mr.height() != h0) ? 1 : 0;
  for (int y = 0; y < mr.height(); ++y)
    for (int x = 0; x < mr.width(); ++x)
      if (!mr[{x - org.x, y - org.y}].is_unknown()) out[14] += 1;
  if (hip) {
    out[6] = (double)c_hip->tests; out[8] = (double)c_hip->updates;
    slamhip_ctx_synchronize(ctx);
    int model = 0, w = 0, h = 0, ox = 0, oy = 0;
    long long grown = 0;
    slamhip_or_die(slamhip_map_info(ctx, 0, &model, &w, &h, &ox, &oy, nullptr, &grown), "map_info");
    out[9] = (double)grown;
    std::vector<double> dev((size_t)w * h * 4);
    slamhip_or_die(slamhip_map_download_window(ctx, 0, 0, 0, w, h, dev.data()), "map_download_window");
    const double unk[4] = {1, 0, 0, 0};
    const GridMap &mv = hip->map();
    for (int y = 0; y < mr.height(); ++y)
      for (int x = 0; x < mr.width(); ++x) {
        const GridMap::Coord c{x - org.x, y - org.y};
        double a[4], b[4];
        belief_of(mr[c], a);
        const int ix = c.x + ox, iy = c.y + oy;
        if (0 <= ix && ix < w && 0 <= iy && iy < h) std::memcpy(b, &dev[((size_t)iy * w + ix) * 4], sizeof b);
        else std::memcpy(b, unk, sizeof b);
        out[2] += 1;
        if (std::memcmp(a, b, sizeof a) != 0) {
          out[3] += 1;
          for (int k = 0; k < 4; ++k) out[4] = std::max(out[4], std::fabs(a[k] - b[k]));
        }
        const double oa = mr.occupancy(c), ob = mv.occupancy(c);
        if (std::memcmp(&oa, &ob, sizeof(double)) != 0) out[12] += 1;
      }
    hip.reset();
    slamhip_ctx_destroy(ctx);
  }
  return 0;
}

// One process_scan over a HOST map of CredibilistCell built by the reference's scan adder (oracle/ref_adapter_scenes.h).
// out (16 doubles): 0-2 delta, 3 probability, 4 scan tests, 5 accepted poses (reference); 6-11 the same of the HIP matcher;
// 12 full uploads of its mirror, 13 known cells of the map
int refcred_host_matcher(int matcher, int strict, int trig_cache, int with_hip, double *out) {
  std::memset(out, 0, sizeof(double) * 16);
  const auto gt = make_cecum_map();
  SlamMap sm(CREDIBILIST);
  sm.build(*gt);
  MapPropertiesProvider props;
  fill_props(props, matcher, strict, trig_cache);
  const LaserScannerParams lsp = to_lsp(15, 270, 90);
  const RobotPose truth = off_boundary({-1.233, -0.648, 1.1});
  const RobotPose init{truth.x + 0.06, truth.y - 0.04, truth.theta + 0.03};
  TransformedLaserScan ts;
  ts.scan = ref_scan(*gt, truth, lsp);
  ts.scan.trig_provider = provider(lsp, trig_cache != 0);
  ts.quality = 1.0;
  ts.pose_delta = RobotPoseDelta{0, 0, 0};
  const GridMap &map = *sm.map;
  const auto org = map.origin();
  for (int y = 0; y < map.height(); ++y)
    for (int x = 0; x < map.width(); ++x)
      if (!map[{x - org.x, y - org.y}].is_unknown()) out[13] += 1;
  {
    auto ref = init_scan_matcher(props);
    auto calls = std::make_shared<Calls>();
    ref->subscribe(calls);
    RobotPoseDelta d{0, 0, 0};
    const double p = ref->process_scan(ts, init, map, d);
    out[0] = d.x; out[1] = d.y; out[2] = d.theta; out[3] = p; out[4] = (double)calls->tests; out[5] = (double)calls->updates;
  }
  if (!with_hip) return 0;
  slamhip_ctx *ctx = nullptr;
  if (slamhip_ctx_create(0, &ctx) != SLAMHIP_OK) {
    std::cerr << "refcred: " << slamhip_last_error() << std::endl;
    return -1;
  }
  {
    TransformedLaserScan th = ts;
    th.scan.trig_provider = provider(lsp, trig_cache != 0);
    auto hip = std::dynamic_pointer_cast<HipGridScanMatcher>(init_hip_credibilist_scan_matcher(props, ctx, 0));
    auto calls = std::make_shared<Calls>();
    hip->subscribe(calls);
    RobotPoseDelta d{0, 0, 0};
    const double p = hip->process_scan(th, init, map, d);
    out[6] = d.x; out[7] = d.y; out[8] = d.theta; out[9] = p; out[10] = (double)calls->tests; out[11] = (double)calls->updates;
    out[12] = (double)hip->mirror().full_uploads();
  }
  slamhip_ctx_destroy(ctx);
  return 0;
}

// oie/type = occupancy: init_hip_credibilist_scan_matcher prints its message and ends the process before any device
// call.  Returns only if it did not.
int refcred_refusal() {
  MapPropertiesProvider props;
  fill_props(props, 1, 1, 0, "occupancy");
  auto m = init_hip_credibilist_scan_matcher(props);
  return m ? 1 : 2;
}

}  // extern "C"
