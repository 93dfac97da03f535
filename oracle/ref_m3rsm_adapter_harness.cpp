// oracle/ref_m3rsm_adapter_harness.cpp -- TEST INFRASTRUCTURE ONLY (built where the reference tree exists).
//
// Drop-in proof of the BF_M3RSM host adapter: HipM3rsmMap / HipM3rsmEngine (slam-constructor_amd/host/slamhip_m3rsm_map.h),
// the BF_M3RSM branch of init_hip_scan_matcher (host/slamhip_init_scan_matching.h) and HipGridScanMatcher over a
// resident map, next to the UNMODIFIED reference headers over a loop of scans:
//   refm3_loop                 per scan: the fine map, the levels and one match through the two factories
//   refm3_engine               the request surface: many-to-many and match-each, both trig providers
//   refm3_reference_selfcheck  the loop on the reference alone (touches nothing of the device library)
//   refm3_edge                 one match on a scene whose end points lie ON cell edges: the raw provider told from the cached
// The reference never lowers a coarse cell (m3rsm_engine.h:96), the device's levels are the tight maximum: the levels and
// the matches are held against a TWIN -- a fresh M3RSMRescalableGridMap that gets the loop map's known fine cells in
// the device's total order (impact descending, then fine x, then fine y), so that every coarse cell is set once, by its
// winner.  That the twin is tight is asserted, cell by cell, before anything is compared with it.
// Access control is relaxed only to move the fine map's origin off its centre, to reach a level's own map and to read the
// library matcher a HipGridScanMatcher owns (slamhip_matcher_stats).
// Output: oracle/_ref/libslamref_m3rsm_adapter.so (links slam-constructor_amd/libslamhip.so).
#include <algorithm>
#include <array>
#include <cassert>
#include <chrono>
#include <cmath>
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
#include <string>
#include <tuple>
#include <typeinfo>
#include <unordered_map>
#include <unordered_set>
#include <utility>
#include <vector>

#define private public
#define protected public
#include "utils/init_scan_matching.h"
#include "utils/init_occupancy_mapping.h"
#include "utils/data_generation/map_primitives.h"
#include "utils/data_generation/grid_map_patcher.h"
#include "utils/data_generation/laser_scan_generator.h"
#include "../test/core/mock_grid_cell.h"
#include "slamhip_init_scan_matching.h"
#include "slamhip_m3rsm_map.h"
#undef private
#undef protected

namespace {

using Map = M3RSMRescalableGridMap<UnboundedPlainGridMap>;
constexpr double kScale = 0.1;
constexpr int kBeams = 90, kRow = 28, kFreshLevelId = 40;

std::string num(double v) {
  char b[40];
  std::snprintf(b, sizeof b, "%.17g", v);
  return b;
}

// scene 0: MeanProbabilityCell, even weights; scene 1: TbmOccConsistentCell, vinySLAM's weights and qualities; scene 2: the
// same cells under even weights
// variant 0: blur 0.3; 1: a dynamic blur; 2: max_range shorter than some beams; 3: 2 + beams without a return (+inf)
struct Variant {
  double blur, max_range;
  bool no_return;
};
Variant variant_of(int v) {
  const double inf = std::numeric_limits<double>::infinity();
  switch (v) {
    case 0: return {0.3, inf, false};
    case 1: return {-0.02, inf, false};
    case 2: return {0.3, 2.5, false};
    default: return {0.3, 2.5, true};
  }
}

void fill_props(MapPropertiesProvider &p, int scene, int variant, int strict, int trig_cache) {
  auto S = [&](const char *k, const std::string &v) { p.set_property(k, v); };
  const Variant va = variant_of(variant);
  S("slam/mapping/blur", num(va.blur));
  if (std::isfinite(va.max_range)) S("slam/mapping/max_range", num(va.max_range));
  S("slam/occupancy_estimator/type", "const");
  S("slam/occupancy_estimator/base_occupied/prob", "0.95");
  S("slam/occupancy_estimator/base_empty/prob", "0.01");
  if (scene == 0) {
    S("slam/mapping/grid/area/type", "mean_probability");
    S("slam/scmtch/spe/wmpp/weighting/type", "even");
  } else {
    S("slam/occupancy_estimator/base_occupied/qual", "0.04");
    S("slam/occupancy_estimator/base_empty/qual", "0.003");
    S("slam/mapping/grid/area/type", "tbm_consistent");
    S("slam/scmtch/spe/wmpp/weighting/type", scene == 1 ? "viny" : "even");
  }
  S("slam/mapping/grid/type", "unbounded_plain");
  S("slam/map/meters_per_cell", num(kScale));
  S("slam/scmtch/spe/type", "wmpp");
  S("slam/scmtch/oope/type", "max");
  S("slam/scmtch/type", "BF_M3RSM");
  // every one non-default, no two alike
  S("slam/scmtch/BF_M3RSM/limits/x_translation", "0.3");
  S("slam/scmtch/BF_M3RSM/limits/y_translation", "0.2");
  S("slam/scmtch/BF_M3RSM/limits/rotation", num(deg2rad(3)));
  S("slam/scmtch/BF_M3RSM/accuracy/rotation", num(deg2rad(1)));
  S("slam/scmtch/BF_M3RSM/accuracy/translation", "0.05");
  S("slam/scmtch/hip/strict", strict ? "true" : "false");
  S("slam/scmtch/hip/trig_cache", trig_cache ? "true" : "false");
}

void payload(int stride, const GridCell &c, double *p) {
  if (stride == 4) {
    const auto &b = static_cast<const TbmBaseCell &>(c).belief();
    p[0] = b.unknown(); p[1] = b.empty(); p[2] = b.occupied(); p[3] = b.conflict();
  } else {
    p[0] = c.occupancy().prob_occ;
  }
}

// counts the scorer calls of the reference's matcher, as tests/golden/m3rsm_harness.cpp records them
class CountingSPE : public ScanProbabilityEstimator {
public:
  explicit CountingSPE(std::shared_ptr<ScanProbabilityEstimator> real)
      : ScanProbabilityEstimator{real->occupancy_observation_probability_estimator()}, _real{real} {}
  LaserScan2D filter_scan(const LaserScan2D &scan, const RobotPose &pose, const GridMap &map) override {
    return _real->filter_scan(scan, pose, map);
  }
  double estimate_scan_probability(const LaserScan2D &scan, const RobotPose &pose, const GridMap &map,
                                   const SPEParams &params) const override {
    ++calls;
    return _real->estimate_scan_probability(scan, pose, map, params);
  }
  mutable long calls = 0;

private:
  std::shared_ptr<ScanProbabilityEstimator> _real;
};

struct Events : public GridScanMatcherObserver {
  long starts = 0, ends = 0, tests = 0, updates = 0;
  RobotPose end_delta{0, 0, 0};  // (the interface hands the delta over as a RobotPose)
  double end_prob = 0;
  void on_matching_start(const RobotPose &, const TransformedLaserScan &, const GridMap &) override { ++starts; }
  void on_scan_test(const RobotPose &, const LaserScan2D &, double) override { ++tests; }
  void on_pose_update(const RobotPose &, const LaserScan2D &, double) override { ++updates; }
  void on_matching_end(const RobotPose &d, const LaserScan2D &, double prob) override {
    ++ends;
    end_delta = d;
    end_prob = prob;
  }
  bool saw(const RobotPoseDelta &d, double prob) const {
    return starts == 1 && ends == 1 && tests == 0 && updates == 0 && std::memcmp(&d.x, &end_delta.x, sizeof(double)) == 0 &&
           std::memcmp(&d.y, &end_delta.y, sizeof(double)) == 0 && std::memcmp(&d.theta, &end_delta.theta, sizeof(double)) == 0 &&
           std::memcmp(&prob, &end_prob, sizeof(double)) == 0;
  }
};

// the room of oracle/ref_world_harness.cpp, from the reference's data-generation utilities
std::shared_ptr<GridMap> make_room() {
  auto gt = std::make_shared<UnboundedPlainGridMap>(std::make_shared<MockGridCell>(0.0), GridMapParams{300, 300, kScale});
  using C = CecumTextRasterMapPrimitive;
  C c1{81, 60, C::BoundPosition::Top}, c2{31, 21, C::BoundPosition::Bot};
  GridMapPatcher{}.apply_text_raster(*gt, c1.to_stream(), DiscretePoint2D{-40, 35}, 1, 1);
  GridMapPatcher{}.apply_text_raster(*gt, c2.to_stream(), DiscretePoint2D{-15, -6}, 1, 1);
  return gt;
}

RobotPose off_boundary(RobotPose p) {  // (the generator's "not on a cell boundary" precondition)
  if (std::fabs(p.x / kScale - std::round(p.x / kScale)) < 1e-3) p.x += 0.013;
  if (std::fabs(p.y / kScale - std::round(p.y / kScale)) < 1e-3) p.y += 0.013;
  return p;
}

// the scanner: 270 degrees in steps of 3; the cached provider's table is made over the same accumulated angles
struct Scanner {
  LaserScannerParams lsp = to_lsp(15, 270, kBeams);
  std::shared_ptr<TrigonometryProvider> provider(bool cached) const {
    if (!cached) return std::make_shared<RawTrigonometryProvider>();
    auto p = std::make_shared<CachedTrigonometryProvider>();
    p->update(-lsp.h_hsector, lsp.h_hsector + lsp.h_angle_inc / 2, lsp.h_angle_inc);
    return p;
  }
  HipScanTrig hip_trig(bool cached) const {
    HipScanTrig t;
    if (cached) {
      t.mode = SLAMHIP_TRIG_CACHED;
      t.a_min = -lsp.h_hsector;
      t.a_max = lsp.h_hsector + lsp.h_angle_inc / 2;
      t.a_inc = lsp.h_angle_inc;
    }
    return t;
  }
  TransformedLaserScan scan(const GridMap &gt, const RobotPose &truth, bool cached, bool no_return) const {
    TransformedLaserScan ts;
    ts.scan = LaserScanGenerator{lsp}.laser_scan_2D(gt, truth, 1);
    ts.scan.trig_provider = provider(cached);
    ts.quality = 1.0;
    ts.pose_delta = RobotPoseDelta{0, 0, 0};
    if (no_return) {
      // beams that came back empty: no obstacle, range +inf.  The reference's filter_scan takes the cell of every raw
      // point before it drops the unoccupied ones, and its own assert (regular_squares_grid.h:42) ends the process on a
      // coordinate of +inf: the empty beams are the ones that point into the world's third quadrant (heading 90 .. 102
      // degrees plus 100 .. 135), whose end point is (-inf, -inf)
      auto &pts = ts.scan.points();
      for (size_t i = 0, k = 0; i < pts.size(); ++i)
        if (pts[i].angle() > deg2rad(100) && k++ % 3 == 0)
          pts[i] = ScanPoint2D::make_polar(std::numeric_limits<double>::infinity(), pts[i].angle(), false);
    }
    return ts;
  }
};

// ---------------------------------------------------------------------------------------------------------------------
// the reference's side of one scene: loop map, scan adder, matcher with a counting estimator, and the twin
struct RefSide {
  MapPropertiesProvider props;
  int stride;
  std::shared_ptr<ObservationImpactEstimator> oie;
  std::shared_ptr<GridCell> proto;
  std::unique_ptr<Map> loop, twin;
  std::shared_ptr<GridMapScanAdder> adder;
  std::shared_ptr<GridScanMatcher> matcher;
  std::shared_ptr<CountingSPE> counter;
  std::shared_ptr<Events> events = std::make_shared<Events>();
  double unk[4] = {0, 0, 0, 0};
  double scale;

  // extra: properties set on top of fill_props' (the edge scene's limits and accuracies)
  RefSide(int scene, int variant, int strict, int trig_cache, int w, int h, int ox, int oy, double cell = kScale,
          const std::map<std::string, std::string> &extra = {})
      : stride{scene >= 1 ? 4 : 1}, scale{cell} {
    fill_props(props, scene, variant, strict, trig_cache);
    for (const auto &kv : extra) props.set_property(kv.first, kv.second);
    oie = init_oie(props, false);
    proto = init_occupied_area_model(props);
    payload(stride, *proto, unk);
    loop = fresh(w, h, ox, oy);
    adder = init_scan_adder(props);
    matcher = init_scan_matcher(props);
    counter = std::make_shared<CountingSPE>(matcher->scan_probability_estimator());
    matcher->set_scan_probability_estimator(counter);
    matcher->subscribe(events);
  }

  std::unique_ptr<Map> fresh(int w, int h, int ox, int oy) const {
    auto m = std::make_unique<Map>(oie, proto, GridMapParams{w, h, scale});
    static_cast<UnboundedPlainGridMap &>(*(*m->_map_cache)[0])._origin = DiscretePoint2D{ox, oy};
    m->set_scale_id(m->finest_scale_id());
    return m;
  }
  double impact(const GridCell &c) const { return oie->estimate_obstacle_impact(c); }
  static const GridMap &level(const Map &m, unsigned id) { return *(*m._map_cache)[id]; }

  void append(const RobotPose &pose, const TransformedLaserScan &ts) {
    loop->set_scale_id(loop->finest_scale_id());
    adder->append_scan(*loop, pose, ts.scan, ts.quality, 0);
  }

  // the twin of the loop map as it is now; false: the twin is NOT tight (a harness error)
  bool make_twin(long *known_out = nullptr) {
    const GridMap &fine = level(*loop, 0);
    const auto org = fine.origin();
    twin = fresh(fine.width(), fine.height(), org.x, org.y);
    struct K {
      double impact;
      int x, y;
    };
    std::vector<K> known;
    for (int y = 0; y < fine.height(); ++y)
      for (int x = 0; x < fine.width(); ++x) {
        const GridCell &c = fine[{x - org.x, y - org.y}];
        if (!c.is_unknown()) known.push_back(K{impact(c), x - org.x, y - org.y});
      }
    std::sort(known.begin(), known.end(), [](const K &a, const K &b) {
      if (a.impact != b.impact) return a.impact > b.impact;
      if (a.x != b.x) return a.x < b.x;
      return a.y < b.y;
    });
    for (const K &k : known) twin->reset({k.x, k.y}, fine[{k.x, k.y}]);
    twin->set_scale_id(twin->finest_scale_id());
    if (known_out) *known_out = (long)known.size();
    // validate() with equality (m3rsm_engine.h:37-59)
    const GridMap &tf = level(*twin, 0);
    const unsigned n = twin->scales_nm();
    for (unsigned id = 1; id < n; ++id) {
      const GridMap &cm = level(*twin, id);
      for (int y = 0; y < cm.height(); ++y)
        for (int x = 0; x < cm.width(); ++x) {
          const auto area_id = cm.internal2external({x, y});
          double mx = std::numeric_limits<double>::lowest();
          bool any = false;
          for (auto &a : GridRasterizedRectangle{tf, cm.world_cell_bounds(area_id), false}.to_vector()) {
            if (tf[a].is_unknown()) continue;
            mx = std::max(mx, impact(tf[a]));
            any = true;
          }
          if (!any) mx = impact(*proto);
          if (impact(cm[area_id]) != mx) {
            std::fprintf(stderr, "refm3: twin level %u cell (%d, %d): impact %.17g, fine maximum %.17g\n", id, area_id.x,
                         area_id.y, impact(cm[area_id]), mx);
            return false;
          }
        }
    }
    return true;
  }

  // how far the loop map's coarse cells sit ABOVE the twin's (levels of equal scale, external coordinates)
  double loose_gap() const {
    double gap = 0;
    const unsigned nl = loop->scales_nm(), nt = twin->scales_nm();
    for (unsigned it = 1; it < nt; ++it) {
      const GridMap &t = level(*twin, it);
      for (unsigned il = 1; il < nl; ++il) {
        const GridMap &l = level(*loop, il);
        if (l.scale() != t.scale()) continue;
        for (int y = 0; y < t.height(); ++y)
          for (int x = 0; x < t.width(); ++x) {
            const auto c = t.internal2external({x, y});
            gap = std::max(gap, impact(l[c]) - impact(t[c]));
          }
      }
    }
    return gap;
  }

  double match(const TransformedLaserScan &ts, const RobotPose &pose, RobotPoseDelta &delta, long *calls, bool *events_ok) {
    *events = Events{};
    counter->calls = 0;
    twin->set_scale_id(twin->finest_scale_id());
    const double prob = matcher->process_scan(ts, pose, *twin, delta);
    *calls = counter->calls;
    *events_ok = events->saw(delta, prob);
    return prob;
  }
};

// the trajectory: about 0.15 m and 1 degree per scan; odometry errors inside the matcher's limits
struct Trajectory {
  RobotPose truth0{kScale / 2, kScale / 2 - 6 * kScale, deg2rad(90)};
  RobotPose truth(int k) const {
    RobotPose p = truth0;
    for (int i = 0; i < k; ++i)
      p = off_boundary(RobotPose{p.x + 0.05 * std::cos(0.35 * i), p.y + 0.14, p.theta + deg2rad(1)});
    return off_boundary(p);
  }
  RobotPose odometry(int k) const {
    const RobotPose t = truth(k);
    return RobotPose{t.x + 0.11 * std::sin(1.7 * k), t.y - 0.07 * std::cos(0.9 * k), t.theta + 0.02 * std::sin(0.6 * k + 1)};
  }
};

constexpr int kW0 = 40, kH0 = 30, kOx0 = 12, kOy0 = 11;  // the fine window before the first scan: small, off its centre

// ---------------------------------------------------------------------------------------------------------------------
// the device's side
struct HipSide {
  slamhip_ctx *ctx;
  int map_id, stride, model;
  slamhip_scan_adder_cfg adder{};
  std::unique_ptr<HipM3rsmMap> m3;
  std::shared_ptr<HipGridScanMatcher> gsm;
  std::shared_ptr<Events> events = std::make_shared<Events>();
  double unk[4];
  bool cached;

  // cells: the fine window's payload to start from (row-major, w x h), or null for an empty window
  HipSide(slamhip_ctx *c, const RefSide &ref, int scene, int variant, int trig_cache, int id, int first_level, int w = kW0,
          int h = kH0, int ox = kOx0, int oy = kOy0, const double *cells = nullptr)
      : ctx{c}, map_id{id}, stride{ref.stride}, model{scene >= 1 ? SLAMHIP_CELL_TBM : SLAMHIP_CELL_OCC},
        cached{trig_cache != 0} {
    std::memcpy(unk, ref.unk, sizeof unk);
    slamhip_or_die(slamhip_map_bind(ctx, id, model, w, h, ox, oy, ref.scale, unk), "map_bind");
    slamhip_or_die(slamhip_map_set_auto_grow(ctx, id, 1), "map_set_auto_grow");
    if (cells) slamhip_or_die(slamhip_map_upload_window(ctx, id, 0, 0, w, h, cells), "map_upload_window");
    const Variant va = variant_of(variant);
    adder.rule = scene >= 1 ? SLAMHIP_RULE_TBM : SLAMHIP_RULE_MEAN;
    adder.scan_quality = 1.0;
    adder.base_occupied_prob = 0.95;
    adder.base_occupied_qual = scene >= 1 ? 0.04 : 1.0;
    adder.base_empty_prob = 0.01;
    adder.base_empty_qual = scene >= 1 ? 0.003 : 1.0;
    adder.blur = va.blur;
    adder.max_range = va.max_range;
    adder.occupancy_estimator = 0;
    adder.area_shift_amount = 0;
    m3 = std::make_unique<HipM3rsmMap>(ctx, id, SLAMHIP_OIE_DISCREPANCY, first_level, GridMapParams{w, h, ref.scale}, 0.5, 0);
    gsm = std::dynamic_pointer_cast<HipGridScanMatcher>(init_hip_scan_matcher(ref.props, ctx, 0, -1, nullptr, m3.get()));
    gsm->subscribe(events);
  }
  ~HipSide() {
    gsm.reset();  // (the matcher before the map it matches against)
    m3.reset();
  }

  // 1 = append_scan rebuilt the levels (the window moved), 0 = it refreshed a window of them
  int append(const RobotPose &pose, const TransformedLaserScan &ts, const Scanner &sc) {
    const auto &pts = ts.scan.points();
    const int n = (int)pts.size();
    std::vector<double> r(n), a(n), c(n), s(n);
    std::vector<int> occ(n);
    for (int i = 0; i < n; ++i) {
      r[i] = pts[i].range();
      a[i] = pts[i].angle();
      occ[i] = pts[i].is_occupied() ? 1 : 0;
    }
    int w0, h0, ox0, oy0, w1, h1, ox1, oy1;
    slamhip_or_die(slamhip_map_info(ctx, map_id, nullptr, &w0, &h0, &ox0, &oy0, nullptr, nullptr), "map_info");
    // the scan adder follows the scan's provider, as the reference's does: the table under the cached one, cos / sin of
    // (heading + angle) under the raw one
    if (cached) {
      const HipScanTrig t = sc.hip_trig(true);
      slamhip_or_die(slamhip_beam_trig_cached(n, a.data(), t.a_min, t.a_max, t.a_inc, c.data(), s.data()), "beam_trig_cached");
      m3->append_scan(adder, pose, n, r.data(), c.data(), s.data(), occ.data());
    } else {
      m3->append_scan_raw(adder, pose, n, r.data(), a.data(), occ.data());
    }
    slamhip_or_die(slamhip_map_info(ctx, map_id, nullptr, &w1, &h1, &ox1, &oy1, nullptr, nullptr), "map_info");
    return (w0 != w1 || h0 != h1 || ox0 != ox1 || oy0 != oy1) ? 1 : 0;
  }

  // fine cells that differ from the reference's fine map, payload for payload over the union of the two windows;
  // *view_mis: the same through HipM3rsmMap::map() (occupancy, as a map consumer reads it)
  long fine_mismatches(const GridMap &fine, long *view_mis) {
    int w, h, ox, oy;
    slamhip_or_die(slamhip_map_info(ctx, map_id, nullptr, &w, &h, &ox, &oy, nullptr, nullptr), "map_info");
    std::vector<double> dev((size_t)w * h * stride);
    slamhip_or_die(slamhip_map_download_window(ctx, map_id, 0, 0, w, h, dev.data()), "map_download_window");
    const auto org = fine.origin();
    const int x0 = std::min(-ox, -org.x), y0 = std::min(-oy, -org.y);
    const int x1 = std::max(w - ox, fine.width() - org.x), y1 = std::max(h - oy, fine.height() - org.y);
    long mis = 0;
    *view_mis = 0;
    for (int y = y0; y < y1; ++y)
      for (int x = x0; x < x1; ++x) {
        double a[4], b[4];
        const GridCell &rc = fine[{x, y}];
        payload(stride, rc, a);
        const int ix = x + ox, iy = y + oy;
        if (0 <= ix && ix < w && 0 <= iy && iy < h) std::memcpy(b, &dev[((size_t)iy * w + ix) * stride], stride * sizeof(double));
        else std::memcpy(b, unk, stride * sizeof(double));
        if (std::memcmp(a, b, stride * sizeof(double)) != 0) ++mis;
        const double pa = rc.occupancy().prob_occ, pb = m3->map()[{x, y}].occupancy().prob_occ;
        if (std::memcmp(&pa, &pb, sizeof(double)) != 0) ++*view_mis;
      }
    return mis;
  }

  struct Levels {
    int n = 0;
    std::vector<int> id, w, h, ox, oy;
    std::vector<double> scale;
    std::vector<std::vector<double>> cells;
  };
  Levels download(slamhip_pyramid *pyr) {
    Levels L;
    slamhip_or_die(slamhip_pyramid_info(pyr, &L.n, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "pyramid_info");
    L.id.resize(L.n); L.w.resize(L.n); L.h.resize(L.n); L.ox.resize(L.n); L.oy.resize(L.n); L.scale.resize(L.n);
    slamhip_or_die(slamhip_pyramid_info(pyr, &L.n, L.n, L.id.data(), L.w.data(), L.h.data(), L.ox.data(), L.oy.data(),
                                        L.scale.data()), "pyramid_info");
    L.cells.resize(L.n);
    for (int k = 0; k < L.n; ++k) {
      L.cells[k].resize((size_t)L.w[k] * L.h[k] * stride);
      slamhip_or_die(slamhip_map_download_window(ctx, L.id[k], 0, 0, L.w[k], L.h[k], L.cells[k].data()), "map_download_window");
    }
    return L;
  }

  // the device's levels against the twin's: *geom = levels whose scale differs or whose window is not inside the
  // twin's (the device keeps the tight window around a level's blocks, the reference a centred one that grows by
  // doubling: the same cells, slamhip.h "LEVELS"), *cells = coarse cells that differ, payload for payload, over the union
  void against_twin(const Levels &L, const Map &twin, long *geom, long *cells) {
    *geom = *cells = 0;
    const int nt = (int)twin.scales_nm() - 1;
    for (int k = 0; k < std::min(L.n, nt); ++k) {
      const GridMap &t = RefSide::level(twin, k + 1);
      const auto org = t.origin();
      const bool inside = -L.ox[k] >= -org.x && -L.oy[k] >= -org.y && L.w[k] - L.ox[k] <= t.width() - org.x &&
                          L.h[k] - L.oy[k] <= t.height() - org.y;
      // (the last level is one cell of infinite scale holding external (0, 0): it is inside any window)
      const double t_scale = t.scale();
      if (std::memcmp(&L.scale[k], &t_scale, sizeof(double)) != 0 || (!inside && k + 1 < L.n)) ++*geom;
      const int x0 = std::min(-L.ox[k], -org.x), y0 = std::min(-L.oy[k], -org.y);
      const int x1 = std::max(L.w[k] - L.ox[k], t.width() - org.x), y1 = std::max(L.h[k] - L.oy[k], t.height() - org.y);
      for (int y = y0; y < y1; ++y)
        for (int x = x0; x < x1; ++x) {
          double a[4], b[4];
          payload(stride, t[{x, y}], a);
          const int ix = x + L.ox[k], iy = y + L.oy[k];
          if (0 <= ix && ix < L.w[k] && 0 <= iy && iy < L.h[k])
            std::memcpy(b, &L.cells[k][((size_t)iy * L.w[k] + ix) * stride], stride * sizeof(double));
          else std::memcpy(b, unk, stride * sizeof(double));
          if (std::memcmp(a, b, stride * sizeof(double)) != 0) ++*cells;
        }
    }
  }

  // ... and against a second pyramid created on the same fine map just now: geometry and payload, bit for bit
  long against_fresh(const Levels &L) {
    slamhip_pyramid *p2 = nullptr;
    slamhip_or_die(slamhip_pyramid_create(ctx, map_id, SLAMHIP_OIE_DISCREPANCY, kFreshLevelId, &p2), "pyramid_create");
    const Levels F = download(p2);
    slamhip_or_die(slamhip_pyramid_destroy(p2), "pyramid_destroy");
    if (F.n != L.n) return 1000000;
    long mis = 0;
    for (int k = 0; k < L.n; ++k) {
      if (F.w[k] != L.w[k] || F.h[k] != L.h[k] || F.ox[k] != L.ox[k] || F.oy[k] != L.oy[k] ||
          std::memcmp(&F.scale[k], &L.scale[k], sizeof(double)) != 0) {
        mis += 1000000;
        continue;
      }
      for (size_t i = 0; i < L.cells[k].size(); i += stride)
        if (std::memcmp(&F.cells[k][i], &L.cells[k][i], stride * sizeof(double)) != 0) ++mis;
    }
    return mis;
  }

  double match(const TransformedLaserScan &ts, const RobotPose &pose, RobotPoseDelta &delta, long long *calls, bool *events_ok) {
    *events = Events{};
    const double prob = gsm->process_scan(ts, pose, m3->map(), delta);
    long long pe = 0, la = 0;
    slamhip_or_die(slamhip_matcher_stats(gsm->_m, calls, &pe, &la), "matcher_stats");
    *events_ok = events->saw(delta, prob);
    return prob;
  }
};


// ---------------------------------------------------------------------------------------------------------------------
// The EDGE scene: what tells the raw provider from the cached one.  33 x 33 cells of 1/8 m, every cell known with a value
// of its own, the robot on a cell centre, ranges odd multiples of 1/16, angles, heading and rotation step multiples of
// 1/64: for seventeen beam angles (heading + rotation) + angle is exactly 0 at one rotation each, cos / sin of it exactly
// (1, 0) under the raw provider, the end point exactly ON a cell edge -- while the cached provider's
// cos t cos a - sin t sin a falls an ulp short of 1 for some of them, into the neighbouring cell.
struct EdgeScene {
  static constexpr int kN = 33, kO = 16;
  static constexpr double kCell = 0.125;
  RobotPose pose{kCell / 2, kCell / 2, 0.5};
  std::map<std::string, std::string> props() const {
    return {{"slam/scmtch/BF_M3RSM/limits/x_translation", "0.125"},
            {"slam/scmtch/BF_M3RSM/limits/y_translation", "0.0625"},
            {"slam/scmtch/BF_M3RSM/limits/rotation", num(8.0 / 64)},
            {"slam/scmtch/BF_M3RSM/accuracy/rotation", num(1.0 / 64)},
            {"slam/scmtch/BF_M3RSM/accuracy/translation", "0.0625"}};
  }
  TransformedLaserScan scan(bool cached) const {
    TransformedLaserScan ts;
    ts.quality = 1.0;
    ts.pose_delta = RobotPoseDelta{0, 0, 0};
    const double a_min = -48.0 / 64, a_inc = 1.0 / 64;
    // (every sum exact: the provider's table holds these angles; four points per angle, one per binade of the range)
    for (double a = a_min; a <= 16.0 / 64; a += a_inc)
      for (double r : {5 / 16.0, 11 / 16.0, 19 / 16.0, 27 / 16.0}) ts.scan.points().push_back(ScanPoint2D::make_polar(r, a, true));
    if (cached) {
      auto p = std::make_shared<CachedTrigonometryProvider>();
      p->update(a_min, 16.0 / 64 + a_inc / 2, a_inc);
      ts.scan.trig_provider = p;
    } else {
      ts.scan.trig_provider = std::make_shared<RawTrigonometryProvider>();
    }
    return ts;
  }
  // every cell written once, with a value of its own in (0.05, 0.95)
  void fill(RefSide &ref) const {
    ref.loop->set_scale_id(0);
    for (int y = 0; y < kN; ++y)
      for (int x = 0; x < kN; ++x) {
        const unsigned hsh = (unsigned)(y * kN + x + 1) * 2654435761u;
        const double p = 0.05 + 0.9 * ((hsh >> 8) & 0xffff) / 65536.0;
        ref.loop->update({x - kO, y - kO}, AreaOccupancyObservation{true, Occupancy{p, 1.0}, Point2D{0, 0}, 1.0});
      }
  }
};
constexpr int EdgeScene::kN, EdgeScene::kO;
constexpr double EdgeScene::kCell;

// one run over n_steps scans; hip == nullptr: the reference alone.  rows: n_steps x kRow
//  0 fine cells that differ            1 branch (1 rebuild, 0 refresh)      2 device levels      3 twin levels
//  4 level geometry mismatches         5 level cells that differ (twin)     6 ... (fresh pyramid)
//  7-9 reference delta, 10 probability 11-13 device delta, 14 probability   15, 16 scorer calls (reference, device)
// 17, 18 observer events as expected (reference, device)                    19 loop map's coarse impact above the twin's (max)
// 20 the reference's match is valid    21 known fine cells                  22 fine cells that differ through map()
// 23 the reference's fine window grew at this step
int run_loop(int scene, int variant, int strict, int trig_cache, int n_steps, bool with_hip, double *rows) {
  std::memset(rows, 0, sizeof(double) * kRow * n_steps);
  const auto gt = make_room();
  const Scanner sc;
  const Trajectory tr;
  const Variant va = variant_of(variant);
  RefSide ref(scene, variant, strict, trig_cache, kW0, kH0, kOx0, kOy0);
  slamhip_ctx *ctx = nullptr;
  std::unique_ptr<HipSide> hip;
  if (with_hip) {
    if (slamhip_ctx_create(0, &ctx) != SLAMHIP_OK) {
      std::cerr << "refm3: " << slamhip_last_error() << std::endl;
      return -1;
    }
    hip = std::make_unique<HipSide>(ctx, ref, scene, variant, trig_cache, 0, 1);
  }
  int rc = 0;
  RobotPose pose = tr.truth(0);
  for (int k = 0; k < n_steps; ++k) {
    double *row = rows + (size_t)kRow * k;
    const TransformedLaserScan ts = sc.scan(*gt, tr.truth(k), trig_cache != 0, va.no_return);
    // 1. the fine map
    const GridMap &fine = RefSide::level(*ref.loop, 0);
    const int rw = fine.width(), rh = fine.height();
    const auto rorg = fine.origin();
    ref.append(pose, ts);
    row[23] = (fine.width() != rw || fine.height() != rh || !(fine.origin() == rorg)) ? 1 : 0;
    if (hip) {
      row[1] = hip->append(pose, ts, sc);
      long view_mis = 0;
      row[0] = (double)hip->fine_mismatches(fine, &view_mis);
      row[22] = (double)view_mis;
    } else {
      row[1] = row[23];
    }
    // 2. the tight twin
    long known = 0;
    if (!ref.make_twin(&known)) {
      rc = 2;
      break;
    }
    row[21] = (double)known;
    row[3] = (double)ref.twin->scales_nm() - 1;
    row[19] = ref.loose_gap();
    // 3. the levels
    if (hip) {
      const HipSide::Levels L = hip->download(hip->m3->pyramid());
      long geom = 0, cells = 0;
      hip->against_twin(L, *ref.twin, &geom, &cells);
      row[2] = L.n;
      row[4] = (double)geom;
      row[5] = (double)cells;
      row[6] = (double)hip->against_fresh(L);
    }
    // 4. the next scan, matched through the two factories
    const TransformedLaserScan next = sc.scan(*gt, tr.truth(k + 1), trig_cache != 0, va.no_return);
    const RobotPose init = tr.odometry(k + 1);
    RobotPoseDelta dr{0, 0, 0}, dh{0, 0, 0};
    long ref_calls = 0;
    bool ev_ref = false, ev_hip = false;
    const double pr = ref.match(next, init, dr, &ref_calls, &ev_ref);
    row[7] = dr.x; row[8] = dr.y; row[9] = dr.theta; row[10] = pr;
    row[15] = (double)ref_calls;
    row[17] = ev_ref ? 1 : 0;
    row[20] = std::isnan(pr) ? 0 : 1;
    if (hip) {
      long long hip_calls = 0;
      const double ph = hip->match(next, init, dh, &hip_calls, &ev_hip);
      row[11] = dh.x; row[12] = dh.y; row[13] = dh.theta; row[14] = ph;
      row[16] = (double)hip_calls;
      row[18] = ev_hip ? 1 : 0;
    }
    // the reference's correction drives both maps' next update
    pose = RobotPose{init.x + dr.x, init.y + dr.y, init.theta + dr.theta};
  }
  hip.reset();
  if (ctx) slamhip_ctx_destroy(ctx);
  return rc;
}

}  // namespace

extern "C" {

int refm3_row_doubles() { return kRow; }

// scene 0 OCC / 1 TBM, variant 0..3 (see Variant), strict 0 / 1, trig_cache 0 / 1; rows: n_steps x refm3_row_doubles().
// 0 = ran; 2 = the twin was not tight (a harness error, nothing was compared with it); -1 = no device
int refm3_loop(int scene, int variant, int strict, int trig_cache, int n_steps, double *rows) {
  return run_loop(scene, variant, strict, trig_cache, n_steps, true, rows);
}

// the same loop on the reference alone (the raw provider, as the default mode runs it)
int refm3_reference_selfcheck(int scene, int variant, int n_steps, double *rows) {
  return run_loop(scene, variant, 1, 0, n_steps, false, rows);
}

// The request surface.  Two maps of one cell model on one context (map A: the loop's trajectory, map B: the same room
// entered 0.6 m further on and turned by 20 degrees), each fed n_scans scans at their true poses; three requests -- two on
// map A from different poses, one on map B.
// out (34 doubles):
//  0 winner (device)  1 winner (reference)  2-4 delta (device)  5 prob (device)  6-8 delta (reference)  9 prob (reference)
// 10 + 4 r .. : match_each of request r = delta, prob      22 + 4 r .. : the lone process_scan of request r through the factory's matcher
// 0 = ran; 2 = a twin was not tight; 3 = the raw provider's request slot came without its angles (SLAMHIP_ERR_STATE);
// 4 = the reference's engine found no match; -1 = no device
int refm3_engine(int scene, int strict, int trig_cache, int n_scans, double *out) {
  std::memset(out, 0, sizeof(double) * 34);
  const auto gt = make_room();
  const Scanner sc;
  Trajectory ta, tb;
  tb.truth0 = off_boundary(RobotPose{ta.truth0.x + 0.3, ta.truth0.y + 0.6, ta.truth0.theta + deg2rad(20)});
  RefSide ra(scene, 0, strict, trig_cache, kW0, kH0, kOx0, kOy0), rb(scene, 0, strict, trig_cache, kW0, kH0, kOx0, kOy0);
  slamhip_ctx *ctx = nullptr;
  if (slamhip_ctx_create(0, &ctx) != SLAMHIP_OK) {
    std::cerr << "refm3: " << slamhip_last_error() << std::endl;
    return -1;
  }
  int rc = 0;
  {
    HipSide ha(ctx, ra, scene, 0, trig_cache, 0, 1), hb(ctx, rb, scene, 0, trig_cache, 20, 21);
    for (int k = 0; k < n_scans; ++k) {
      const auto sa = sc.scan(*gt, ta.truth(k), trig_cache != 0, false), sb = sc.scan(*gt, tb.truth(k), trig_cache != 0, false);
      ra.append(ta.truth(k), sa);
      rb.append(tb.truth(k), sb);
      ha.append(ta.truth(k), sa, sc);
      hb.append(tb.truth(k), sb, sc);
    }
    if (!ra.make_twin() || !rb.make_twin()) rc = 2;
    if (rc == 0) {
      struct Req {
        RobotPose pose;
        TransformedLaserScan ts;
        RefSide *ref;
        HipSide *hip;
      };
      std::vector<Req> reqs;
      reqs.push_back(Req{ta.odometry(n_scans), sc.scan(*gt, ta.truth(n_scans), trig_cache != 0, false), &ra, &ha});
      reqs.push_back(Req{ta.odometry(n_scans - 1), sc.scan(*gt, ta.truth(n_scans - 1), trig_cache != 0, false), &ra, &ha});
      reqs.push_back(Req{tb.odometry(n_scans), sc.scan(*gt, tb.truth(n_scans), trig_cache != 0, false), &rb, &hb});
      // the library matcher the engine runs on: HipM3rsmMap::matcher with the configuration the factory derives
      slamhip_spe_cfg cfg{};
      cfg.oope = SLAMHIP_OOPE_MAX;
      cfg.oie = SLAMHIP_OIE_DISCREPANCY;
      cfg.sum_order = strict ? SLAMHIP_SUM_SEQUENTIAL : SLAMHIP_SUM_TREE256;
      cfg.pose_trig = !strict ? SLAMHIP_POSE_TRIG_DEVICE : (trig_cache ? SLAMHIP_POSE_TRIG_HOST : SLAMHIP_POSE_TRIG_RAW_EXACT);
      slamhip_matcher *m = ha.m3->matcher(cfg, 0.3, 0.2, deg2rad(3), deg2rad(1), 0.05);
      auto spe = init_spe(ra.props);
      const int first_slot = 7;
      HipM3rsmEngine engine(ctx, m, spe, scene == 1 ? 1 : 0, sc.hip_trig(trig_cache != 0), first_slot,
                            scene == 1 ? std::make_shared<VinySlamSPW>() : std::shared_ptr<ScanPointWeighting>());
      int slots_per_request = 1;  // (viny: one scan per rotation of the root layer, hip_store_rotation_scans)
      if (scene == 1) slamhip_or_die(slamhip_matcher_m3rsm_rotations(m, 0, nullptr, &slots_per_request), "m3rsm_rotations");
      engine.reset_engine_state();
      for (size_t r = 0; r < reqs.size() && rc == 0; ++r) {
        engine.add_scan_matching_request(reqs[r].pose, reqs[r].ts.scan, *reqs[r].hip->m3);
        if (cfg.pose_trig == SLAMHIP_POSE_TRIG_RAW_EXACT) {
          // the slot must have got its angles: one bound on the request answers, instead of SLAMHIP_ERR_STATE
          slamhip_m3rsm_request q;
          q.pyramid = reqs[r].hip->m3->pyramid();
          q.scan_slot = first_slot + (int)r * slots_per_request;
          q.init_pose[0] = reqs[r].pose.x; q.init_pose[1] = reqs[r].pose.y; q.init_pose[2] = reqs[r].pose.theta;
          const int which = 0;
          const double rot = 0, rect[4] = {0, 0, 0, 0};
          double score = 0;
          int lvl = 0;
          const int e = slamhip_pyramid_score_requests(ctx, &cfg, 1, &q, 1, &which, &rot, rect, &score, &lvl);
          if (e == SLAMHIP_ERR_STATE) rc = 3;
          else slamhip_or_die(e, "pyramid_score_requests");
        }
      }
      if (rc == 0) {
        const auto best = engine.best_match();
        out[0] = best.request;
        out[2] = best.pose_delta.x; out[3] = best.pose_delta.y; out[4] = best.pose_delta.theta; out[5] = best.prob_upper_bound;
        const auto each = engine.match_each();
        for (size_t r = 0; r < reqs.size(); ++r) {
          out[10 + 4 * r] = each[r].pose_delta.x; out[11 + 4 * r] = each[r].pose_delta.y;
          out[12 + 4 * r] = each[r].pose_delta.theta; out[13 + 4 * r] = each[r].prob_upper_bound;
        }
        // the lone calls through the adapter matcher the factory made
        for (size_t r = 0; r < reqs.size(); ++r) {
          RobotPoseDelta d{0, 0, 0};
          long long calls = 0;
          bool ev = false;
          const double p = reqs[r].hip->match(reqs[r].ts, reqs[r].pose, d, &calls, &ev);
          out[22 + 4 * r] = d.x; out[23 + 4 * r] = d.y; out[24 + 4 * r] = d.theta; out[25 + 4 * r] = p;
        }
        // the reference's engine under the matcher's own loop (bf_multi_res_scan_matcher.h:32-65), three requests
        M3RSMEngine ref_engine;
        ref_engine.reset_engine_state();
        ref_engine.set_translation_lookup_range(0.3, 0.2);
        ref_engine.set_rotation_lookup_range(2 * deg2rad(3), deg2rad(1));
        ra.twin->set_scale_id(0);
        rb.twin->set_scale_id(0);
        SafeRescalableMap safe_a{*ra.twin}, safe_b{*rb.twin};
        auto ref_spe = init_spe(ra.props);
        for (auto &q : reqs) ref_engine.add_scan_matching_request(ref_spe, q.pose, q.ts.scan, q.ref == &ra ? (GridMap &)safe_a : (GridMap &)safe_b, true);
        out[1] = -1;
        while (1) {
          auto bm = ref_engine.next_best_match(0.05);
          if (!bm.is_valid()) {
            rc = 4;
            break;
          }
          if (bm.is_finest()) {
            for (size_t r = 0; r < reqs.size(); ++r)
              if (bm.pose == &reqs[r].pose) out[1] = (double)r;
            const Point2D c = bm.translation_drift.center();
            out[6] = c.x; out[7] = c.y; out[8] = bm.rotation; out[9] = bm.prob_upper_bound;
            break;
          }
          auto pts = bm.translation_drift.corners();
          pts.push_back(bm.translation_drift.center());
          for (const auto &cp : pts) ref_engine.add_match(Match{M3RSMEngine::Rect{cp}, bm});
        }
      }
      slamhip_matcher_destroy(m);
    }
  }
  slamhip_ctx_destroy(ctx);
  return rc;
}


// The edge scene through the two factories under strict mode.  with_hip = 0: the reference alone (no device call).
// out (16 doubles): 0-2 delta, 3 prob, 4 calls, 5 events as expected (reference); 6-11 the same of the device
// 0 = ran; 2 = the twin was not tight; -1 = no device
int refm3_edge(int trig_cache, int with_hip, double *out) {
  std::memset(out, 0, sizeof(double) * 16);
  const EdgeScene e;
  RefSide ref(0, 0, 1, trig_cache, EdgeScene::kN, EdgeScene::kN, EdgeScene::kO, EdgeScene::kO, EdgeScene::kCell, e.props());
  e.fill(ref);
  if (!ref.make_twin()) return 2;
  const TransformedLaserScan ts = e.scan(trig_cache != 0);
  RobotPoseDelta d{0, 0, 0};
  long calls = 0;
  bool ev = false;
  const double p = ref.match(ts, e.pose, d, &calls, &ev);
  out[0] = d.x; out[1] = d.y; out[2] = d.theta; out[3] = p; out[4] = (double)calls; out[5] = ev ? 1 : 0;
  if (!with_hip) return 0;
  slamhip_ctx *ctx = nullptr;
  if (slamhip_ctx_create(0, &ctx) != SLAMHIP_OK) {
    std::cerr << "refm3: " << slamhip_last_error() << std::endl;
    return -1;
  }
  {
    const GridMap &fine = RefSide::level(*ref.loop, 0);
    std::vector<double> cells((size_t)EdgeScene::kN * EdgeScene::kN);
    for (int y = 0; y < EdgeScene::kN; ++y)
      for (int x = 0; x < EdgeScene::kN; ++x)
        cells[(size_t)y * EdgeScene::kN + x] = fine[{x - EdgeScene::kO, y - EdgeScene::kO}].occupancy().prob_occ;
    HipSide hip(ctx, ref, 0, 0, trig_cache, 0, 1, EdgeScene::kN, EdgeScene::kN, EdgeScene::kO, EdgeScene::kO, cells.data());
    RobotPoseDelta dh{0, 0, 0};
    long long hip_calls = 0;
    bool evh = false;
    const double ph = hip.match(ts, e.pose, dh, &hip_calls, &evh);
    out[6] = dh.x; out[7] = dh.y; out[8] = dh.theta; out[9] = ph; out[10] = (double)hip_calls; out[11] = evh ? 1 : 0;
  }
  slamhip_ctx_destroy(ctx);
  return 0;
}

}  // extern "C"
