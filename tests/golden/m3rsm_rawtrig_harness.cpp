// tests/golden/m3rsm_rawtrig_harness.cpp -- TEST INFRASTRUCTURE ONLY (golden data for tests/golden/m3rsm_rawtrig.npz).
//
// m3rsm_harness.cpp with ONE difference: the scan's trig provider is the reference's default, RawTrigonometryProvider
// (src/core/trigonometry_utils.h:17-35; use_trig_cache = false), which evaluates std::cos / std::sin(base + a) per beam.
// A small program around the UNMODIFIED reference headers (slam_constructor's src/, given with -I): the reference's own
// BruteForceMultiResolutionScanMatcher::process_scan over M3RSMRescalableGridMap<UnboundedPlainGridMap> with a recording
// ScanProbabilityEstimator, every scorer call written down in call order.  Per scene three runs:
//   A  the matcher itself under the raw provider (the engine runs with prerotate_scan = true): result and trace;
//   B  the reference's M3RSMEngine driven by the matcher's loop with prerotate_scan = false on the same polar scan;
//   D  run A once more by this same binary with the scan under CachedTrigonometryProvider: what the raw provider's
//      trace is told apart from.
// tests/golden/make_golden_m3rsm_rawtrig.py compiles it (g++ -std=c++14 -O3, the reference's own flags), feeds it one
// file of doubles and packs what it writes; the binary is never committed and nothing in the product path knows about it.
//
//   m3rsm_rawtrig_harness <input.bin> <output.bin>
//
// Input and output are flat arrays of doubles in the order read / written below.  Access control is relaxed only so
// that the fine map's origin can be moved off its centre.
#include <algorithm>
#include <cassert>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <iterator>
#include <limits>
#include <map>
#include <memory>
#include <queue>
#include <set>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

#define private public
#define protected public
#include "core/maps/plain_grid_map.h"
#include "core/maps/grid_cell.h"
#include "core/maps/tbm_grid_cells.h"
#include "slams/credibilist/grid_cell.h"
#include "core/scan_matchers/observation_impact_estimators.h"
#include "core/scan_matchers/occupancy_observation_probability.h"
#include "core/scan_matchers/weighted_mean_point_probability_spe.h"
#include "core/scan_matchers/m3rsm_engine.h"
#include "core/scan_matchers/bf_multi_res_scan_matcher.h"
#undef private
#undef protected

namespace {

std::vector<double> in_buf, out_buf;
size_t in_pos = 0;
double rd() {
  if (in_pos >= in_buf.size()) {
    std::fprintf(stderr, "m3rsm_rawtrig_harness: input too short\n");
    std::exit(2);
  }
  return in_buf[in_pos++];
}
int rdi() { return (int)rd(); }
void wr(double v) { out_buf.push_back(v); }

enum { GRID_CELL = 0, TBM_CONSISTENT = 1, CREDIBILIST = 2 };

std::shared_ptr<GridCell> prototype(int cls) {
  switch (cls) {
    case GRID_CELL: return std::make_shared<GridCell>(Occupancy{0.5, 1});
    case TBM_CONSISTENT: return std::make_shared<TbmOccConsistentCell>();
    default: return std::make_shared<CredibilistCell>();
  }
}

void write_payload(int cls, const GridCell &c) {
  if (cls == GRID_CELL) {
    wr(c.occupancy().prob_occ);
    return;
  }
  const TBM &t = cls == CREDIBILIST ? static_cast<const CredibilistCell &>(c).belief()
                                    : static_cast<const TbmBaseCell &>(c).belief();
  wr(t.unknown());
  wr(t.empty());
  wr(t.occupied());
  wr(t.conflict());
}

using Map = M3RSMRescalableGridMap<UnboundedPlainGridMap>;
using Rect = M3RSMEngine::Rect;

// one scorer call: what was asked and what came back; (px, py) = the first point of the scan it was asked about, which
// tells the prerotated scans of run A apart
struct Record {
  RobotPose pose;
  LightWeightRectangle area;
  double value;
  int scale_id;
  double px, py;
};

// A ScanProbabilityEstimator of our own that hands every call to the reference's estimator and writes it down
class RecordingSPE : public ScanProbabilityEstimator {
public:
  RecordingSPE(std::shared_ptr<ScanProbabilityEstimator> real, OOPE oope) : ScanProbabilityEstimator{oope}, _real{real} {}
  LaserScan2D filter_scan(const LaserScan2D &scan, const RobotPose &pose, const GridMap &map) override {
    filtered = _real->filter_scan(scan, pose, map);
    return filtered;
  }
  double estimate_scan_probability(const LaserScan2D &scan, const RobotPose &pose, const GridMap &map,
                                   const SPEParams &params) const override {
    const double v = _real->estimate_scan_probability(scan, pose, map, params);
    const auto &pts = scan.points();
    const bool cart = !pts.empty() && pts[0]._type == ScanPoint2D::PointType::Cartesian;
    log.push_back(Record{pose, params.sp_analysis_area, v, (int)dynamic_cast<const Map &>(map).scale_id(),
                         cart ? pts[0].x() : 0.0, cart ? pts[0].y() : 0.0});
    return v;
  }
  mutable std::vector<Record> log;
  LaserScan2D filtered;

private:
  std::shared_ptr<ScanProbabilityEstimator> _real;
};

void write_records(const std::vector<Record> &log) {
  wr((double)log.size());
  for (const Record &c : log) {
    wr(c.pose.x);
    wr(c.pose.y);
    wr(c.pose.theta);
    wr(c.area.bot());
    wr(c.area.top());
    wr(c.area.left());
    wr(c.area.right());
    wr(c.value);
    wr(c.scale_id);
    wr(c.px);
    wr(c.py);
  }
}

}  // namespace

int main(int argc, char **argv) {
  if (argc != 3) return 1;
  {
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 1;
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    in_buf.resize(bytes / sizeof(double));
    if (std::fread(in_buf.data(), sizeof(double), in_buf.size(), f) != in_buf.size()) return 1;
    std::fclose(f);
  }
  const int n_scenes = rdi();
  for (int k = 0; k < n_scenes; ++k) {
    const int cls = rdi(), oie_kind = rdi();
    const int w = rdi(), h = rdi();
    const double scale = rd();
    const int ox = rdi(), oy = rdi();
    std::shared_ptr<ObservationImpactEstimator> oie;
    if (oie_kind == 0) oie = std::make_shared<DiscrepancyOIE>();
    else oie = std::make_shared<OccupancyOIE>();
    Map map(oie, prototype(cls), GridMapParams{w, h, scale});
    // the finest map's origin, before anything is written
    static_cast<UnboundedPlainGridMap &>(*(*map._map_cache)[0])._origin = DiscretePoint2D{ox, oy};
    map.set_scale_id(map.finest_scale_id());
    const int n_obs = rdi();
    for (int i = 0; i < n_obs; ++i) {
      const int x = rdi(), y = rdi();
      const bool is_occ = rd() != 0.0;
      const double prob = rd(), est_quality = rd(), quality = rd();
      map.update({x, y}, AreaOccupancyObservation{is_occ, Occupancy{prob, est_quality}, Point2D{0, 0}, quality});
    }
    // ---- every level: geometry, then per cell (internal order, y ascending) payload, is_unknown, impact ----
    const unsigned n_scales = map.scales_nm();
    wr(n_scales);
    wr(map.validate() ? 1 : 0);
    write_payload(cls, *map.cell_prototype());
    for (unsigned id = 0; id < n_scales; ++id) {
      map.set_scale_id(id);
      const int lw = map.width(), lh = map.height();
      const DiscretePoint2D o = map.origin();
      wr(lw);
      wr(lh);
      wr(o.x);
      wr(o.y);
      wr(map.scale());
      for (int y = 0; y < lh; ++y)
        for (int x = 0; x < lw; ++x) {
          const GridCell &c = map[{x - o.x, y - o.y}];
          write_payload(cls, c);
          wr(c.is_unknown() ? 1 : 0);
          wr(oie->estimate_obstacle_impact(c));
        }
    }
    map.set_scale_id(map.finest_scale_id());
    // ---- the match ----
    const RobotPose pose{rd(), rd(), rd()};
    const int n = rdi();
    TransformedLaserScan tscan;
    tscan.quality = 1.0;
    std::vector<double> ranges(n), angles(n);
    for (double &v : ranges) v = rd();
    for (double &v : angles) v = rd();
    const double a_min = rd(), a_max = rd(), a_inc = rd();
    for (int i = 0; i < n; ++i) tscan.scan.points().emplace_back(ranges[i], angles[i], true);
    tscan.scan.trig_provider = std::make_shared<RawTrigonometryProvider>();
    const double max_x = rd(), max_y = rd(), max_th = rd(), rot_step = rd(), trl_step = rd();
    auto oope = std::make_shared<MaxOccupancyObservationPE>(oie);
    auto spw = std::make_shared<EvenSPW>();
    auto real = std::make_shared<WeightedMeanPointProbabilitySPE>(oope, spw, 0, std::numeric_limits<double>::infinity());
    auto spe = std::make_shared<RecordingSPE>(real, oope);
    // run A: the reference's matcher, the scan under the raw provider
    {
      BruteForceMultiResolutionScanMatcher matcher(spe, max_x, max_y, max_th, rot_step, trl_step);
      RobotPoseDelta delta;
      const double prob = matcher.process_scan(tscan, pose, map, delta);
      // the scan as the device takes it -- what filter_scan kept --: range, cos a, sin a (libm's, as the raw provider has
      // them at base angle 0), weight, factor, and the point's angle
      const auto &pts = spe->filtered.points();
      wr((double)pts.size());
      for (size_t i = 0; i < pts.size(); ++i) {
        wr(pts[i].range());
        wr(std::cos(pts[i].angle()));
        wr(std::sin(pts[i].angle()));
        wr(spw->weight(pts, i));
        wr(pts[i].factor());
        wr(pts[i].angle());
      }
      wr(delta.x);
      wr(delta.y);
      wr(delta.theta);
      wr(prob);
      write_records(spe->log);
    }
    // run B: the reference's engine, not prerotated, under the matcher's own loop
    {
      spe->log.clear();
      map.set_scale_id(map.finest_scale_id());
      M3RSMEngine engine;
      engine.reset_engine_state();
      engine.set_translation_lookup_range(max_x, max_y);
      engine.set_rotation_lookup_range(2 * max_th, rot_step);
      SafeRescalableMap rescalable_map{map};
      engine.add_scan_matching_request(spe, pose, tscan.scan, rescalable_map, false);
      RobotPoseDelta delta;
      double prob = 0;
      while (1) {
        auto best_match = engine.next_best_match(trl_step);
        if (!best_match.is_valid()) return 3;
        if (best_match.is_finest()) {
          delta = {best_match.translation_drift.center(), best_match.rotation};
          prob = best_match.prob_upper_bound;
          break;
        }
        auto crucial_points = best_match.translation_drift.corners();
        crucial_points.push_back(best_match.translation_drift.center());
        for (const auto &cp : crucial_points) engine.add_match(Match{M3RSMEngine::Rect{cp}, best_match});
      }
      wr(delta.x);
      wr(delta.y);
      wr(delta.theta);
      wr(prob);
      write_records(spe->log);
    }
    // run D: run A with the scan under the cached provider
    {
      spe->log.clear();
      map.set_scale_id(map.finest_scale_id());
      auto trig = std::make_shared<CachedTrigonometryProvider>();
      trig->update(a_min, a_max, a_inc);
      tscan.scan.trig_provider = trig;
      BruteForceMultiResolutionScanMatcher matcher(spe, max_x, max_y, max_th, rot_step, trl_step);
      RobotPoseDelta delta;
      const double prob = matcher.process_scan(tscan, pose, map, delta);
      wr(delta.x);
      wr(delta.y);
      wr(delta.theta);
      wr(prob);
      write_records(spe->log);
    }
    map.set_scale_id(map.finest_scale_id());
  }
  FILE *f = std::fopen(argv[2], "wb");
  if (!f) return 1;
  std::fwrite(out_buf.data(), sizeof(double), out_buf.size(), f);
  std::fclose(f);
  return 0;
}
