// tests/golden/pyramid_harness.cpp -- TEST INFRASTRUCTURE ONLY (golden data for tests/golden/pyramid.npz).
//
// A small program around the UNMODIFIED reference headers (slam_constructor's src/, given with -I):
// M3RSMRescalableGridMap<UnboundedPlainGridMap> (core/scan_matchers/m3rsm_engine.h) filled through GridMap::update, every
// level read back, validate(); and the reference's own M3RSMEngine (the same header) run over it with a recording
// ScanProbabilityEstimator: add_scan_matching_request makes the root layer, next_best_match branches (split4_evenly /
// split_horz / split_vert), and every scorer call -- pose, sp_analysis_area, the map's scale_id, the value -- is written
// down in call order.
// tests/golden/make_golden_pyramid.py compiles it (g++ -std=c++14 -O3, the reference's own flags), feeds it one file of
// doubles and packs what it writes; the binary is never committed and nothing in the product path knows about it.
//
//   pyramid_harness <input.bin> <output.bin>
//
// Input and output are flat arrays of doubles in the order read / written below.  Access control is relaxed only so
// that the fine map's origin can be moved off its centre and the cached trig provider's table can be read.
#include <algorithm>
#include <cassert>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <iterator>
#include <limits>
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
#undef private
#undef protected

namespace {

std::vector<double> in_buf, out_buf;
size_t in_pos = 0;
double rd() {
  if (in_pos >= in_buf.size()) {
    std::fprintf(stderr, "pyramid_harness: input too short\n");
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

// one scorer call of the engine: what it asked and what it got
struct Record {
  RobotPose pose;
  LightWeightRectangle area;
  double value;
  int scale_id;
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
    log.push_back(Record{pose, params.sp_analysis_area, v, (int)dynamic_cast<const Map &>(map).scale_id()});
    return v;
  }
  mutable std::vector<Record> log;
  LaserScan2D filtered;

private:
  std::shared_ptr<ScanProbabilityEstimator> _real;
};

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
  const int n_maps = rdi();
  for (int k = 0; k < n_maps; ++k) {
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
    // ---- matches ----
    const int n_sets = rdi();
    for (int s = 0; s < n_sets; ++s) {
      const RobotPose pose{rd(), rd(), rd()};
      const int n = rdi();
      auto raw_scan = std::make_shared<LaserScan2D>();
      std::vector<double> ranges(n), angles(n);
      for (double &v : ranges) v = rd();
      for (double &v : angles) v = rd();
      const double a_min = rd(), a_max = rd(), a_inc = rd();
      for (int i = 0; i < n; ++i) raw_scan->points().emplace_back(ranges[i], angles[i], true);
      auto trig = std::make_shared<CachedTrigonometryProvider>();
      trig->update(a_min, a_max, a_inc);
      raw_scan->trig_provider = trig;
      const double sector = rd(), rot_step = rd(), trl_step = rd();
      auto oope = std::make_shared<MaxOccupancyObservationPE>(oie);
      auto spw = std::make_shared<EvenSPW>();
      auto real = std::make_shared<WeightedMeanPointProbabilitySPE>(oope, spw, 0, std::numeric_limits<double>::infinity());
      auto spe = std::make_shared<RecordingSPE>(real, oope);
      // runs of the reference's own engine, every scorer call it makes recorded in call order: the root layer by
      // M3RSMEngine::add_scan_matching_request, then the branches of M3RSMEngine::next_best_match, called until `cap` records lie behind the root layer.  The generator
      // gives run 0 the square translation range (split4_evenly all the way down) and two more runs ranges twice as wide
      // as high and twice as high as wide, whose last branch is one-sided (split_horz / split_vert).  At most `cap`
      // records behind the root layer are kept per run.
      const int n_runs = rdi();
      wr(n_runs);
      bool scan_written = false;
      for (int r = 0; r < n_runs; ++r) {
        const double max_x = rd(), max_y = rd();
        const size_t cap = (size_t)rdi();
        spe->log.clear();
        map.set_scale_id(map.finest_scale_id());
        M3RSMEngine engine;
        engine.set_translation_lookup_range(max_x, max_y);
        engine.set_rotation_lookup_range(sector, rot_step);
        engine.add_scan_matching_request(spe, pose, *raw_scan, map, false);
        const size_t n_roots = spe->log.size();
        if (!scan_written) {
          // the scan as the device takes it -- what filter_scan kept --: the provider's table entries, weights, factors
          const auto &pts = spe->filtered.points();
          wr((double)pts.size());
          for (size_t i = 0; i < pts.size(); ++i) {
            const int idx = std::round((pts[i].angle() - a_min) / a_inc);
            wr(pts[i].range());
            wr(trig->_cos[idx]);
            wr(trig->_sin[idx]);
            wr(spw->weight(pts, i));
            wr(pts[i].factor());
          }
          scan_written = true;
        }
        // (a call that returns a finest match without branching leaves nothing behind: ask again, as the engine's
        // user does when it adds its own matches, until enough branches are on record or the queue is empty)
        Match best = engine.next_best_match(trl_step);
        for (int k = 0; k < 256 && best.is_valid() && spe->log.size() < n_roots + cap; ++k) best = engine.next_best_match(trl_step);
        const size_t kept = std::min(spe->log.size(), n_roots + cap);
        wr((double)n_roots);
        wr((double)kept);
        wr(best.is_valid() ? best.prob_upper_bound : -1.0);
        for (size_t i = 0; i < kept; ++i) {
          const Record &c = spe->log[i];
          wr(c.pose.x);
          wr(c.pose.y);
          wr(c.pose.theta);
          wr(c.area.bot());
          wr(c.area.top());
          wr(c.area.left());
          wr(c.area.right());
          wr(c.value);
          wr(c.scale_id);
        }
      }
      map.set_scale_id(map.finest_scale_id());
    }
  }
  FILE *f = std::fopen(argv[2], "wb");
  if (!f) return 1;
  std::fwrite(out_buf.data(), sizeof(double), out_buf.size(), f);
  std::fclose(f);
  return 0;
}
