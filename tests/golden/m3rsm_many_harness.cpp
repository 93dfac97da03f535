// tests/golden/m3rsm_many_harness.cpp -- TEST INFRASTRUCTURE ONLY (golden data for tests/golden/m3rsm_many.npz).
//
// A small program around the UNMODIFIED reference headers (slam_constructor's src/, given with -I): the reference's own
// M3RSMEngine (core/scan_matchers/m3rsm_engine.h) given SEVERAL scan matching requests -- each its own scan, pose and
// M3RSMRescalableGridMap<UnboundedPlainGridMap> -- and driven by the loop of BruteForceMultiResolutionScanMatcher::
// process_scan (core/scan_matchers/bf_multi_res_scan_matcher.h:44-65), with a recording ScanProbabilityEstimator per
// request (each over an estimator and a point weighting of that request's own) that writes every scorer call down in call
// order.  Per scene:
//   M  all requests in one engine, prerotate_scan = true (as the matcher runs it): winner, result, trace;
//   N  the same with prerotate_scan = false;
//   P  run M once more with every score multiplied by 1 +- 1e-12;
//   L  every request alone in an engine of its own (prerotated): result and number of calls.
// tests/golden/make_golden_m3rsm_many.py compiles it (g++ -std=c++14 -O3, the reference's own flags), feeds it one file
// of doubles and packs what it writes; the binary is never committed and nothing in the product path knows about it.
//
//   m3rsm_many_harness <input.bin> <output.bin>
//
// Input and output are flat arrays of doubles in the order read / written below.  Access control is relaxed only so
// that a fine map's origin can be moved off its centre and the cached trig provider's table can be read.
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
    std::fprintf(stderr, "m3rsm_harness: input too short\n");
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

// one scorer call: whose it was, what was asked and what came back; (px, py) = the first point of the scan it was asked
// about, which tells the prerotated scans of a request apart
struct Record {
  int request;
  RobotPose pose;
  LightWeightRectangle area;
  double value;
  int scale_id;
  double px, py;
};

struct Log {
  std::vector<Record> calls;
  bool perturb = false;
};

// A ScanProbabilityEstimator of our own, one per request, that hands every call to the reference's estimator and writes
// it down in the log all requests share
class RecordingSPE : public ScanProbabilityEstimator {
public:
  RecordingSPE(std::shared_ptr<ScanProbabilityEstimator> real, OOPE oope, int request, Log *log)
      : ScanProbabilityEstimator{oope}, _real{real}, _request{request}, _log{log} {}
  LaserScan2D filter_scan(const LaserScan2D &scan, const RobotPose &pose, const GridMap &map) override {
    filtered = _real->filter_scan(scan, pose, map);
    return filtered;
  }
  double estimate_scan_probability(const LaserScan2D &scan, const RobotPose &pose, const GridMap &map,
                                   const SPEParams &params) const override {
    double v = _real->estimate_scan_probability(scan, pose, map, params);
    const auto &pts = scan.points();
    const bool cart = !pts.empty() && pts[0]._type == ScanPoint2D::PointType::Cartesian;
    _log->calls.push_back(Record{_request, pose, params.sp_analysis_area, v, (int)dynamic_cast<const Map &>(map).scale_id(),
                                 cart ? pts[0].x() : 0.0, cart ? pts[0].y() : 0.0});
    if (_log->perturb) {
      const unsigned k = (unsigned)_log->calls.size() * 2654435761u;
      v = v * (((k >> 13) & 1) ? 1 + 1e-12 : 1 - 1e-12);
    }
    return v;
  }
  LaserScan2D filtered;

private:
  std::shared_ptr<ScanProbabilityEstimator> _real;
  int _request;
  Log *_log;
};

void write_records(const std::vector<Record> &log) {
  wr((double)log.size());
  for (const Record &c : log) {
    wr(c.request);
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

struct Scan {
  LaserScan2D scan;
  std::shared_ptr<CachedTrigonometryProvider> trig;
  double a_min, a_inc;
};

// (an estimator and a weighting of its own per request, as add_scan_matching_request's signature allows: the reference's
// ScanPointWeighting keeps the weights of the scan it filtered LAST -- EvenSPW::reset, weighted_mean_point_probability_
// spe.h:23-25 --, so requests that shared one would all be scored with the last request's weights)
struct Request {
  int map, scan;
  RobotPose pose{0, 0, 0};
  std::shared_ptr<EvenSPW> spw;
  std::shared_ptr<RecordingSPE> spe;
};

struct Limits {
  double max_x, max_y, max_th, rot_step, trl_step;
};

// The requests `which` in one engine under the matcher's loop: writes winner, delta (3), prob; the calls are in the log
void run_engine(std::vector<std::unique_ptr<Map>> &maps, std::vector<Scan> &scans, std::vector<Request> &reqs,
                const std::vector<int> &which, const Limits &lim, bool prerotate) {
  for (auto &m : maps) m->set_scale_id(m->finest_scale_id());
  M3RSMEngine engine;
  engine.reset_engine_state();
  engine.set_translation_lookup_range(lim.max_x, lim.max_y);
  engine.set_rotation_lookup_range(2 * lim.max_th, lim.rot_step);
  // (SafeRescalableMap restores a map's scale when it goes; one per map, alive for the whole search, as the matcher's is)
  std::vector<std::unique_ptr<SafeRescalableMap>> safe;
  for (auto &m : maps) safe.emplace_back(new SafeRescalableMap{*m});
  for (int r : which)
    engine.add_scan_matching_request(reqs[r].spe, reqs[r].pose, scans[reqs[r].scan].scan, *safe[reqs[r].map], prerotate);
  int winner = -1;
  RobotPoseDelta delta;
  double prob = 0;
  while (1) {
    auto best_match = engine.next_best_match(lim.trl_step);
    if (!best_match.is_valid()) std::exit(3);
    if (best_match.is_finest()) {
      delta = {best_match.translation_drift.center(), best_match.rotation};
      prob = best_match.prob_upper_bound;
      for (int r : which)
        if (best_match.pose == &reqs[r].pose) winner = r;
      break;
    }
    auto crucial_points = best_match.translation_drift.corners();
    crucial_points.push_back(best_match.translation_drift.center());
    for (const auto &cp : crucial_points) engine.add_match(Match{M3RSMEngine::Rect{cp}, best_match});
  }
  wr(winner);
  wr(delta.x);
  wr(delta.y);
  wr(delta.theta);
  wr(prob);
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
    std::shared_ptr<ObservationImpactEstimator> oie;
    if (oie_kind == 0) oie = std::make_shared<DiscrepancyOIE>();
    else oie = std::make_shared<OccupancyOIE>();
    // ---- the maps: geometry, updates; then every level written out as m3rsm_harness does ----
    const int n_maps = rdi();
    std::vector<std::unique_ptr<Map>> maps;
    for (int mi = 0; mi < n_maps; ++mi) {
      const int w = rdi(), h = rdi();
      const double scale = rd();
      const int ox = rdi(), oy = rdi();
      maps.emplace_back(new Map(oie, prototype(cls), GridMapParams{w, h, scale}));
      Map &map = *maps.back();
      static_cast<UnboundedPlainGridMap &>(*(*map._map_cache)[0])._origin = DiscretePoint2D{ox, oy};
      map.set_scale_id(map.finest_scale_id());
      const int n_obs = rdi();
      for (int i = 0; i < n_obs; ++i) {
        const int x = rdi(), y = rdi();
        const bool is_occ = rd() != 0.0;
        const double prob = rd(), est_quality = rd(), quality = rd();
        map.update({x, y}, AreaOccupancyObservation{is_occ, Occupancy{prob, est_quality}, Point2D{0, 0}, quality});
      }
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
    }
    // ---- the scans ----
    const int n_scans = rdi();
    std::vector<Scan> scans(n_scans);
    for (Scan &s : scans) {
      const int n = rdi();
      std::vector<double> ranges(n), angles(n);
      for (double &v : ranges) v = rd();
      for (double &v : angles) v = rd();
      s.a_min = rd();
      const double a_max = rd();
      s.a_inc = rd();
      for (int i = 0; i < n; ++i) s.scan.points().emplace_back(ranges[i], angles[i], true);
      s.trig = std::make_shared<CachedTrigonometryProvider>();
      s.trig->update(s.a_min, a_max, s.a_inc);
      s.scan.trig_provider = s.trig;
    }
    const Limits lim{rd(), rd(), rd(), rd(), rd()};
    // ---- the requests ----
    auto oope = std::make_shared<MaxOccupancyObservationPE>(oie);
    Log log;
    const int n_req = rdi();
    std::vector<Request> reqs(n_req);
    std::vector<int> all;
    for (int r = 0; r < n_req; ++r) {
      reqs[r].map = rdi();
      reqs[r].scan = rdi();
      reqs[r].pose = RobotPose{rd(), rd(), rd()};
      reqs[r].spw = std::make_shared<EvenSPW>();
      auto real = std::make_shared<WeightedMeanPointProbabilitySPE>(oope, reqs[r].spw, 0, std::numeric_limits<double>::infinity());
      reqs[r].spe = std::make_shared<RecordingSPE>(real, oope, r, &log);
      all.push_back(r);
    }
    // run M; then, per request, the scan as the device takes it -- what filter_scan kept --: the provider's table
    // entries, weights, factors
    run_engine(maps, scans, reqs, all, lim, true);
    write_records(log.calls);
    for (int r = 0; r < n_req; ++r) {
      const Scan &s = scans[reqs[r].scan];
      const auto &pts = reqs[r].spe->filtered.points();
      wr((double)pts.size());
      for (size_t i = 0; i < pts.size(); ++i) {
        const int idx = std::round((pts[i].angle() - s.a_min) / s.a_inc);
        wr(pts[i].range());
        wr(s.trig->_cos[idx]);
        wr(s.trig->_sin[idx]);
        wr(reqs[r].spw->weight(pts, i));
        wr(pts[i].factor());
      }
    }
    // run N: not prerotated
    log.calls.clear();
    run_engine(maps, scans, reqs, all, lim, false);
    write_records(log.calls);
    // run P: perturbed scores
    log.calls.clear();
    log.perturb = true;
    run_engine(maps, scans, reqs, all, lim, true);
    wr((double)log.calls.size());
    log.perturb = false;
    // runs L: every request alone
    for (int r = 0; r < n_req; ++r) {
      log.calls.clear();
      run_engine(maps, scans, reqs, std::vector<int>{r}, lim, true);
      wr((double)log.calls.size());
    }
    log.calls.clear();
  }
  FILE *f = std::fopen(argv[2], "wb");
  if (!f) return 1;
  std::fwrite(out_buf.data(), sizeof(double), out_buf.size(), f);
  std::fclose(f);
  return 0;
}
