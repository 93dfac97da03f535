// tests/golden/credibilist_harness.cpp -- TEST INFRASTRUCTURE ONLY (golden data for tests/golden/credibilist.npz).
//
// A small program around the UNMODIFIED reference headers (slam_constructor's src/, given with -I): the CredibilistCell
// of src/slams/credibilist/grid_cell.h through the reference's own scan adder, scan probability estimators, matchers
// and single-hypothesis world.  tests/golden/make_golden_credibilist.py compiles it (g++ -std=c++14 -O3, the
// reference's own flags), feeds it one file of doubles and packs what it writes; the binary is never committed and
// nothing in the product path knows about it.
//
//   credibilist_harness <input.bin> <output.bin>
//
// Input and output are flat arrays of doubles in the order read / written below.  Access control is relaxed only so
// that the hand-made edge beliefs can be put into a cell (CredibilistCell::_belief).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#define private public
#define protected public
#include "core/maps/plain_grid_map.h"
#include "core/maps/grid_map_scan_adders.h"
#include "core/maps/const_occupancy_estimator.h"
#include "core/scan_matchers/observation_impact_estimators.h"
#include "core/scan_matchers/occupancy_observation_probability.h"
#include "core/scan_matchers/weighted_mean_point_probability_spe.h"
#include "core/scan_matchers/monte_carlo_scan_matcher.h"
#include "core/scan_matchers/hill_climbing_scan_matcher.h"
#include "core/states/single_state_hypothesis_laser_scan_grid_world.h"
#include "slams/credibilist/grid_cell.h"
#undef private
#undef protected

namespace {

std::vector<double> in_buf, out_buf;
size_t in_pos = 0;
double rd() {
  if (in_pos >= in_buf.size()) {
    std::fprintf(stderr, "credibilist_harness: input too short\n");
    std::exit(2);
  }
  return in_buf[in_pos++];
}
int rdi() { return (int)rd(); }
void wr(double v) { out_buf.push_back(v); }

struct Trace : public GridScanMatcherObserver {
  std::vector<double> poses, scores, accepted;
  void on_scan_test(const RobotPose &p, const LaserScan2D &, double s) override {
    poses.push_back(p.x);
    poses.push_back(p.y);
    poses.push_back(p.theta);
    scores.push_back(s);
    accepted.push_back(0);
  }
  void on_pose_update(const RobotPose &, const LaserScan2D &, double) override {
    if (!accepted.empty()) accepted.back() = 1;
  }
};

// the scorer's fixed observation (weighted_mean_point_probability_spe.h: expected_scan_point_observation)
AreaOccupancyObservation scorer_observation() { return AreaOccupancyObservation{true, {1.0, 1.0}, {0, 0}, 1.0}; }

void write_belief(const GridCell &c) {
  const TBM &t = static_cast<const CredibilistCell &>(c).belief();
  wr(t.unknown());
  wr(t.empty());
  wr(t.occupied());
  wr(t.conflict());
}

void write_map(const GridMap &m) {
  wr(m.width());
  wr(m.height());
  wr(m.origin().x);
  wr(m.origin().y);
  for (int y = 0; y < m.height(); ++y)
    for (int x = 0; x < m.width(); ++x) write_belief(m[{x - m.origin().x, y - m.origin().y}]);
}

struct ScanGeom {
  int n;
  double a_min, a_inc;
};

LaserScan2D make_scan(const ScanGeom &g, const std::vector<double> &ranges, bool cached) {
  LaserScan2D s;
  for (int i = 0; i < g.n; ++i) s.points().emplace_back(ranges[i], g.a_min + i * g.a_inc, true);
  if (cached) {
    auto p = std::make_shared<CachedTrigonometryProvider>();
    // (a_max as src/ros/laser_scan_observer.h:80 passes it: the last angle + two increments)
    p->update(g.a_min, g.a_min + (g.n - 1) * g.a_inc + 2 * g.a_inc, g.a_inc);
    s.trig_provider = p;
  } else {
    s.trig_provider = std::make_shared<RawTrigonometryProvider>();
  }
  return s;
}

std::vector<double> read_ranges(int n) {
  std::vector<double> r(n);
  for (auto &v : r) v = rd();
  return r;
}

std::shared_ptr<GridMapScanAdder> make_adder(const double *base4, double blur) {
  auto est = std::make_shared<ConstOccupancyEstimator>(Occupancy{base4[0], base4[1]}, Occupancy{base4[2], base4[3]});
  return WallDistanceBlurringScanAdder::builder()
      .set_occupancy_estimator(est)
      .set_observation_quality_estimator(std::make_shared<IdleOMQE>())
      .set_blur_distance(blur)
      .set_max_usable_range(std::numeric_limits<double>::infinity())
      .build();
}

std::shared_ptr<WeightedMeanPointProbabilitySPE> make_spe(int oope) {
  auto oie = std::make_shared<DiscrepancyOIE>();
  std::shared_ptr<OccupancyObservationProbabilityEstimator> o;
  switch (oope) {
    case 1: o = std::make_shared<MaxOccupancyObservationPE>(oie); break;
    case 2: o = std::make_shared<MeanOccupancyObservationPE>(oie); break;
    case 3: o = std::make_shared<OverlapWeightedOccupancyObservationPE>(oie); break;
    default: o = std::make_shared<ObstacleBasedOccupancyObservationPE>(oie); break;
  }
  return std::make_shared<WeightedMeanPointProbabilitySPE>(o, std::make_shared<EvenSPW>());
}

void write_trace(GridScanMatcher &sm, const LaserScan2D &scan, const RobotPose &pose, const GridMap &map) {
  TransformedLaserScan ts;
  ts.scan = scan;
  ts.quality = 1.0;
  auto obs = std::make_shared<Trace>();
  sm.subscribe(obs);
  RobotPoseDelta d;
  const double prob = sm.process_scan(ts, pose, map, d);
  sm.unsubscribe(obs);
  wr((double)obs->scores.size());
  wr(prob);
  wr(d.x);
  wr(d.y);
  wr(d.theta);
  for (double v : obs->poses) wr(v);
  for (double v : obs->scores) wr(v);
  for (double v : obs->accepted) wr(v);
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
  ScanGeom g;
  g.n = rdi();
  g.a_min = rd();
  g.a_inc = rd();
  const int map_w = rdi(), map_h = rdi();
  const double scale = rd(), blur = rd();
  double base4[4], area4[4];
  for (double &v : base4) v = rd();
  for (double &v : area4) v = rd();

  // ---- cells: update sequences through CredibilistCell::operator+=, then hand-made beliefs ----
  const int n_cells = rdi(), n_steps = rdi();
  const auto obs = scorer_observation();
  for (int c = 0; c < n_cells; ++c) {
    CredibilistCell cell;
    for (int s = 0; s < n_steps; ++s) {
      const double prob = rd(), qual = rd(), quality = rd();
      cell += AreaOccupancyObservation{true, {prob, qual}, {0, 0}, quality};
      write_belief(cell);
      wr(1.0 - cell.discrepancy(obs));
      wr(cell.occupancy().prob_occ);
    }
  }
  const int n_edges = rdi();
  for (int e = 0; e < n_edges; ++e) {
    const double u = rd(), em = rd(), o = rd(), cf = rd();
    CredibilistCell cell;
    cell._belief = TBM(u, em, o, cf);
    wr(1.0 - cell.discrepancy(obs));
  }
  {  // a never-observed cell
    CredibilistCell cell;
    write_belief(cell);
    wr(1.0 - cell.discrepancy(obs));
    wr(cell.occupancy().prob_occ);
  }

  // ---- scene: a map built by the scan adder, the beliefs after each append ----
  auto map = std::make_shared<UnboundedPlainGridMap>(std::make_shared<CredibilistCell>(), GridMapParams{map_w, map_h, scale});
  auto adder = make_adder(base4, blur);
  const int n_map_scans = rdi();
  for (int k = 0; k < n_map_scans; ++k) {
    const double x = rd(), y = rd(), th = rd(), quality = rd();
    const int cached = rdi();
    auto scan = make_scan(g, read_ranges(g.n), cached != 0);
    adder->append_scan(*map, RobotPose{x, y, th}, scan, quality, 0);
    write_map(*map);
  }

  // ---- scores: every OOPE with the raw and the cached provider ----
  const RobotPose init{rd(), rd(), rd()};
  const auto match_ranges = read_ranges(g.n);
  const int n_poses = rdi();
  std::vector<double> poses(3 * (size_t)n_poses);
  for (auto &v : poses) v = rd();
  for (int cached = 0; cached < 2; ++cached) {
    auto raw_scan = make_scan(g, match_ranges, cached != 0);
    for (int oope = 0; oope < 4; ++oope) {
      auto spe = make_spe(oope);
      auto fs = spe->filter_scan(raw_scan, init, *map);
      if (oope == 0) {
        wr((double)fs.points().size());
        for (auto &p : fs.points()) wr(p.range());
        for (auto &p : fs.points()) wr(p.angle());
        for (auto &p : fs.points()) wr(p.factor());
        EvenSPW spw;
        spw.reset(fs);
        for (size_t i = 0; i < fs.points().size(); ++i) wr(spw.weight(fs.points(), i));
      }
      ScanProbabilityEstimator::SPEParams prm;
      if (oope != 0) prm.sp_analysis_area = LightWeightRectangle{area4[0], area4[1], area4[2], area4[3]};
      for (int i = 0; i < n_poses; ++i)
        wr(spe->estimate_scan_probability(fs, RobotPose{poses[3 * i], poses[3 * i + 1], poses[3 * i + 2]}, *map, prm));
    }
  }

  // ---- matcher traces (cached provider) ----
  double hc[3], mc[5];
  for (double &v : hc) v = rd();
  for (double &v : mc) v = rd();
  {
    auto scan = make_scan(g, match_ranges, true);
    HillClimbingScanMatcher hcm(make_spe(0), (unsigned)hc[0], hc[1], hc[2]);
    write_trace(hcm, scan, init, *map);
    MonteCarloScanMatcher mcm(make_spe(0), (unsigned)mc[0], mc[1], mc[2], (unsigned)mc[3], (unsigned)mc[4]);
    write_trace(mcm, scan, init, *map);
  }

  // ---- world: init_credibilist_slam's world (src/slams/credibilist/init_slam.h) over a few scans ----
  {
    SingleStateHypothesisLSGWProperties props;
    props.localized_scan_quality = 0.9;
    props.raw_scan_quality = 0.6;
    props.grid_map = std::make_shared<UnboundedPlainGridMap>(std::make_shared<CredibilistCell>(), GridMapParams{map_w, map_h, scale});
    props.gsm = std::make_shared<HillClimbingScanMatcher>(make_spe(0), (unsigned)hc[0], hc[1], hc[2]);
    props.gmsa = make_adder(base4, blur);
    SingleStateHypothesisLaserScanGridWorld world(props);
    const int n_world = rdi();
    for (int k = 0; k < n_world; ++k) {
      TransformedLaserScan ts;
      ts.pose_delta = RobotPoseDelta{rd(), rd(), rd()};
      ts.scan = make_scan(g, read_ranges(g.n), true);
      ts.quality = 1.0;
      world.handle_sensor_data(ts);
      wr(world.pose().x);
      wr(world.pose().y);
      wr(world.pose().theta);
      wr(ts.quality);
    }
    write_map(world.map());
  }

  FILE *f = std::fopen(argv[2], "wb");
  if (!f) return 1;
  std::fwrite(out_buf.data(), sizeof(double), out_buf.size(), f);
  std::fclose(f);
  return 0;
}
