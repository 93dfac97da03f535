// slamhip_scan_generator.h -- the reference's laser scan generator over a map that lives in HBM.
//
// Compiled ONLY with the reference headers on the include path (-I<reference>/src), like slamhip_reference_adapter.h;
// it contains no reference code.  LaserScanGenerator::laser_scan_2D (src/utils/data_generation/laser_scan_generator.h:
// 35-80) reads every cell of every beam through GridMap::operator[]; over a HipResidentMapView that is one synchronous
// 64 x 64 download per chunk the beams cross.  HipLaserScanGenerator ray-casts on the device instead
// (HipResidentMapView::generate_scans -> slamhip_map_generate_scans) and returns the same LaserScan2D: the points
// (range, angle, occupied) of the beams that hit, in beam order, with a RawTrigonometryProvider.  The scanner parameters
// are the reference's own type (LaserScannerParams, to_lsp).  Where the reference would fail an assertion inside a beam
// (an occupied cell the ray meets in neither one nor two points, a scan point outside its cell) this generator throws
// std::logic_error; a robot on a cell boundary (the reference's opening assertion) is refused by the library, and
// slamhip_or_die ends the process as the assertion would.
// A second pair of calls takes a GMapping filter with per-particle maps and particle indices instead of a map: the
// scans come from the particles' own tiled maps (slamhip_gmapping_particle_generate_scans).
#ifndef SLAMHIP_SCAN_GENERATOR_H
#define SLAMHIP_SCAN_GENERATOR_H

#include <memory>
#include <stdexcept>
#include <vector>

#include "core/states/robot_pose.h"
#include "core/states/sensor_data.h"
#include "core/trigonometry_utils.h"
#include "utils/data_generation/laser_scan_generator.h"
#include "slamhip_reference_adapter.h"

class HipLaserScanGenerator {
public:
  explicit HipLaserScanGenerator(LaserScannerParams ls_params = {}) : _max_dist{ls_params.max_dist} {
    int n = 0;
    slamhip_or_die(slamhip_scan_gen_angles(ls_params.h_hsector, ls_params.h_angle_inc, 0, nullptr, &n), "scan_gen_angles");
    _angles.resize((size_t)n);
    slamhip_or_die(slamhip_scan_gen_angles(ls_params.h_hsector, ls_params.h_angle_inc, n, _angles.data(), &n), "scan_gen_angles");
    // the build of glibc's sincos this process runs: the bits the reference's generator would produce here
    slamhip_or_die(slamhip_scan_gen_libm_variant(&_variant), "scan_gen_libm_variant");
    if (_variant < 0) throw std::logic_error("HipLaserScanGenerator: this host's libm is not one the library restates");
  }

  const std::vector<double> &angles() const { return _angles; }

  LaserScan2D laser_scan_2D(const HipResidentMapView &map, const RobotPose &pose, double occ_threshold = 1) const {
    return laser_scans_2D(map, std::vector<RobotPose>{pose}, occ_threshold)[0];
  }

  // many poses in one launch
  std::vector<LaserScan2D> laser_scans_2D(const HipResidentMapView &map, const std::vector<RobotPose> &poses,
                                          double occ_threshold = 1) const {
    const int k = (int)poses.size(), b = (int)_angles.size();
    const std::vector<double> xyt = pack(poses);
    std::vector<double> range((size_t)k * b);
    std::vector<unsigned char> status((size_t)k * b);
    map.generate_scans(_variant, k, xyt.data(), b, _angles.data(), _max_dist, occ_threshold, range.data(), status.data());
    return scans_of(k, range, status);
  }

  // The same from the particles' OWN maps of a GMapping filter with per-particle maps
  // (slamhip_gmapping_enable_particle_maps): scan j is what LOCAL particle particles[j] sees from poses[j] over its
  // tiled map, all of them in one launch over the tile pool (slamhip_gmapping_particle_generate_scans).  A particle may
  // be named several times.
  std::vector<LaserScan2D> laser_scans_2D(slamhip_gmapping *filter, const std::vector<int> &particles,
                                          const std::vector<RobotPose> &poses, double occ_threshold = 1) const {
    if (particles.size() != poses.size()) throw std::logic_error("HipLaserScanGenerator: one pose per named particle");
    const int k = (int)poses.size(), b = (int)_angles.size();
    const std::vector<double> xyt = pack(poses);
    std::vector<double> range((size_t)k * b);
    std::vector<unsigned char> status((size_t)k * b);
    slamhip_or_die(slamhip_gmapping_particle_generate_scans(filter, _variant, 0, k, particles.data(), xyt.data(), b, _angles.data(),
                                                            _max_dist, occ_threshold, range.data(), status.data()),
                   "gmapping_particle_generate_scans");
    return scans_of(k, range, status);
  }

  LaserScan2D laser_scan_2D(slamhip_gmapping *filter, int particle, const RobotPose &pose, double occ_threshold = 1) const {
    return laser_scans_2D(filter, std::vector<int>{particle}, std::vector<RobotPose>{pose}, occ_threshold)[0];
  }

private:
  static std::vector<double> pack(const std::vector<RobotPose> &poses) {
    std::vector<double> xyt(3 * poses.size());
    for (size_t p = 0; p < poses.size(); ++p) {
      xyt[3 * p] = poses[p].x;
      xyt[3 * p + 1] = poses[p].y;
      xyt[3 * p + 2] = poses[p].theta;
    }
    return xyt;
  }

  // the beams that hit, in beam order; status 2 throws
  std::vector<LaserScan2D> scans_of(int k, const std::vector<double> &range, const std::vector<unsigned char> &status) const {
    const int b = (int)_angles.size();
    std::vector<LaserScan2D> scans((size_t)k);
    for (int p = 0; p < k; ++p) {
      scans[p].trig_provider = std::make_shared<RawTrigonometryProvider>();
      for (int i = 0; i < b; ++i) {
        const unsigned char s = status[(size_t)p * b + i];
        if (s == 2) throw std::logic_error("HipLaserScanGenerator: the reference's generator fails an assertion on this beam");
        if (s == 1) scans[p].points().push_back(ScanPoint2D::make_polar(range[(size_t)p * b + i], _angles[i], true));
      }
    }
    return scans;
  }

private:
  double _max_dist;
  std::vector<double> _angles;
  int _variant = -1;
};

#endif
