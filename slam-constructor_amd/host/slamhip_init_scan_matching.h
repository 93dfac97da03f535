// slamhip_init_scan_matching.h -- the factory a maintainer adds next to init_scan_matcher
// (src/utils/init_scan_matching.h:193-218): same properties, same console lines, but the matcher it
// returns runs on the GPU through the C-ABI.  Compiled only with the reference headers on the include
// path; contains no reference code.  oracle/sm_runner_hip.cpp is the reference's offline tool
// (src/utils/sm_runner.cpp) with this factory in place of the reference's.
#ifndef SLAMHIP_INIT_SCAN_MATCHING_H
#define SLAMHIP_INIT_SCAN_MATCHING_H

#include <cstdlib>
#include <iostream>
#include <memory>
#include <string>

#include "utils/init_scan_matching.h"
#include "slamhip_reference_adapter.h"
#include "slamhip_m3rsm_map.h"

// cell_model >= 0: the payload model of the map instead of the one "slam/mapping/grid/area/type" names (a world whose
// cell class is fixed by its factory: slamhip_credibilist_slam.h), with the reader of its cells' belief masses.
// m3rsm_map: the resident map with its levels that "slam/scmtch/type" = BF_M3RSM matches against (the multi-resolution
// matcher bounds its candidates on levels kept in HBM, so it needs the map to live there: slamhip_m3rsm_map.h)
inline std::shared_ptr<GridScanMatcher> init_hip_scan_matcher(const PropertiesProvider &props,
                                                              slamhip_ctx *ctx = nullptr, int map_id = 0,
                                                              int cell_model = -1,
                                                              HipMapMirror::BeliefReader belief_reader = nullptr,
                                                              HipM3rsmMap *m3rsm_map = nullptr) {
  if (!ctx) slamhip_or_die(slamhip_ctx_create(props.get_int("slam/scmtch/hip/device", 0), &ctx), "ctx_create");
  // the reference's own SPE: still does filter_scan on the host and prints "Used OIE/OOPE/SWP"
  auto spe = init_spe(props);
  slamhip_spe_cfg cfg{};
  const auto oope = props.get_str(Slam_SM_NS + "oope/type", "obstacle");
  cfg.oope = oope == "max" ? SLAMHIP_OOPE_MAX
             : oope == "mean" ? SLAMHIP_OOPE_MEAN
             : oope == "overlap" ? SLAMHIP_OOPE_OVERLAP : SLAMHIP_OOPE_OBSTACLE;
  cfg.oie = props.get_str(Slam_SM_NS + "oie/type", "discrepancy") == "occupancy" ? SLAMHIP_OIE_OCCUPANCY
                                                                                 : SLAMHIP_OIE_DISCREPANCY;
  cfg.sum_order = props.get_bool(Slam_SM_NS + "hip/strict", false) ? SLAMHIP_SUM_SEQUENTIAL : SLAMHIP_SUM_TREE256;
  // strict: the reference's bits.  Scans carry the RawTrigonometryProvider unless the node was started with
  // use_trig_cache (src/ros/init_utils.h:56-58; laser_scan_observer.h:77-86) -- "hip/trig_cache" says so here --:
  // cos / sin(theta + a) per beam by the restated libm (RAW_EXACT), or the cached provider's angle addition (HOST)
  const bool strict = props.get_bool(Slam_SM_NS + "hip/strict", false);
  const bool trig_cache = props.get_bool(Slam_SM_NS + "hip/trig_cache", false);
  cfg.pose_trig = !strict ? SLAMHIP_POSE_TRIG_DEVICE : (trig_cache ? SLAMHIP_POSE_TRIG_HOST : SLAMHIP_POSE_TRIG_RAW_EXACT);
  const auto type = scan_matcher_type(props);
  std::cout << "Used Scan Matcher: " << type << std::endl;
  slamhip_matcher *m = nullptr;
  if (type == "MC") {
    const std::string ns = Slam_SM_NS + "MC/";
    const auto seed = props.get_int(ns + "seed", std::random_device{}());
    std::cout << "[INFO] MC Scan Matcher seed: " << seed << std::endl;
    slamhip_or_die(slamhip_matcher_create_mc(ctx, &cfg, seed, props.get_dbl(ns + "dispersion/translation", 0.2),
                                             props.get_dbl(ns + "dispersion/rotation", 0.1),
                                             props.get_uint(ns + "dispersion/failed_attempts_limit", 20),
                                             props.get_uint(ns + "attempts_limit", 100), &m), "create_mc");
  } else if (type == "HC") {
    const std::string ns = Slam_SM_NS + "HC/distortion/";
    slamhip_or_die(slamhip_matcher_create_hc(ctx, &cfg, props.get_uint(ns + "failed_attempts_limit", 6),
                                             props.get_dbl(ns + "translation", 0.1),
                                             props.get_dbl(ns + "rotation", 0.1), &m), "create_hc");
  } else if (type == "BF") {
    const std::string ns = Slam_SM_NS + "BF/";
    const double r[9] = {props.get_dbl(ns + "x/from", -0.5), props.get_dbl(ns + "x/to", 0.5),
                         props.get_dbl(ns + "x/step", 0.1), props.get_dbl(ns + "y/from", -0.5),
                         props.get_dbl(ns + "y/to", 0.5), props.get_dbl(ns + "y/step", 0.1),
                         props.get_dbl(ns + "t/from", -deg2rad(5)), props.get_dbl(ns + "t/to", deg2rad(5)),
                         props.get_dbl(ns + "t/step", deg2rad(1))};
    slamhip_or_die(slamhip_matcher_create_bf(ctx, &cfg, r, &m), "create_bf");
  } else if (is_m3rsm(type)) {
    // init_bf_m3rsm (src/utils/init_scan_matching.h:171-183): the same keys, the same defaults
    if (!m3rsm_map) {
      std::cerr << "scan matcher type BF_M3RSM needs the resident map with its levels (HipM3rsmMap)" << std::endl;
      std::exit(-1);
    }
    const std::string ns = Slam_SM_NS + "BF_M3RSM/";
    // (strict: the bounds take the scan's provider as the other matchers do -- RAW_EXACT under the raw provider, whose
    // kept angles HipGridScanMatcher hands over with every scan, HOST with "hip/trig_cache")
    const auto ang_acc = props.get_dbl(ns + "accuracy/rotation", deg2rad(0.1));
    const auto trl_acc = props.get_dbl(ns + "accuracy/translation", 0.05);
    const auto max_x_err = props.get_dbl(ns + "limits/x_translation", 1);
    const auto max_y_err = props.get_dbl(ns + "limits/y_translation", 1);
    const auto max_rot_err = props.get_dbl(ns + "limits/rotation", deg2rad(5));
    m = m3rsm_map->matcher(cfg, max_x_err, max_y_err, max_rot_err, ang_acc, trl_acc);
    map_id = m3rsm_map->map_id();
  } else {
    std::cerr << "scan matcher type " << type << " is outside the HIP path (MC / HC / BF / BF_M3RSM)" << std::endl;
    std::exit(-1);
  }
  const auto area = props.get_str("slam/mapping/grid/area/type", "<undefined>");
  // TBM cells score through their belief masses; every other model (and the occupancy OIE) through
  // occupancy().prob_occ
  const int model = cell_model >= 0 ? cell_model
                    : (area.rfind("tbm", 0) == 0 && cfg.oie == SLAMHIP_OIE_DISCREPANCY) ? SLAMHIP_CELL_TBM
                                                                                        : SLAMHIP_CELL_OCC;
  const auto w = props.get_str(Slam_SM_NS + "spe/wmpp/weighting/type", "even");
  const int weighting = w == "viny" ? 1 : (w == "ahr" ? 2 : 0);
  const auto gm = props.get_str("slam/mapping/grid/type", "<undefined>");
  const bool bounded = gm == "plain" || gm == "lazy_tiled";
  auto mirror = std::make_shared<HipMapMirror>(ctx, map_id, model, bounded);
  mirror->set_belief_reader(belief_reader);
  auto gsm = std::make_shared<HipGridScanMatcher>(spe, ctx, m, mirror, weighting);
  if (is_m3rsm(type)) {
    gsm->set_resident_map(true);  // (the map is matched where it lives: nothing to mirror)
    // the reference's matcher weighs PREROTATED points: any weighting but `even` turns with the candidate's rotation
    if (weighting == 1)
      gsm->set_m3rsm_rotation_weights(std::make_shared<VinySlamSPW>(), m3rsm_map->pyramid(),
                                      props.get_int(Slam_SM_NS + "hip/m3rsm_first_scan_slot", 0));
    else if (weighting == 2)
      gsm->set_m3rsm_rotation_weights(std::make_shared<AngleHistogramReciprocalSPW>(), m3rsm_map->pyramid(),
                                      props.get_int(Slam_SM_NS + "hip/m3rsm_first_scan_slot", 0));
  }
  if (props.get_str(Slam_SM_NS + "spe/type", "<undefined>") == "wmpp")  // (init_spe's own parameters, :99-100)
    gsm->set_filter_params(props.get_uint(Slam_SM_NS + "spe/wmpp/sp_skip_rate", 0),
                           props.get_dbl(Slam_SM_NS + "spe/wmpp/sp_max_usable_range", -1), bounded);
  return gsm;
}

#endif  // SLAMHIP_INIT_SCAN_MATCHING_H
