// slamhip_credibilist_slam.h -- the factory next to init_credibilist_slam (src/slams/credibilist/init_slam.h:14-26):
// the single-hypothesis world over CredibilistCell (src/slams/credibilist/grid_cell.h) with its map resident in HBM.
// Same properties as init_hip_resident_1h_slam (slamhip_resident_world.h); what init_credibilist_slam fixes is fixed
// here too: the cell class (SLAMHIP_CELL_CREDIBILIST, updated by SLAMHIP_RULE_TBM -- CredibilistCell::operator+= is
// TbmBaseCell's, operation for operation --, vacuous prototype (u, e, o, c) = (1, 0, 0, 0)) and the scan qualities
// 0.9 (localized) / 0.6 (raw).  The cell scores by its own rule, 1 - disjunctive(observation, belief).occupied()
// (csrc/slamhip_internal.h credibilist_probability), under the discrepancy OIE only.
//
// This header includes slams/credibilist/grid_cell.h, whose TBM_prob_conversion.h DEFINES non-inline functions
// (TBM_to_O, AOO_to_TBM): include it in ONE translation unit of a program, the one that used to include
// slams/credibilist/init_slam.h.  Compiled only with the reference headers on the include path; contains no
// reference code.
#ifndef SLAMHIP_CREDIBILIST_SLAM_H
#define SLAMHIP_CREDIBILIST_SLAM_H

#include <cstring>
#include <iostream>
#include <memory>

#include "utils/init_occupancy_mapping.h"
#include "slams/credibilist/grid_cell.h"
#include "slamhip_resident_world.h"

// the payload of a CredibilistCell for HipMapMirror / HipMirroredGridMap (a host map of such cells mirrored into HBM):
// its own belief() -- the class is no TbmBaseCell
inline void slamhip_credibilist_belief(const GridCell &c, double *out4) {
  const TBM &b = static_cast<const CredibilistCell &>(c).belief();
  out4[0] = b.unknown();
  out4[1] = b.empty();
  out4[2] = b.occupied();
  out4[3] = b.conflict();
}

// a HIP matcher over a HOST map of CredibilistCell (init_hip_scan_matcher with the cell model and its reader set)
inline std::shared_ptr<GridScanMatcher> init_hip_credibilist_scan_matcher(const PropertiesProvider &props,
                                                                          slamhip_ctx *ctx = nullptr, int map_id = 0) {
  if (props.get_str(Slam_SM_NS + "oie/type", "discrepancy") == "occupancy") {
    std::cerr << "credibilist cells score through the discrepancy OIE on the HIP path" << std::endl;
    std::exit(-1);
  }
  return init_hip_scan_matcher(props, ctx, map_id, SLAMHIP_CELL_CREDIBILIST, slamhip_credibilist_belief);
}

inline std::shared_ptr<HipResidentWorld> init_hip_resident_credibilist_slam(const PropertiesProvider &props,
                                                                            slamhip_ctx *ctx = nullptr, int map_id = 0) {
  if (!ctx) slamhip_or_die(slamhip_ctx_create(props.get_int("slam/scmtch/hip/device", 0), &ctx), "ctx_create");
  HipResidentWorld::Config cfg;
  cfg.localized_scan_quality = 0.9;  // init_slam.h:17-18 ("FIXME: move to params")
  cfg.raw_scan_quality = 0.6;
  cfg.map = init_grid_map_params(props);
  cfg.map_id = map_id;
  const auto grid = props.get_str("slam/mapping/grid/type", "<undefined>");
  if (grid != "unbounded_plain" && grid != "unbounded_lazy_tiled") {
    std::cerr << "the resident world keeps an unbounded dense window; grid type " << grid << " is outside it" << std::endl;
    std::exit(-1);
  }
  cfg.cell_model = SLAMHIP_CELL_CREDIBILIST;
  cfg.tbm_kind = 1;  // map() reports TBM_to_O: occupied + 0.5 unknown (TBM_prob_conversion.h:8-10)
  cfg.adder.rule = SLAMHIP_RULE_TBM;
  const double vacuous[4] = {1.0, 0.0, 0.0, 0.0};  // TBM(): total ignorance (transferable_belief_model.h:32,67-72)
  std::memcpy(cfg.unknown, vacuous, sizeof(vacuous));
  slamhip_init_resident_adder(props, cfg);
  auto gsm = std::dynamic_pointer_cast<HipGridScanMatcher>(init_hip_credibilist_scan_matcher(props, ctx, map_id));
  gsm->set_resident_map(true);
  return std::make_shared<HipResidentWorld>(ctx, gsm, cfg);
}

#endif  // SLAMHIP_CREDIBILIST_SLAM_H
