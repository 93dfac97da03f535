// oracle/ref_adapter_scenes.h -- TEST INFRASTRUCTURE ONLY: the scenes ref_consumers_harness.cpp and
// ref_credibilist_harness.cpp share.  Our own code over the reference's classes; included AFTER the reference's headers
// (with access control relaxed: a hand-made belief is put into a cell the way tests/golden/map_render_harness.cpp does it).
//
//   make_cecum_map   the hand-made map: MockGridCell, 77 x 45 cells of 0.1 m, origin (45, 26) -- moved off the centre by a
//                    GridMapPatcher offset: a one-cell raster stamped at (-45, -26) makes the 64 x 37 window grow by
//                    (13, 8) on the low sides only -- and a 60 x 38 cecum, open at the bottom, stamped inside
//   make_wider_world the cecum plus a trough below its open end and a second cecum on its right: what `extra_pose` scans
//   SlamMap          a map of one of the cell classes the resident factories produce, built by the reference's scan adder
//                    from scans the reference's generator takes off the cecum; starts at 40 x 30 cells and grows
//   special cells    beliefs a scan cannot produce (conflict is normalised away by every update), written on both sides
//   DevMap           the map copied into HBM (slamhip_map_bind + slamhip_map_upload_window) under a HipResidentMapView
#ifndef SLAMHIP_ORACLE_REF_ADAPTER_SCENES_H
#define SLAMHIP_ORACLE_REF_ADAPTER_SCENES_H

namespace scn {

constexpr double kScale = 0.1;
enum { MOCK = 0, MEAN = 1, AFFINE = 2, TBM_CONSISTENT = 3, TBM_UNKNOWN_EVEN = 4, CREDIBILIST = 5, N_CLASSES = 6 };

inline std::string num(double v) {
  char b[40];
  std::snprintf(b, sizeof b, "%.17g", v);
  return b;
}

inline int stride(int cls) { return cls >= TBM_CONSISTENT ? 4 : 1; }
inline int model(int cls) {
  return cls == CREDIBILIST ? SLAMHIP_CELL_CREDIBILIST : (cls >= TBM_CONSISTENT ? SLAMHIP_CELL_TBM : SLAMHIP_CELL_OCC);
}
// what a HipResidentMapView over the class is given: tbm_unknown_even_occ and TBM_to_O are both o + 0.5 u
inline int tbm_kind(int cls) { return (cls == TBM_UNKNOWN_EVEN || cls == CREDIBILIST) ? 1 : 0; }
inline int rule(int cls) {
  return cls == MEAN ? SLAMHIP_RULE_MEAN : (cls == AFFINE ? SLAMHIP_RULE_AFFINE : (cls == MOCK ? SLAMHIP_RULE_LAST : SLAMHIP_RULE_TBM));
}
inline const char *area_type(int cls) {
  switch (cls) {
    case MEAN: return "mean_probability";
    case AFFINE: return "affine_quality_merge";
    case TBM_CONSISTENT: return "tbm_consistent";
    default: return "tbm_unknown_even_occ";
  }
}
// the threshold the generator scenes use on a map of the class: the stamped walls are 1; built walls lie above these
inline double occ_threshold(int cls) { return cls == MOCK ? 1.0 : (cls >= TBM_UNKNOWN_EVEN ? 0.55 : 0.6); }

inline std::shared_ptr<GridCell> prototype(int cls) {
  switch (cls) {
    case MOCK: return std::make_shared<MockGridCell>(0.0);
    case MEAN: return std::make_shared<MeanProbabilityCell>();
    case AFFINE: return std::make_shared<AffineQualityMergeCell>();
    case TBM_CONSISTENT: return std::make_shared<TbmOccConsistentCell>();
    case TBM_UNKNOWN_EVEN: return std::make_shared<TbmUnknownEvenOccCell>();
    default: return std::make_shared<CredibilistCell>();
  }
}

inline void payload(int cls, const GridCell &c, double *p) {
  if (stride(cls) == 1) {
    p[0] = c.occupancy().prob_occ;
    return;
  }
  const TBM &b = cls == CREDIBILIST ? static_cast<const CredibilistCell &>(c).belief() : static_cast<const TbmBaseCell &>(c).belief();
  p[0] = b.unknown(); p[1] = b.empty(); p[2] = b.occupied(); p[3] = b.conflict();
}

// the scan adder of every scene: blur 0.3 m, the constant estimator; TBM classes with qualities under 1 so that the
// masses move scan by scan
constexpr double kOccProb = 0.95, kEmptyProb = 0.01, kBlur = 0.3;
inline double occ_qual(int cls) { return cls >= TBM_CONSISTENT ? 0.4 : 1.0; }
inline double empty_qual(int cls) { return cls >= TBM_CONSISTENT ? 0.1 : 1.0; }
inline void mapping_props(MapPropertiesProvider &p, int cls) {
  p.set_property("slam/mapping/blur", num(kBlur));
  p.set_property("slam/occupancy_estimator/type", "const");
  p.set_property("slam/occupancy_estimator/base_occupied/prob", num(kOccProb));
  p.set_property("slam/occupancy_estimator/base_empty/prob", num(kEmptyProb));
  p.set_property("slam/occupancy_estimator/base_occupied/qual", num(occ_qual(cls)));
  p.set_property("slam/occupancy_estimator/base_empty/qual", num(empty_qual(cls)));
  p.set_property("slam/mapping/grid/area/type", area_type(cls));
  p.set_property("slam/mapping/grid/type", "unbounded_plain");
  p.set_property("slam/map/meters_per_cell", num(kScale));
}
inline slamhip_scan_adder_cfg device_adder(int cls, double scan_quality) {
  slamhip_scan_adder_cfg a{};
  a.rule = rule(cls);
  a.scan_quality = scan_quality;
  a.base_occupied_prob = kOccProb;
  a.base_occupied_qual = occ_qual(cls);
  a.base_empty_prob = kEmptyProb;
  a.base_empty_qual = empty_qual(cls);
  a.blur = kBlur;
  a.max_range = std::numeric_limits<double>::infinity();
  a.occupancy_estimator = 0;
  a.area_shift_amount = 0;
  return a;
}

inline RobotPose off_boundary(RobotPose p) {  // (the generator's "not on a cell boundary" precondition)
  if (std::fabs(p.x / kScale - std::round(p.x / kScale)) < 1e-3) p.x += 0.013;
  if (std::fabs(p.y / kScale - std::round(p.y / kScale)) < 1e-3) p.y += 0.013;
  return p;
}

// cecum: top wall y = 15, x in [-40, 19]; side walls x = -40 and x = 19 down to y = -22; open below
constexpr int kCecumW = 60, kCecumH = 38, kCecumX = -40, kCecumY = 15;
inline std::shared_ptr<UnboundedPlainGridMap> make_cecum_map() {
  auto m = std::make_shared<UnboundedPlainGridMap>(std::make_shared<MockGridCell>(0.0), GridMapParams{64, 37, kScale});
  std::stringstream one{" \n"};
  GridMapPatcher{}.apply_text_raster(*m, one, DiscretePoint2D{-45, -26}, 1, 1);
  using C = CecumTextRasterMapPrimitive;
  C c{kCecumW, kCecumH, C::BoundPosition::Top};
  GridMapPatcher{}.apply_text_raster(*m, c.to_stream(), DiscretePoint2D{kCecumX, kCecumY}, 1, 1);
  return m;
}

// the world after the robot has left the cecum: a trough below the open end and a second cecum to the right, both outside
// every window built from the cecum alone -- the scans of `extra_pose` make a map GROW
inline std::shared_ptr<UnboundedPlainGridMap> make_wider_world() {
  auto m = make_cecum_map();
  using C = CecumTextRasterMapPrimitive;
  C trough{31, 8, C::BoundPosition::Bot}, right{9, 20, C::BoundPosition::Top};
  GridMapPatcher{}.apply_text_raster(*m, trough.to_stream(), DiscretePoint2D{-25, -30}, 1, 1);
  GridMapPatcher{}.apply_text_raster(*m, right.to_stream(), DiscretePoint2D{30, 0}, 1, 1);
  return m;
}

inline LaserScan2D ref_scan(const GridMap &gt, const RobotPose &pose, const LaserScannerParams &lsp, double thr = 1.0) {
  return LaserScanGenerator{lsp}.laser_scan_2D(gt, pose, thr);
}

// the poses the SLAM-built maps are made from (inside the cecum) and the quality of each append
inline std::vector<RobotPose> build_poses() {
  return {off_boundary({-1.033, -0.948, 1.5708}), off_boundary({-0.533, -0.512, 1.9}), off_boundary({0.267, -0.148, 1.2}),
          off_boundary({-2.033, 0.352, 0.6}), off_boundary({0.667, -1.448, 2.6}), off_boundary({-3.033, -1.252, 0.9}),
          off_boundary({1.233, 0.652, 3.3})};
}
inline double build_quality(int k) {
  const double q[7] = {0.9, 0.6, 0.75, 0.85, 0.65, 0.8, 0.7};
  return q[k % 7];
}
// one more scan, taken off make_wider_world(): the update between two looks at a map.  0: below the open end, looking down
// into the trough; 1: outside the cecum on the right, looking at the second one
inline RobotPose extra_pose(int k) { return k == 0 ? off_boundary({-1.033, -2.452, -1.57}) : off_boundary({2.533, -2.652, 0.2}); }

struct SlamMap {
  int cls;
  MapPropertiesProvider props;
  std::shared_ptr<UnboundedPlainGridMap> map;
  std::shared_ptr<GridMapScanAdder> adder;
  long grown = 0;
  LaserScannerParams lsp = to_lsp(15, 270, 90);

  explicit SlamMap(int c) : cls{c} {
    mapping_props(props, c);
    map = std::make_shared<UnboundedPlainGridMap>(prototype(c), GridMapParams{40, 30, kScale});
    adder = init_scan_adder(props);
  }
  void append(const GridMap &gt, const RobotPose &pose, double quality) { append(ref_scan(gt, pose, lsp), pose, quality); }
  void append(const LaserScan2D &scan, const RobotPose &pose, double quality) {
    const int w = map->width(), h = map->height();
    const auto org = map->origin();
    adder->append_scan(*map, pose, scan, quality, 0);
    if (w != map->width() || h != map->height() || !(org == map->origin())) ++grown;
  }
  void build(const GridMap &gt) {
    int k = 0;
    for (const auto &p : build_poses()) append(gt, p, build_quality(k++));
  }
};

// hand-made beliefs on two cells next to the cecum's top wall, inside every built window (external coordinates)
struct Special {
  int x, y;
  double tbm[4];
};
inline std::vector<Special> special_cells() {
  return {{-12, 13, {0.7, 0.0, 0.0, 0.3}},    // occupied + empty == 0 with unknown < 1
          {-11, 13, {0.2, 0.3, 0.4, 0.1}},    // conflict the normalisation never leaves behind
          {-10, 13, {0.0, 0.0, 0.0, 1.0}}};   // nothing but conflict
}
inline void put_special_host(int cls, UnboundedPlainGridMap &m) {
  if (stride(cls) != 4) return;
  for (const auto &s : special_cells()) {
    auto cell = prototype(cls);
    if (cls == CREDIBILIST) {
      auto &c = static_cast<CredibilistCell &>(*cell);
      c._belief = TBM(s.tbm[0], s.tbm[1], s.tbm[2], s.tbm[3]);
      c.refresh_grid_cell();
    } else {
      auto &c = static_cast<TbmBaseCell &>(*cell);
      c._belief = TBM(s.tbm[0], s.tbm[1], s.tbm[2], s.tbm[3]);
      c._occupancy = c.tbm2occ(c._belief);
    }
    cell->_is_unknown = false;
    m.reset({s.x, s.y}, *cell);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// a host map's copy in HBM under a view
struct DevMap {
  slamhip_ctx *ctx;
  int id, cls;
  std::unique_ptr<HipResidentMapView> view;

  DevMap(slamhip_ctx *c, int map_id, int cell_class, const GridMap &m) : ctx{c}, id{map_id}, cls{cell_class} {
    upload(m);
    view = std::make_unique<HipResidentMapView>(ctx, id, GridMapParams{m.width(), m.height(), m.scale()},
                                                prototype(cls)->occupancy().prob_occ, tbm_kind(cls));
  }
  // the whole host map again, whatever its geometry is now; the TBM special cells go through slamhip_map_apply_dirty
  void upload(const GridMap &m) {
    const int st = stride(cls), w = m.width(), h = m.height();
    const auto org = m.origin();
    double unk[4] = {0, 0, 0, 0};
    payload(cls, *m.new_cell(), unk);
    slamhip_or_die(slamhip_map_bind(ctx, id, model(cls), w, h, org.x, org.y, m.scale(), unk), "map_bind");
    slamhip_or_die(slamhip_map_set_auto_grow(ctx, id, 1), "map_set_auto_grow");
    std::vector<double> buf((size_t)w * h * st);
    std::vector<int> xy;
    std::vector<double> vals;
    for (int y = 0; y < h; ++y)
      for (int x = 0; x < w; ++x) {
        double *p = &buf[((size_t)y * w + x) * st];
        payload(cls, m[{x - org.x, y - org.y}], p);
        if (st == 4 && p[3] != 0.0) {  // a hand-made belief: the window gets the unknown cell, the dirty path the belief
          xy.push_back(x);
          xy.push_back(y);
          vals.insert(vals.end(), p, p + 4);
          std::memcpy(p, unk, sizeof unk);
        }
      }
    slamhip_or_die(slamhip_map_upload_window(ctx, id, 0, 0, w, h, buf.data()), "map_upload_window");
    if (!xy.empty()) slamhip_or_die(slamhip_map_apply_dirty(ctx, id, (int)xy.size() / 2, xy.data(), vals.data()), "map_apply_dirty");
    if (view) view->invalidate();
  }
};

}  // namespace scn

#endif
