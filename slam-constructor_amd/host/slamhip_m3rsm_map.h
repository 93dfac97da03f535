// slamhip_m3rsm_map.h -- a resident map with its max-impact levels: the device counterpart of
// M3RSMRescalableGridMap<UnboundedPlainGridMap> (src/core/scan_matchers/m3rsm_engine.h:17-131).
//
// The reference keeps the coarse levels up to date inside GridMap::update, cell by cell.  Here the fine map lives in
// HBM (HipResidentMapView reads it back for the map's consumers), the levels are a slamhip_pyramid over it, and
// append_scan refreshes the levels behind every scan it writes -- queued on the context's stream, so the caller does
// not wait for either.  bounds() is Match::prob_upper_bound (:156-180) for a batch of candidates; matcher() makes the
// device counterpart of BruteForceMultiResolutionScanMatcher over these levels (slamhip_matcher_create_m3rsm: the
// best-first engine, M3RSMEngine :252-365, replayed on the host over expand launches).
// Compiled only with the reference headers on the include path; contains no reference code.
#ifndef SLAMHIP_M3RSM_MAP_H
#define SLAMHIP_M3RSM_MAP_H

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <iostream>
#include <limits>
#include <memory>
#include <vector>

#include "slamhip_reference_adapter.h"

class HipM3rsmMap {
public:
  // map_id: the fine map, already bound (slamhip_map_bind) with cell model OCC, TBM or CREDIBILIST; the levels take
  // the ids first_level_map_id, first_level_map_id + 1, ...
  HipM3rsmMap(slamhip_ctx *ctx, int map_id, int oie, int first_level_map_id, const GridMapParams &params,
              double unknown_prob = 0.5, int tbm_kind = 0)
      : _ctx{ctx}, _map_id{map_id} {
    slamhip_or_die(slamhip_pyramid_create(ctx, map_id, oie, first_level_map_id, &_pyr), "pyramid_create");
    _view = std::make_shared<HipResidentMapView>(ctx, map_id, params, unknown_prob, tbm_kind);
  }
  ~HipM3rsmMap() { slamhip_pyramid_destroy(_pyr); }
  HipM3rsmMap(const HipM3rsmMap &) = delete;
  HipM3rsmMap &operator=(const HipM3rsmMap &) = delete;

  const GridMap &map() const { return *_view; }
  slamhip_pyramid *pyramid() { return _pyr; }
  int map_id() const { return _map_id; }
  void invalidate_view() { _view->invalidate(); }  // the fine map has been written behind the view's back

  // BruteForceMultiResolutionScanMatcher over this map's levels, with init_bf_m3rsm's parameters
  // (src/utils/init_scan_matching.h:171-183).  The caller owns the matcher and destroys it before this map.
  slamhip_matcher *matcher(const slamhip_spe_cfg &cfg, double max_x_error = 1, double max_y_error = 1,
                           double max_th_error = deg2rad(5), double angle_step = deg2rad(0.1),
                           double translation_step = 0.05) {
    slamhip_matcher *m = nullptr;
    slamhip_or_die(slamhip_matcher_create_m3rsm(_ctx, &cfg, _pyr, max_x_error, max_y_error, max_th_error, angle_step,
                                                translation_step, &m), "create_m3rsm");
    return m;
  }

  // GridMapScanAdder::append_scan on the fine map (slamhip_map_append_scan_q), then the levels over what it wrote:
  // the cells within the longest beam (plus the blur) of the pose -- or everything, when the window has grown.
  // cos_a / sin_a: the scan's provider table (slamhip_beam_trig_cached / _raw); the heading is added by the cached
  // provider's formulas -- the reference's bits for a scan under CachedTrigonometryProvider
  void append_scan(const slamhip_scan_adder_cfg &adder, const RobotPose &pose, int n, const double *range,
                   const double *cos_a, const double *sin_a, const int *is_occ, const double *quality = nullptr) {
    const Window before = window();
    const double p3[3] = {pose.x, pose.y, pose.theta};
    long long nu = 0;
    slamhip_or_die(slamhip_map_append_scan_q(_ctx, _map_id, &adder, p3, n, range, cos_a, sin_a, is_occ, quality, &nu),
                   "map_append_scan");
    levels_behind_scan(before, adder, pose, n, range);
  }

  // The same for a scan under the reference's DEFAULT provider (RawTrigonometryProvider: cos / sin(heading + angle) per
  // point by the host's libm, slamhip_map_append_scan_raw): the reference's bits where a cell's value depends on the end
  // point continuously -- a dynamic blur scales the written occupancy by the beam's length, the area estimator by the
  // beam's chords --, which the table form reaches only to the last ulp
  void append_scan_raw(const slamhip_scan_adder_cfg &adder, const RobotPose &pose, int n, const double *range,
                       const double *angle, const int *is_occ, const double *quality = nullptr) {
    const Window before = window();
    const double p3[3] = {pose.x, pose.y, pose.theta};
    long long nu = 0;
    slamhip_or_die(slamhip_map_append_scan_raw(_ctx, _map_id, &adder, p3, n, range, angle, is_occ, quality, &nu),
                   "map_append_scan_raw");
    levels_behind_scan(before, adder, pose, n, range);
  }

  // Match::prob_upper_bound of n candidates (rotation, translation rectangle) around `pose` on the context's scan
  void bounds(const slamhip_spe_cfg &cfg, const RobotPose &pose, const std::vector<double> &rotation,
              const std::vector<LightWeightRectangle> &drift, std::vector<double> &prob_upper_bound, std::vector<int> &level) {
    const int n = (int)rotation.size();
    std::vector<double> rect(4 * (size_t)n);
    for (int i = 0; i < n; ++i) {
      rect[4 * i] = drift[i].bot();
      rect[4 * i + 1] = drift[i].top();
      rect[4 * i + 2] = drift[i].left();
      rect[4 * i + 3] = drift[i].right();
    }
    prob_upper_bound.resize(n);
    level.resize(n);
    const double p3[3] = {pose.x, pose.y, pose.theta};
    slamhip_or_die(slamhip_pyramid_score_matches(_ctx, _pyr, &cfg, p3, n, rotation.data(), rect.data(),
                                                 prob_upper_bound.data(), level.data()), "pyramid_score_matches");
  }

private:
  struct Window {
    int w = 0, h = 0, ox = 0, oy = 0;
    double scale = 1.0;
    bool operator!=(const Window &o) const { return w != o.w || h != o.h || ox != o.ox || oy != o.oy; }
  };
  Window window() const {
    Window g;
    slamhip_or_die(slamhip_map_info(_ctx, _map_id, nullptr, &g.w, &g.h, &g.ox, &g.oy, &g.scale, nullptr), "map_info");
    return g;
  }
  void levels_behind_scan(const Window &before, const slamhip_scan_adder_cfg &adder, const RobotPose &pose, int n,
                          const double *range) {
    _view->invalidate();
    const Window g = window();
    if (g != before) {
      slamhip_or_die(slamhip_pyramid_rebuild(_pyr), "pyramid_rebuild");
      return;
    }
    const double scale = g.scale;
    const int w = g.w, h = g.h, ox = g.ox, oy = g.oy;
    double reach = 0.0;
    for (int i = 0; i < n; ++i) reach = std::max(reach, std::isfinite(range[i]) ? range[i] : 0.0);
    if (std::isfinite(adder.max_range)) reach = std::min(reach, adder.max_range);
    reach += std::fabs(adder.blur) + 2 * scale;  // (a dynamic blur is a fraction of the beam: inside twice the reach)
    if (adder.blur < 0) reach *= 2;
    const int x0 = std::max(0, (int)std::floor((pose.x - reach) / scale) + ox);
    const int y0 = std::max(0, (int)std::floor((pose.y - reach) / scale) + oy);
    const int x1 = std::min(w - 1, (int)std::floor((pose.x + reach) / scale) + ox);
    const int y1 = std::min(h - 1, (int)std::floor((pose.y + reach) / scale) + oy);
    if (x1 < x0 || y1 < y0) return;
    slamhip_or_die(slamhip_pyramid_refresh(_pyr, x0, y0, x1 - x0 + 1, y1 - y0 + 1), "pyramid_refresh");
  }

  slamhip_ctx *_ctx;
  int _map_id;
  slamhip_pyramid *_pyr = nullptr;
  std::shared_ptr<HipResidentMapView> _view;
};

// The request surface of M3RSMEngine (add_scan_matching_request :291-316, then the matcher's loop around
// next_best_match, bf_multi_res_scan_matcher.h:44-65) over HipM3rsmMaps: any number of (pose, scan, map) requests, one
// search over all of them (slamhip_matcher_m3rsm_match_many), the best match of any request as the answer.  `matcher`
// (made by HipM3rsmMap::matcher: its limits, steps and cfg hold for every request) and the maps outlive the engine; the
// maps share one context.  Request k keeps its filtered scan in scan slot first_scan_slot + k.
class HipM3rsmEngine {
public:
  struct BestMatch {
    int request = -1;  // -1: no request had a valid match
    RobotPoseDelta pose_delta{0, 0, 0};
    double prob_upper_bound = std::numeric_limits<double>::quiet_NaN();
    bool is_valid() const { return request >= 0; }
  };

  // rotation_spw: the estimator's weighting where it is not `even` (VinySlamSPW, AngleHistogramReciprocalSPW) -- the
  // reference weighs prerotated points, so every request keeps one scan per rotation of the matcher's root layer
  // (hip_store_rotation_scans; request k takes the slots first_scan_slot + k * rotations ...)
  HipM3rsmEngine(slamhip_ctx *ctx, slamhip_matcher *matcher, std::shared_ptr<ScanProbabilityEstimator> spe,
                 int weighting = 0, const HipScanTrig &trig = HipScanTrig{}, int first_scan_slot = 0,
                 std::shared_ptr<ScanPointWeighting> rotation_spw = nullptr)
      : _ctx{ctx}, _matcher{matcher}, _spe{spe}, _weighting{weighting}, _trig{trig}, _first_slot{first_scan_slot},
        _rot_spw{rotation_spw} {
    slamhip_or_die(slamhip_matcher_set_m3rsm_rotation_slots(matcher, rotation_spw ? 1 : 0), "set_m3rsm_rotation_slots");
    if (rotation_spw) slamhip_or_die(slamhip_matcher_m3rsm_rotations(matcher, 0, nullptr, &_slots_per_request), "m3rsm_rotations");
  }

  void reset_engine_state() { _requests.clear(); }

  // the scan is filtered by the estimator against the map's fine level, as add_scan_matching_request does, and stored
  void add_scan_matching_request(const RobotPose &pose, const LaserScan2D &raw_scan, HipM3rsmMap &map) {
    const LaserScan2D scan = _spe->filter_scan(raw_scan, pose, map.map());
    if (_rot_spw) {
      slamhip_m3rsm_request q;
      q.pyramid = map.pyramid();
      q.scan_slot = _first_slot + int(_requests.size()) * _slots_per_request;
      q.init_pose[0] = pose.x;
      q.init_pose[1] = pose.y;
      q.init_pose[2] = pose.theta;
      hip_store_rotation_scans(_ctx, _matcher, scan, pose.theta, *_rot_spw, _trig, q.scan_slot);
      _requests.push_back(q);
      return;
    }
    const auto &pts = scan.points();
    const int n = int(pts.size());
    std::vector<double> r(n), a(n), f(n), w(n), c(n), s(n);
    for (int i = 0; i < n; ++i) {
      r[i] = pts[i].range();
      a[i] = pts[i].angle();
      f[i] = pts[i].factor();
    }
    slamhip_or_die(slamhip_scan_weights(_weighting, n, r.data(), a.data(), w.data()), "scan_weights");
    if (_trig.mode == SLAMHIP_TRIG_CACHED)
      slamhip_or_die(slamhip_beam_trig_cached(n, a.data(), _trig.a_min, _trig.a_max, _trig.a_inc, c.data(), s.data()),
                     "beam_trig_cached");
    else
      slamhip_or_die(slamhip_beam_trig_raw(n, a.data(), c.data(), s.data()), "beam_trig_raw");
    slamhip_m3rsm_request q;
    q.pyramid = map.pyramid();
    q.scan_slot = _first_slot + int(_requests.size());
    q.init_pose[0] = pose.x;
    q.init_pose[1] = pose.y;
    q.init_pose[2] = pose.theta;
    slamhip_or_die(slamhip_scan_store(_ctx, q.scan_slot, n, r.data(), c.data(), s.data(), w.data(), f.data()), "scan_store");
    // a scan under the reference's default provider: the kept points' angles go with the slot, for a matcher made with
    // SLAMHIP_POSE_TRIG_RAW_EXACT (the other modes do not read them)
    if (_trig.mode != SLAMHIP_TRIG_CACHED)
      slamhip_or_die(slamhip_scan_store_angles(_ctx, q.scan_slot, n, a.data()), "scan_store_angles");
    _requests.push_back(q);
  }

  size_t requests_nm() const { return _requests.size(); }

  // BruteForceMultiResolutionScanMatcher::process_scan's loop over every request added since the last reset
  BestMatch best_match() {
    BestMatch best;
    double delta[3] = {0, 0, 0};
    slamhip_or_die(slamhip_matcher_m3rsm_match_many(_matcher, int(_requests.size()), _requests.data(), &best.request, delta,
                                                    &best.prob_upper_bound), "m3rsm_match_many");
    best.pose_delta = RobotPoseDelta{delta[0], delta[1], delta[2]};
    return best;
  }

  // K INDEPENDENT matches: every request added since the last reset searched on its own, as K matchers' process_scan
  // would, in lock-step over shared launches (slamhip_matcher_m3rsm_match_each).  One match per request, in the order
  // added; request k's is_valid() is false where its search found nothing.
  std::vector<BestMatch> match_each() {
    const size_t n = _requests.size();
    std::vector<double> deltas(3 * n, 0.0), probs(n, 0.0);
    slamhip_or_die(slamhip_matcher_m3rsm_match_each(_matcher, int(n), _requests.data(), deltas.data(), probs.data()),
                   "m3rsm_match_each");
    std::vector<BestMatch> out(n);
    for (size_t k = 0; k < n; ++k) {
      out[k].request = probs[k] == probs[k] ? int(k) : -1;  // (NaN: no match)
      out[k].pose_delta = RobotPoseDelta{deltas[3 * k], deltas[3 * k + 1], deltas[3 * k + 2]};
      out[k].prob_upper_bound = probs[k];
    }
    return out;
  }

  // The filter parameters of the estimator (WeightedMeanPointProbabilitySPE: skip rate, usable range; bounded: the maps
  // have a rim) that match_each_raw hands the library instead of running filter_scan on the host
  void set_filter_params(unsigned skip_rate, double max_range, bool bounded) {
    _skip_rate = skip_rate;
    _max_range = max_range;
    _bounded = bounded;
    _own_filter = true;
  }

  // K INDEPENDENT matches from K RAW scans (slamhip_matcher_m3rsm_match_each_raw): request k = (poses[k], scans[k],
  // maps[k]); the library filters every scan against its map's fine level, assembles all of them on the device in one
  // launch and runs the searches of match_each -- no filter_scan, no scan_store per robot.  Needs set_filter_params, and
  // an estimator whose weighting does not turn with the candidate (rotation_spw unset: rotation-slot scans are not made
  // on the device).  The requests added with add_scan_matching_request are not touched.
  std::vector<BestMatch> match_each_raw(const std::vector<RobotPose> &poses, const std::vector<const LaserScan2D *> &scans,
                                        const std::vector<HipM3rsmMap *> &maps) {
    const size_t n = poses.size();
    if (scans.size() != n || maps.size() != n || !_own_filter || _rot_spw) {
      std::cerr << "[slamhip] HipM3rsmEngine::match_each_raw: one scan and one map per pose, filter parameters set, no "
                   "rotation weighting" << std::endl;
      std::exit(-1);
    }
    std::vector<BestMatch> out(n);
    // (a scan without points: the library asks for n > 0; the reference's answer for it is the empty scan's)
    std::vector<size_t> live;
    std::vector<slamhip_m3rsm_raw_request> req;
    std::vector<std::vector<double>> r(n), a(n), f(n);
    std::vector<std::vector<int>> occ(n);
    for (size_t k = 0; k < n; ++k) {
      const auto &pts = scans[k]->points();
      const int m = int(pts.size());
      if (m == 0) continue;
      r[k].resize(m);
      a[k].resize(m);
      f[k].resize(m);
      occ[k].resize(m);
      for (int i = 0; i < m; ++i) {
        r[k][i] = pts[i].range();
        a[k][i] = pts[i].angle();
        f[k][i] = pts[i].factor();
        occ[k][i] = pts[i].is_occupied() ? 1 : 0;
      }
      slamhip_m3rsm_raw_request q;
      q.pyramid = maps[k]->pyramid();
      q.scan = slamhip_raw_scan{m, r[k].data(), a[k].data(), occ[k].data(), f[k].data(), _trig.mode, _trig.a_min, _trig.a_max,
                                _trig.a_inc, _skip_rate, _max_range, _bounded ? 1 : 0, _weighting};
      q.init_pose[0] = poses[k].x;
      q.init_pose[1] = poses[k].y;
      q.init_pose[2] = poses[k].theta;
      req.push_back(q);
      live.push_back(k);
    }
    if (req.empty()) return out;
    std::vector<double> deltas(3 * req.size(), 0.0), probs(req.size(), 0.0);
    slamhip_or_die(slamhip_matcher_m3rsm_match_each_raw(_matcher, int(req.size()), req.data(), deltas.data(), probs.data(), nullptr),
                   "m3rsm_match_each_raw");
    for (size_t l = 0; l < live.size(); ++l) {
      BestMatch &b = out[live[l]];
      b.request = probs[l] == probs[l] ? int(live[l]) : -1;  // (NaN: no match, or the filter kept nothing)
      b.pose_delta = RobotPoseDelta{deltas[3 * l], deltas[3 * l + 1], deltas[3 * l + 2]};
      b.prob_upper_bound = probs[l];
    }
    return out;
  }

private:
  slamhip_ctx *_ctx;
  slamhip_matcher *_matcher;
  std::shared_ptr<ScanProbabilityEstimator> _spe;
  bool _own_filter = false, _bounded = false;
  unsigned _skip_rate = 0;
  double _max_range = -1;
  int _weighting;
  HipScanTrig _trig;
  int _first_slot;
  std::shared_ptr<ScanPointWeighting> _rot_spw;
  int _slots_per_request = 1;
  std::vector<slamhip_m3rsm_request> _requests;
};

// K robots' map updates and the levels behind them in shared launches: ONE slamhip_map_append_scan_batch over the maps'
// fine levels (scan k into maps[k] from poses[k]; cos_a / sin_a: the scans' provider tables, as for
// HipM3rsmMap::append_scan) and ONE slamhip_pyramid_refresh_batch over the cells each scan can have reached -- the reach
// rule of HipM3rsmMap::append_scan; a map whose window grew gets slamhip_pyramid_rebuild instead.  The maps share `ctx`
// and are distinct.  HipM3rsmMap::append_scan stays what it is for one robot.
struct HipM3rsmScan {
  int n;
  const double *range, *cos_a, *sin_a;
  const int *is_occ;
  const double *quality;  // may be null
};
inline void hip_m3rsm_append_scans(slamhip_ctx *ctx, const std::vector<HipM3rsmMap *> &maps, const slamhip_scan_adder_cfg &adder,
                                   const std::vector<RobotPose> &poses, const std::vector<HipM3rsmScan> &scans) {
  const size_t K = maps.size();
  if (poses.size() != K || scans.size() != K) {
    std::cerr << "[slamhip] hip_m3rsm_append_scans: one pose and one scan per map" << std::endl;
    std::exit(-1);
  }
  if (K == 0) return;
  struct Window {
    int w = 0, h = 0, ox = 0, oy = 0;
    double scale = 1.0;
  };
  const auto window_of = [&](int map_id) {
    Window g;
    slamhip_or_die(slamhip_map_info(ctx, map_id, nullptr, &g.w, &g.h, &g.ox, &g.oy, &g.scale, nullptr), "map_info");
    return g;
  };
  std::vector<Window> before(K);
  std::vector<slamhip_map_update_job> jobs(K);
  for (size_t k = 0; k < K; ++k) {
    before[k] = window_of(maps[k]->map_id());
    slamhip_map_update_job &j = jobs[k];
    j = slamhip_map_update_job{};
    j.map_id = maps[k]->map_id();
    j.pose[0] = poses[k].x;
    j.pose[1] = poses[k].y;
    j.pose[2] = poses[k].theta;
    j.scan_quality = adder.scan_quality;
    j.n = scans[k].n;
    j.range = scans[k].range;
    j.cos_a = scans[k].cos_a;
    j.sin_a = scans[k].sin_a;
    j.is_occ = scans[k].is_occ;
    j.quality = scans[k].quality;
  }
  std::vector<long long> n_updates(K, 0);
  slamhip_or_die(slamhip_map_append_scan_batch(ctx, &adder, int(K), jobs.data(), n_updates.data(), nullptr), "map_append_scan_batch");
  std::vector<slamhip_pyramid_refresh_job> refresh;
  for (size_t k = 0; k < K; ++k) {
    maps[k]->invalidate_view();
    const Window g = window_of(maps[k]->map_id());
    if (g.w != before[k].w || g.h != before[k].h || g.ox != before[k].ox || g.oy != before[k].oy) {
      slamhip_or_die(slamhip_pyramid_rebuild(maps[k]->pyramid()), "pyramid_rebuild");
      continue;
    }
    double reach = 0.0;
    for (int i = 0; i < scans[k].n; ++i) reach = std::max(reach, std::isfinite(scans[k].range[i]) ? scans[k].range[i] : 0.0);
    if (std::isfinite(adder.max_range)) reach = std::min(reach, adder.max_range);
    reach += std::fabs(adder.blur) + 2 * g.scale;  // (a dynamic blur is a fraction of the beam: inside twice the reach)
    if (adder.blur < 0) reach *= 2;
    const int x0 = std::max(0, (int)std::floor((poses[k].x - reach) / g.scale) + g.ox);
    const int y0 = std::max(0, (int)std::floor((poses[k].y - reach) / g.scale) + g.oy);
    const int x1 = std::min(g.w - 1, (int)std::floor((poses[k].x + reach) / g.scale) + g.ox);
    const int y1 = std::min(g.h - 1, (int)std::floor((poses[k].y + reach) / g.scale) + g.oy);
    if (x1 < x0 || y1 < y0) continue;
    refresh.push_back(slamhip_pyramid_refresh_job{maps[k]->pyramid(), x0, y0, x1 - x0 + 1, y1 - y0 + 1});
  }
  slamhip_or_die(slamhip_pyramid_refresh_batch(ctx, int(refresh.size()), refresh.data()), "pyramid_refresh_batch");
}

#endif  // SLAMHIP_M3RSM_MAP_H
