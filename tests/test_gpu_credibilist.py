"""GPU suite: the credibilist cell model (SLAMHIP_CELL_CREDIBILIST) on the device scoring path, against
tests/golden/credibilist.npz -- the reference's CredibilistCell (src/slams/credibilist/grid_cell.h) through its own scan
adder, scan probability estimators, matchers and single-hypothesis world (tests/golden/make_golden_credibilist.py).

The payload is the TBM one (u, e, o, c), updated by SLAMHIP_RULE_TBM; the per-beam probability is the cell's own,
1 - (1 - disjunctive((0, 0, 1, 0), belief).occupied()) (csrc/slamhip_internal.h credibilist_probability):
  * strict modes (beam-order sum; host pose trig = the cached provider, RAW_EXACT = the raw one) equal the reference's
    scores bit for bit, the default tree sum to 1e-12; the same for the window OOPEs;
  * the probability plane (SLAMHIP_OPT_TBM_PLANE) changes no bit of any scorer form and follows every writer;
  * the same payload bound as TBM and as CREDIBILIST scores differently, each by its own rule;
  * HC / MC traces, K6 appends and a 5-scan world loop reproduce the reference."""
import ctypes as C

import numpy as np
import pytest
from helpers import assert_trace_equal, load

import __graft_entry__ as ge

pytestmark = pytest.mark.gpu

STRICT = dict(sum_order=1, pose_trig=1)  # SLAMHIP_SUM_SEQUENTIAL, SLAMHIP_POSE_TRIG_HOST: the cached provider's bits
VACUOUS = np.array([1.0, 0.0, 0.0, 0.0])
WINDOW_OOPES = (("max", 1), ("mean", 2), ("overlap", 3))


@pytest.fixture(scope="module")
def pkg():
    return ge.load_package()


@pytest.fixture(scope="module")
def g():
    return load("credibilist.npz")


@pytest.fixture(scope="module")
def tctx(pkg):
    c = pkg.Context(0, testing=True)
    yield c
    c.close()


class Window:
    """what Context.upload_map takes"""

    def __init__(self, cell_model, payload, origin, scale):
        self.cell_model, self.payload = cell_model, np.ascontiguousarray(payload, dtype=np.float64)
        self.height, self.width = payload.shape[:2]
        self.origin, self.scale, self.unknown = (int(origin[0]), int(origin[1])), float(scale), VACUOUS


def scene_map(pkg, g, k=2, model=None):
    return Window(pkg.CELL_CREDIBILIST if model is None else model, g["map_after"][k], g["map_origin"], g["map_scale"])


def cached_trig(pkg, g, angle):
    return pkg.beam_trig(angle, pkg.TRIG_CACHED, float(g["a_min"]), float(g["a_max_passed"]), float(g["a_inc"]))


def upload_scan(pkg, ctx, g, trig="cached"):
    r, a = g[trig + "_f_range"], g[trig + "_f_angle"]
    c, s = cached_trig(pkg, g, a) if trig == "cached" else pkg.beam_trig(a)
    ctx.scan_upload(r, c, s, g[trig + "_f_weight"], g[trig + "_f_factor"])
    ctx.scan_set_angles(a)


def plane(ctx, map_id):
    valid, bad = C.c_int(-1), C.c_longlong(-1)
    assert ctx.L.slamhip_map_debug_prob_plane(ctx.h, map_id, C.byref(valid), C.byref(bad)) == 0
    return valid.value, bad.value


def both(pkg, ctx, fn):
    """fn() with the plane on and off"""
    out = []
    for on in (1, 0):
        ctx.set_option(pkg.OPT_TBM_PLANE, on)
        out.append(fn())
    ctx.set_option(pkg.OPT_TBM_PLANE, 1)
    return out


def test_bind_reports_the_model_and_rejects_what_does_not_fit_it(pkg, tctx, g):
    ctx = tctx
    ctx.upload_map(5, scene_map(pkg, g))  # (the parent: "unknown cell model")
    info = ctx.map_info(5)
    assert info["cell_model"] == pkg.CELL_CREDIBILIST == 3 and (info["width"], info["height"]) == (160, 160)
    np.testing.assert_array_equal(ctx.map_download_window(5, 0, 0, 160, 160, pkg.STRIDE[pkg.CELL_CREDIBILIST]), g["map_after"][2])
    upload_scan(pkg, ctx, g)
    with pytest.raises(pkg.SlamHipError, match="OccupancyOIE over TBM cells"):
        ctx.score_poses(5, pkg.spe_cfg(oie=pkg.OIE_OCCUPANCY), g["poses"])
    with pytest.raises(pkg.SlamHipError, match="GMAPPING OOPE needs"):
        ctx.score_poses(5, pkg.spe_cfg(oope=pkg.OOPE_GMAPPING), g["poses"])
    c, s = cached_trig(pkg, g, g["cached_f_angle"])
    for rule in (pkg.RULE_LAST, pkg.RULE_AFFINE, pkg.RULE_MEAN, pkg.RULE_GMAPPING):
        with pytest.raises(pkg.SlamHipError, match="does not fit the map's payload model"):
            ctx.map_append_scan(5, rule, g["init_pose"], g["match_range"], c, s)
        with pytest.raises(pkg.SlamHipError, match="does not fit the map's payload model"):
            ctx.map_append_scan_raw(5, rule, g["init_pose"], g["match_range"], g["cached_f_angle"])
    np.testing.assert_array_equal(ctx.map_download_window(5, 0, 0, 160, 160, 4), g["map_after"][2])
    unk = (C.c_double * 4)(1.0, 0.0, 0.0, 0.0)  # a model past the last one is still refused
    assert ctx.L.slamhip_map_bind(ctx.h, 6, pkg.CELL_CREDIBILIST + 1, 16, 16, 8, 8, C.c_double(0.05), unk) != 0
    assert b"unknown cell model" in ctx.L.slamhip_last_error()
    ctx.map_release(5)


@pytest.mark.parametrize("plane_on", [1, 0])
def test_k1_scores_equal_the_reference(pkg, tctx, g, plane_on):
    ctx = tctx
    ctx.set_option(pkg.OPT_TBM_PLANE, plane_on)
    try:
        ctx.upload_map(0, scene_map(pkg, g))
        poses = g["poses"]
        for trig, pose_trig in (("cached", pkg.POSE_TRIG_HOST), ("raw", pkg.POSE_TRIG_RAW_EXACT)):
            upload_scan(pkg, ctx, g, trig)
            want = g[trig + "_obstacle_scores"]
            assert want[2] == 0.0 and np.count_nonzero(want) == len(want) - 1  # every end point outside: the prototype cell
            strict = ctx.score_poses(0, pkg.spe_cfg(sum_order=pkg.SUM_SEQUENTIAL, pose_trig=pose_trig), poses)
            print(trig, "obstacle strict: max |diff|", np.max(np.abs(strict - want)))
            np.testing.assert_array_equal(strict, want)
            assert strict[0] == strict[1]
            for kw in (dict(), dict(pose_trig=pose_trig)):
                tree = ctx.score_poses(0, pkg.spe_cfg(**kw), poses)
                print(trig, "obstacle tree", kw, ": max rel", np.max(np.abs(tree[want != 0] / want[want != 0] - 1)))
                np.testing.assert_allclose(tree, want, rtol=1e-12, atol=0)
                assert tree[2] == 0.0
            for name, oope in WINDOW_OOPES:
                want = g["%s_%s_scores" % (trig, name)]
                assert want[2] == 0.0
                strict = ctx.score_poses(0, pkg.spe_cfg(oope=oope, area=g["area"], sum_order=pkg.SUM_SEQUENTIAL, pose_trig=pose_trig), poses)
                print(trig, name, "strict: max |diff|", np.max(np.abs(strict - want)))
                np.testing.assert_array_equal(strict, want)
                tree = ctx.score_poses(0, pkg.spe_cfg(oope=oope, area=g["area"]), poses)
                np.testing.assert_allclose(tree, want, rtol=1e-12, atol=0)
                assert tree[2] == 0.0
        assert plane(ctx, 0)[0] == plane_on
    finally:
        ctx.set_option(pkg.OPT_TBM_PLANE, 1)


MATCHERS = (("HC", [6, 0.1, 0.1]), ("MC", [20261018, 0.2, 0.1, 100, 100]),
            ("BF", [-0.1, 0.1, 0.05, -0.1, 0.1, 0.05, -0.04, 0.04, 0.02]))


def test_every_scorer_form_returns_the_same_bits_through_the_plane(pkg, tctx, g):
    ctx = tctx
    ctx.upload_map(0, scene_map(pkg, g))
    upload_scan(pkg, ctx, g)
    poses = g["poses"]
    for kw in (dict(), dict(sum_order=1), dict(pose_trig=1), dict(sum_order=1, pose_trig=1), dict(pose_trig=2),
               dict(sum_order=1, pose_trig=2)):
        on, off = both(pkg, ctx, lambda: ctx.score_poses(0, pkg.spe_cfg(**kw), poses))
        np.testing.assert_array_equal(on, off, err_msg=repr(kw))
        assert on[2] == 0.0 and np.count_nonzero(on) == len(on) - 1
    assert plane(ctx, 0) == (1, 0)
    for kind, prm in MATCHERS:
        for mode in ((2, 1, 0) if kind != "BF" else (None,)):
            def run():
                m = pkg.Matcher(ctx, kind, pkg.spe_cfg(), prm)
                if mode is not None:
                    m.set_device_chain(mode)
                t = m.process_scan(0, g["init_pose"], trace=True)
                m.close()
                return t
            on, off = both(pkg, ctx, run)
            assert_trace_equal(on, off)
            assert on["n_calls"] > 20


def test_the_plane_follows_every_writer(pkg, tctx, g):
    ctx = tctx
    ctx.upload_map(3, scene_map(pkg, g, k=0))
    upload_scan(pkg, ctx, g)
    ctx.map_set_auto_grow(3, True)
    cfg = pkg.spe_cfg()
    poses = g["poses"]
    rs = np.random.RandomState(9)
    assert plane(ctx, 3)[0] == 0  # nobody has asked yet
    ctx.score_poses(3, cfg, poses)
    assert plane(ctx, 3) == (1, 0)

    def check(what):
        assert plane(ctx, 3) == (1, 0), what
        on, off = both(pkg, ctx, lambda: ctx.score_poses(3, cfg, poses))
        np.testing.assert_array_equal(on, off, err_msg=what)
        return on

    before = check("full upload")
    blk = np.tile(np.array([0.2, 0.1, 0.6, 0.1]), (40, 50, 1)) + rs.rand(40, 50, 4) * 0.05
    ctx.map_upload_window(3, 70, 90, blk)
    assert np.any(check("partial upload") != before)
    xy = rs.randint(0, 160, (300, 2)).astype(np.int32)
    ctx.map_apply_dirty(3, xy, rs.dirichlet([1, 1, 1, 1], 300))
    check("dirty log")
    c, s = cached_trig(pkg, g, g["cached_f_angle"])
    base, blur = tuple(g["base"]), float(g["blur"])
    for path in (0, 1, 2):
        ctx.set_option(pkg.OPT_K6_PATH, path)
        for k in range(2):
            nu = ctx.map_append_scan(3, pkg.RULE_TBM, g["map_pose"][k + 1], g["map_range"][k + 1], c, s, None, quality=0.9, base=base, blur=blur)
            assert nu > 1000
            check("K6 path %d scan %d" % (path, k))
    ctx.set_option(pkg.OPT_K6_PATH, 0)
    ctx.map_append_scan_raw(3, pkg.RULE_TBM, g["map_pose"][2], g["map_range"][2], g["cached_f_angle"], None, quality=0.9, base=base, blur=blur)
    check("K6 with the raw provider")
    # a window that grows drops the plane; the next scorer call derives it again
    grown0 = ctx.map_info(3)["times_grown"]
    a16 = np.linspace(-1, 1, 16)
    ctx.map_append_scan(3, pkg.RULE_TBM, np.array([3.0, 0.0, 0.0]), np.full(16, 3.0), np.cos(a16), np.sin(a16), None, base=base)
    assert ctx.map_info(3)["times_grown"] > grown0 and plane(ctx, 3)[0] == 0
    check_scores = ctx.score_poses(3, cfg, poses)
    assert plane(ctx, 3) == (1, 0)
    ctx.set_option(pkg.OPT_TBM_PLANE, 0)
    np.testing.assert_array_equal(check_scores, ctx.score_poses(3, cfg, poses))
    ctx.set_option(pkg.OPT_TBM_PLANE, 1)
    ctx.map_release(3)


def test_the_same_payload_scores_by_the_model_it_is_bound_as(pkg, tctx, g, oracle):
    """a dispatcher that sent the new model to the TBM or OCC kernels would show here"""
    import pyoracle as po
    ctx = tctx
    ctx.upload_map(0, scene_map(pkg, g))
    ctx.upload_map(1, scene_map(pkg, g, model=pkg.CELL_TBM))
    upload_scan(pkg, ctx, g)
    poses = g["poses"]
    tbm_map = po.GridMapData(po.CELL_TBM, g["map_after"][2], g["map_origin"], float(g["map_scale"]), VACUOUS)
    c, s = cached_trig(pkg, g, g["cached_f_angle"])
    # (the oracle looks the beams' cos / sin up in the cached provider's table)
    idx = np.round((g["cached_f_angle"] - float(g["a_min"])) / float(g["a_inc"])).astype(np.int64)
    tab_cos, tab_sin = np.zeros(idx.max() + 1), np.zeros(idx.max() + 1)
    tab_cos[idx], tab_sin[idx] = c, s
    scan = po.ScanData(g["cached_f_range"], g["cached_f_angle"], g["cached_f_weight"], g["cached_f_factor"], po.TRIG_CACHED,
                       float(g["a_min"]), float(g["a_inc"]), tab_sin, tab_cos)
    want_tbm = oracle.score_poses(tbm_map, scan, po.make_cfg(), poses)
    for on in (1, 0):
        ctx.set_option(pkg.OPT_TBM_PLANE, on)
        cred = ctx.score_poses(0, pkg.spe_cfg(**STRICT), poses)
        tbm = ctx.score_poses(1, pkg.spe_cfg(**STRICT), poses)
        np.testing.assert_array_equal(cred, g["cached_obstacle_scores"])
        np.testing.assert_array_equal(tbm, want_tbm)
        assert np.all(cred != tbm)  # (a never-observed cell alone: 0 against the TBM cell's 0.5)
        for name, oope in WINDOW_OOPES:
            kw = dict(oope=oope, area=g["area"], **STRICT)
            cw, tw = ctx.score_poses(0, pkg.spe_cfg(**kw), poses), ctx.score_poses(1, pkg.spe_cfg(**kw), poses)
            np.testing.assert_array_equal(cw, g["cached_%s_scores" % name])
            np.testing.assert_array_equal(tw, oracle.score_poses(tbm_map, scan, po.make_cfg(oope=oope, area=tuple(g["area"])), poses))
            assert np.all(cw != tw)
    ctx.set_option(pkg.OPT_TBM_PLANE, 1)
    # ... and through the chains: the two maps give two different matches
    for kind, prm in MATCHERS[:2]:
        for mode in (2, 1, 0):
            ts = []
            for map_id in (0, 1):
                m = pkg.Matcher(ctx, kind, pkg.spe_cfg(**STRICT), prm)
                m.set_device_chain(mode)
                ts.append(m.process_scan(map_id, g["init_pose"], trace=True))
                m.close()
            assert_trace_equal(ts[0], golden_trace(g, kind.lower()))
            assert ts[1]["scores"][0] != ts[0]["scores"][0]
    ctx.map_release(1)


def golden_trace(g, name):
    return dict(prob=float(g[name + "_prob"]), delta=g[name + "_delta"], n_calls=int(g[name + "_n_calls"]),
                poses=g[name + "_poses"], scores=g[name + "_scores"], accepted=g[name + "_accepted"])


@pytest.mark.parametrize("kind", ["HC", "MC"])
def test_matcher_traces_equal_the_reference(pkg, tctx, g, kind):
    ctx = tctx
    ctx.upload_map(0, scene_map(pkg, g))
    upload_scan(pkg, ctx, g)
    ref = golden_trace(g, kind.lower())
    assert ref["n_calls"] > 60 and ref["accepted"].sum() >= 1
    for cfg_kw, exact in ((STRICT, True), (dict(), False)):
        traces = {}
        for mode in (0, 1, 2):
            m = pkg.Matcher(ctx, kind, pkg.spe_cfg(**cfg_kw), g[kind.lower() + "_params"])
            m.set_device_chain(mode)
            traces[mode] = m.process_scan(0, g["init_pose"], trace=True)
            m.close()
            if exact:
                assert_trace_equal(traces[mode], ref)  # bit for bit: poses, scores, accept flags, delta, prob
            else:
                assert_trace_equal(traces[mode], ref, exact_scores=False, rtol=1e-12)
        for mode in (1, 2):  # every device-chain mode is the host-driven one
            assert_trace_equal(traces[mode], traces[0])


@pytest.mark.parametrize("path", [0, 1, 2])
def test_k6_appends_reproduce_the_reference_beliefs(pkg, tctx, g, path):
    ctx = tctx
    ctx.set_option(pkg.OPT_K6_PATH, path)
    try:
        ctx.map_bind(2, pkg.CELL_CREDIBILIST, 160, 160, tuple(int(v) for v in g["map_origin"]), float(g["map_scale"]), VACUOUS)
        angle = float(g["a_min"]) + np.arange(int(g["n_beams"])) * float(g["a_inc"])
        np.testing.assert_array_equal(angle, g["cached_f_angle"])
        c, s = cached_trig(pkg, g, angle)
        base, blur = tuple(g["base"]), float(g["blur"])
        for k in range(3):
            if int(g["map_cached"][k]):
                nu = ctx.map_append_scan(2, pkg.RULE_TBM, g["map_pose"][k], g["map_range"][k], c, s, None,
                                         quality=float(g["map_quality"][k]), base=base, blur=blur)
            else:  # the raw provider's golden through the raw entry point
                nu = ctx.map_append_scan_raw(2, pkg.RULE_TBM, g["map_pose"][k], g["map_range"][k], angle, None,
                                             quality=float(g["map_quality"][k]), base=base, blur=blur)
            assert nu > 1000
            got = ctx.map_download_window(2, 0, 0, 160, 160, 4)
            print("append", k, "cells that differ:", int(np.any(got != g["map_after"][k], axis=2).sum()))
            np.testing.assert_array_equal(got, g["map_after"][k])
        assert ctx.map_info(2)["times_grown"] == 0
    finally:
        ctx.set_option(pkg.OPT_K6_PATH, 0)
        ctx.map_release(2)


def test_world_loop_reproduces_the_reference_world(pkg, tctx, g):
    """SingleStateHypothesisLaserScanGridWorld::handle_sensor_data with init_credibilist_slam's qualities, in Python:
    odometry, match, add the delta, append with 0.9 after a correction and 0.6 without one"""
    ctx = tctx
    ox, oy = (int(v) for v in g["map_origin"])
    ctx.map_bind(4, pkg.CELL_CREDIBILIST, 160, 160, (ox, oy), float(g["map_scale"]), VACUOUS)
    geom = dict(width=160, height=160, origin=(ox, oy), scale=float(g["map_scale"]), bounded=False)
    angle = float(g["a_min"]) + np.arange(int(g["n_beams"])) * float(g["a_inc"])
    c, s = cached_trig(pkg, g, angle)
    idx = np.round((angle - float(g["a_min"])) / float(g["a_inc"])).astype(np.int64)
    tab_cos, tab_sin = np.zeros(idx.max() + 1), np.zeros(idx.max() + 1)
    tab_cos[idx], tab_sin[idx] = c, s
    occ = np.ones(angle.size, np.int32)
    base, blur = tuple(g["base"]), float(g["blur"])
    pose = np.zeros(3)
    qualities = []
    for k in range(len(g["world_odom"])):
        pose = pose + g["world_odom"][k]
        rng = g["world_range"][k]
        kept = pkg.filter_scan(rng, angle, occ, pose, geom, trig_mode=pkg.TRIG_CACHED, a_min=float(g["a_min"]),
                               a_delta=float(g["a_inc"]), tab_sin=tab_sin, tab_cos=tab_cos)
        assert kept.size == angle.size
        ctx.scan_upload(rng[kept], c[kept], s[kept], pkg.scan_weights("even", rng[kept], angle[kept]))
        m = pkg.Matcher(ctx, "HC", pkg.spe_cfg(**STRICT), g["hc_params"])
        delta = m.process_scan(4, pose, trace=False)["delta"]
        m.close()
        pose = pose + delta
        corrected = bool(np.any(np.abs(delta) > 1e-7 * np.maximum(1.0, np.abs(delta))))  # RobotPoseDelta::operator bool
        qualities.append(0.9 if corrected else 0.6)
        ctx.map_append_scan(4, pkg.RULE_TBM, pose, rng, c, s, None, quality=qualities[-1], base=base, blur=blur)
        print("scan", k, "pose", pose, "golden", g["world_pose"][k])
        np.testing.assert_array_equal(pose, g["world_pose"][k])
    np.testing.assert_array_equal(qualities, g["world_quality"])
    assert set(qualities) == {0.9, 0.6}
    np.testing.assert_array_equal(ctx.map_download_window(4, 0, 0, 160, 160, 4), g["world_final"])
    ctx.map_release(4)
