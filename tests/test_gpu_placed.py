"""GPU suite: scorers, matchers and map updates FAR FROM THE WORLD ORIGIN.

Every other GPU test sits on (0, 0).  Here every scene stands at a station of tests/placed_scenes.py: O (the control: the
existing behaviour), Q1 .. Q4 (one per quadrant, 500 ... 2000 m out, headings 0.3 / 3.1 / -2.9 / 7.6) and F1 / F2 (1e5 ...
2e5 m out).  The window's origin is an index bias that lies outside the window there, floor(x / scale) runs on large and
negative quotients, rounding slacks meet coordinates whose ulp is 1e-13 ... 3e-11 m, GMapping cells carry obstacle means in
world metres, and the batch calls read origin, pose and scan per job from tables.

Held to: tests/golden/placed.npz (the compiled reference, Q stations) and the CPU oracle on the same inputs (every
station; tests/test_oracle_placed.py pins the oracle to that golden bit for bit).  Bars:
  * bit-exact modes -- beam-order sum + host pose trig against the oracle behind a provider whose table holds the
    uploaded (cos a, sin a); the tree sum against the oracle's tree order; POSE_TRIG_RAW_EXACT and the GMapping exact mode
    against the raw provider; map updates; chain == host-driven; batch == lone: equality, as near the origin;
  * non-exact modes (device sincos / exp): station O keeps the near-origin contract (1e-12, GMapping 1e-11, default-mode
    GMapping traces 1e-10).  Far out the allowance is measured on the reference side alone (placed_cases.probe): the
    oracle at each pose and at its eight neighbours one ulp away in x and / or y; 4 x the largest relative change + the
    near-origin tolerance.  A piecewise-constant scorer (1-cell, max, mean) leaves out the poses whose ORACLE score
    changes under that probe, at most 2 % of a case, and keeps 1e-12 on the rest;
  * default-mode accept traces equal the strict ones at every station."""
import ctypes as C

import numpy as np
import placed_cases as pc
import placed_scenes as ps
import pytest
from helpers import assert_trace_equal

import __graft_entry__ as ge

pytestmark = pytest.mark.gpu
STRICT = dict(sum_order=1, pose_trig=1)  # SLAMHIP_SUM_SEQUENTIAL, SLAMHIP_POSE_TRIG_HOST
HC6, HC128, HC128_TINY = [6, 0.1, 0.1], [128, 0.1, 0.1], [128, 1e-9, 1e-9]
MC = [666666, 0.2, 0.1, 20, 100]
BF = [-0.2, 0.2, 0.05, -0.2, 0.2, 0.05, -0.04, 0.04, 0.02]  # 9 x 9 x 5


@pytest.fixture(scope="module")
def pkg():
    return ge.load_package()


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def tctx(pkg):
    """a context of the library with the test hooks (slamhip_map_debug_*)"""
    c = pkg.Context(0, testing=True)
    yield c
    c.close()


@pytest.fixture(scope="module")
def po():
    import pyoracle
    return pyoracle


@pytest.fixture(scope="module")
def g():
    return pc.golden()


@pytest.fixture(scope="module")
def variant(pkg):
    v = pkg.libm_variant()
    if v < 0:
        pytest.skip("this host's libm is neither build of glibc's sin / cos / exp: no exact modes here")
    return v


def device_trig(pkg, scan):
    if getattr(scan, "trig_mode", 0) == 1:
        idx = np.round((scan.angle - scan.a_min) / scan.a_delta).astype(np.int64)
        return scan.tab_cos[idx].copy(), scan.tab_sin[idx].copy()
    return pkg.beam_trig(scan.angle)


def upload(pkg, ctx, m, scan, map_id=0):
    """map + scan; returns the oracle's view of what was uploaded: a provider whose table holds exactly the (cos a, sin a)
    the device got -- the angle-addition arithmetic of SLAMHIP_POSE_TRIG_HOST"""
    ctx.upload_map(map_id, m)
    cos_a, sin_a = device_trig(pkg, scan)
    ctx.scan_upload(scan.range, cos_a, sin_a, scan.weight, scan.factor)
    ctx.scan_set_angles(scan.angle)
    return table_scan(scan, cos_a, sin_a)


def table_scan(scan, cos_a, sin_a):
    import pyoracle as po
    return po.ScanData(scan.range, np.arange(scan.range.size, dtype=np.float64), scan.weight, scan.factor, po.TRIG_CACHED, 0.0, 1.0,
                       np.ascontiguousarray(sin_a), np.ascontiguousarray(cos_a))


def raw_scan(scan):
    import pyoracle as po
    return po.ScanData(scan.range, scan.angle, scan.weight, scan.factor)


def default_trace_equals(t, ref, oracle, po, m, oscan, ocfg, station, near_rtol=None, what=""):
    """a default-mode trace against the strict one: the same calls, poses, decisions and result pose; scores under the
    non-exact rule, the probe run over the trace's own poses in call order"""
    assert t["n_calls"] == ref["n_calls"], what
    np.testing.assert_array_equal(t["accepted"], ref["accepted"], err_msg=what)
    np.testing.assert_array_equal(t["poses"], ref["poses"], err_msg=what)
    np.testing.assert_array_equal(t["delta"], ref["delta"], err_msg=what)
    rows = pc.probe(oracle, m, oscan, ocfg, ref["poses"])
    rtol, left_out = pc.compare_non_exact(t["scores"], rows, ocfg.oope, station, what, near_rtol=near_rtol)
    if left_out:
        print("%s at %s: %.2f %% of the trace's poses left out as ill-conditioned" % (what, station, 100 * left_out))
    return rtol, left_out


# ---- scorers ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("station", ps.ALL)
def test_scorers_against_the_oracle_at_every_station(pkg, ctx, po, oracle, variant, station):
    """score_poses on the synthetic scenes: OCC at 0.1 m / 360 beams, TBM at 0.05 m / 720 beams (three 256-beam blocks;
    the probability plane on and off) -- strict, tree-sum, default, RAW_EXACT, over the 1-cell and the window OOPEs."""
    for kind in ("occ", "tbm"):
        sc = pc.scene(station, **pc.SYNTH_KINDS[kind])
        m, scan = sc["map"], sc["scan"]
        poses = pc.synth_poses(sc, kind)
        for plane in ((1, 0) if kind == "tbm" else (1,)):
            ctx.set_option(pkg.OPT_TBM_PLANE, plane)
            try:
                tab = upload(pkg, ctx, m, scan)
                for oname, oope, area, n in [("1-cell", po.OOPE_OBSTACLE, (0, 0, 0, 0), 64)] + \
                        [(nm, k, pc.WIN_AREA_SYNTH, 24) for nm, k in pc.WIN_OOPES]:
                    what = "%s %s plane %d" % (kind, oname, plane)
                    p = poses[:n]
                    strict = ctx.score_poses(0, pkg.spe_cfg(oope=oope, area=area, **STRICT), p)
                    np.testing.assert_array_equal(strict, oracle.score_poses(m, tab, po.make_cfg(oope=oope, area=area), p), err_msg=what)
                    tree = ctx.score_poses(0, pkg.spe_cfg(oope=oope, area=area, pose_trig=1), p)
                    want_tree = oracle.score_poses(m, tab, po.make_cfg(oope=oope, area=area, sum_order=po.SUM_TREE256), p)
                    np.testing.assert_array_equal(tree, want_tree, err_msg=what)
                    exact = ctx.score_poses(0, pkg.spe_cfg(oope=oope, area=area, sum_order=1, pose_trig=pkg.POSE_TRIG_RAW_EXACT), p[:24])
                    np.testing.assert_array_equal(exact, oracle.score_poses(m, raw_scan(scan), po.make_cfg(oope=oope, area=area), p[:24]),
                                                  err_msg=what)
                    dflt = ctx.score_poses(0, pkg.spe_cfg(oope=oope, area=area), p)  # (pose_trig 0: device sincos)
                    rows = pc.probe(oracle, m, tab, po.make_cfg(oope=oope, area=area), p)
                    np.testing.assert_array_equal(rows[0], strict)
                    pc.compare_non_exact(dflt, rows, oope, station, what)
                    assert dflt[0] == dflt[1] and strict[0] == strict[1]  # identical poses -> identical bits
                    assert len(np.unique(strict)) > n // 2  # (the scene tells the poses apart)
            finally:
                ctx.set_option(pkg.OPT_TBM_PLANE, 1)


@pytest.mark.parametrize("station", ps.ALL)
def test_gmapping_scorer_against_the_oracle_at_every_station(pkg, ctx, po, oracle, variant, station):
    """The GMapping OOPE: obstacle means in world metres.  Exact mode == the oracle, bit for bit, cache included; host trig
    + device exp within the allowance."""
    sc = pc.scene(station, **pc.SYNTH_KINDS["gm"])
    m, scan = sc["map"], sc["scan"]
    poses = pc.synth_poses(sc, "gm")
    upload(pkg, ctx, m, scan)
    ocfg = po.make_cfg(oope=po.OOPE_GMAPPING)
    cache = po.Oracle.new_gm_cache()
    want = oracle.score_poses(m, raw_scan(scan), ocfg, poses, cache)
    ctx.gm_cache_reset()
    exact = ctx.score_poses(0, pkg.spe_cfg(oope=pkg.OOPE_GMAPPING, sum_order=1, pose_trig=pkg.POSE_TRIG_RAW_EXACT), poses)
    np.testing.assert_array_equal(exact, want)
    cx, cy, pr = ctx.gm_cache_get()
    assert (cx, cy, pr) == (cache.cx, cache.cy, cache.prob)
    assert len(np.unique(want)) > 40 and want.min() > 0
    rows = pc.probe(oracle, m, raw_scan(scan), ocfg, poses)
    for pose_trig in (1, 0):
        ctx.gm_cache_reset()
        got = ctx.score_poses(0, pkg.spe_cfg(oope=pkg.OOPE_GMAPPING, pose_trig=pose_trig), poses)
        pc.compare_non_exact(got, rows, po.OOPE_GMAPPING, station, "gmapping pose_trig %d" % pose_trig)
        cx, cy, pr = ctx.gm_cache_get()
        assert (cx, cy) == (cache.cx, cache.cy)


@pytest.mark.parametrize("station", ps.Q_STATIONS)
def test_scorers_against_the_reference_golden(pkg, ctx, po, oracle, variant, g, station):
    """The reference's own scores on the reference's own maps, cached and raw provider."""
    st = station
    for tname, trig in (("cached", po.TRIG_CACHED), ("raw", po.TRIG_RAW)):
        for name, weighting in (("mean", "even"), ("tbm", "viny")):
            m, scan = pc.final_map(g, st, name), pc.golden_scan(g, st, trig, weighting)
            tab = upload(pkg, ctx, m, scan)
            key = "%s_%s_%s_" % (st, name, tname)
            poses = g[st + "_poses"]
            strict = ctx.score_poses(0, pkg.spe_cfg(**STRICT), poses)
            np.testing.assert_array_equal(strict, g[key + "scores"], err_msg=key)  # bit-exact with the reference
            rows = pc.probe(oracle, m, tab, po.make_cfg(), poses)
            pc.compare_non_exact(ctx.score_poses(0, pkg.spe_cfg(), poses), rows, po.OOPE_OBSTACLE, st, key)
            for kname, kind in pc.WIN_OOPES:
                ocfg = po.make_cfg(oope=kind, area=g["win_area"])
                got = ctx.score_poses(0, pkg.spe_cfg(oope=kind, area=g["win_area"], **STRICT), poses[:24])
                rows = pc.probe(oracle, m, tab, ocfg, poses[:24])  # the oracle in the arithmetic of the upload
                np.testing.assert_array_equal(rows[0], got, err_msg=key + kname)
                if trig == po.TRIG_CACHED or kname != "overlap":
                    np.testing.assert_array_equal(got, g[key + "win_" + kname], err_msg=key + kname)
                else:  # host trig against libm's sin(theta + a): one ulp of an end point, and overlap weights are continuous
                    rows_raw = pc.probe(oracle, m, scan, ocfg, poses[:24])
                    np.testing.assert_array_equal(rows_raw[0], g[key + "win_" + kname])
                    pc.compare_non_exact(got, rows_raw, kind, st, key + kname + " host trig")
                dflt = ctx.score_poses(0, pkg.spe_cfg(oope=kind, area=g["win_area"]), poses[:24])
                pc.compare_non_exact(dflt, rows, kind, st, key + kname)
            if trig == po.TRIG_RAW:
                exact = pkg.spe_cfg(sum_order=1, pose_trig=pkg.POSE_TRIG_RAW_EXACT)
                np.testing.assert_array_equal(ctx.score_poses(0, exact, poses[:24]), g[key + "scores"][:24], err_msg=key)
                for kname, kind in pc.WIN_OOPES:
                    cfg = pkg.spe_cfg(oope=kind, area=g["win_area"], sum_order=1, pose_trig=pkg.POSE_TRIG_RAW_EXACT)
                    np.testing.assert_array_equal(ctx.score_poses(0, cfg, poses[:24]), g[key + "win_" + kname], err_msg=key + kname)
        # the GMapping OOPE on the reference's GMapping map
        m, scan = pc.final_map(g, st, "gmapping"), pc.golden_scan(g, st, trig)
        upload(pkg, ctx, m, scan)
        want = g["%s_gmapping_%s_scores" % (st, tname)]
        rows = pc.probe(oracle, m, scan, po.make_cfg(oope=po.OOPE_GMAPPING), g[st + "_gm_poses"])
        np.testing.assert_array_equal(rows[0], want)
        ctx.gm_cache_reset()
        got = ctx.score_poses(0, pkg.spe_cfg(oope=pkg.OOPE_GMAPPING, pose_trig=1), g[st + "_gm_poses"])
        pc.compare_non_exact(got, rows, po.OOPE_GMAPPING, st, "gmapping " + tname)
        if trig == po.TRIG_RAW:
            ctx.gm_cache_reset()
            exact = ctx.score_poses(0, pkg.spe_cfg(oope=pkg.OOPE_GMAPPING, sum_order=1, pose_trig=pkg.POSE_TRIG_RAW_EXACT), g[st + "_gm_poses"])
            np.testing.assert_array_equal(exact, want)


# ---- matchers -----------------------------------------------------------------------------------------------------------------
def three_rules(pkg, ctx, po, oracle, kind, okind, prm, m, oscan, init, station, what):
    """chain == host-driven bit for bit (tie check off); strict == oracle; default (checked) == the strict accept trace"""
    if kind != "BF":
        runs = {}
        for mode in (2, 1, 0):
            mt = pkg.Matcher(ctx, kind, pkg.spe_cfg(), prm)
            mt.set_device_chain(mode)
            mt.set_tie_check(0)
            runs[mode] = [mt.process_scan(0, init + k * np.array([0.013, -0.007, 0.004]), trace=True) for k in range(2)]
            if mode == 2:
                assert mt.resident_stats() == dict(matches=2, gave_up=0), what
            assert (mt.stats()["kernels_launched"] > 0) == (mode != 0), what
            mt.close()
        for mode in (2, 1):
            for a, b in zip(runs[mode], runs[0]):
                assert_trace_equal(a, b)
    ref = oracle.process_scan(oracle.enumerator(okind, prm), m, oscan, po.make_cfg(), init)
    strict = pkg.Matcher(ctx, kind, pkg.spe_cfg(**STRICT), prm)
    assert_trace_equal(strict.process_scan(0, init, trace=True), ref)
    strict.close()
    for mode in ((2, 1, 0) if kind != "BF" else (None,)):
        mt = pkg.Matcher(ctx, kind, pkg.spe_cfg(), prm)
        if mode is not None:
            mt.set_device_chain(mode)
        default_trace_equals(mt.process_scan(0, init, trace=True), ref, oracle, po, m, oscan, po.make_cfg(), station,
                             what="%s mode %r" % (what, mode))
        mt.close()
    return ref


@pytest.mark.parametrize("station", ps.ALL)
def test_matchers_against_the_oracle_at_every_station(pkg, ctx, po, oracle, station):
    """HC and MC in device-chain modes 2, 1 and 0, and BF, on the synthetic scenes (OCC: one 256-beam block and a part;
    TBM: 720 beams, VinySlam weights)."""
    for kind in ("occ", "tbm"):
        sc = pc.scene(station, **pc.SYNTH_KINDS[kind])
        tab = upload(pkg, ctx, sc["map"], sc["scan"])
        for mk, okind, prm in (("HC", po.SM_HC, HC6), ("MC", po.SM_MC, MC)) + ((("BF", po.SM_BF, BF),) if kind == "occ" else ()):
            ref = three_rules(pkg, ctx, po, oracle, mk, okind, prm, sc["map"], tab, sc["init_pose"], station, "%s %s" % (kind, mk))
            assert ref["accepted"][1:].any() or mk == "MC", (kind, mk)


@pytest.mark.parametrize("station", ps.Q_STATIONS)
def test_matchers_against_the_reference_golden(pkg, ctx, po, oracle, variant, g, station):
    st = station
    m, scan = pc.final_map(g, st, "mean"), pc.golden_scan(g, st, po.TRIG_CACHED)
    tab = upload(pkg, ctx, m, scan)
    init = g[st + "_init_pose"]
    for name, kind, prm in (("hc6", "HC", HC6), ("hc128", "HC", HC128), ("hc128tiny", "HC", HC128_TINY), ("mc", "MC", MC), ("bf", "BF", BF)):
        ref = pc.trace(g, "%s_mean_cached_%s_" % (st, name))
        np.testing.assert_array_equal(g[{"mc": "mc_params", "bf": "bf_params"}.get(name, name + "_params")], prm)
        strict = pkg.Matcher(ctx, kind, pkg.spe_cfg(**STRICT), prm)
        assert_trace_equal(strict.process_scan(0, init, trace=True), ref)  # bit-exact: poses, scores, accept flags, delta, prob
        strict.close()
        for mode in ((2, 1, 0) if kind != "BF" else (None,)):
            mt = pkg.Matcher(ctx, kind, pkg.spe_cfg(), prm)
            if mode is not None:
                mt.set_device_chain(mode)
            default_trace_equals(mt.process_scan(0, init, trace=True), ref, oracle, po, m, tab, po.make_cfg(), st, what="%s %s mode %r" % (st, name, mode))
            mt.close()
    # the raw provider on the TBM map: host trig takes the reference's accept path bit for bit here as near the origin, the
    # restated libm is the raw provider itself
    m, scan = pc.final_map(g, st, "tbm"), pc.golden_scan(g, st, po.TRIG_RAW, "viny")
    upload(pkg, ctx, m, scan)
    ref = pc.trace(g, st + "_tbm_raw_hc6_")
    for cfg in (pkg.spe_cfg(**STRICT), pkg.spe_cfg(sum_order=1, pose_trig=pkg.POSE_TRIG_RAW_EXACT)):
        mt = pkg.Matcher(ctx, "HC", cfg, HC6)
        assert_trace_equal(mt.process_scan(0, init, trace=True), ref)
        mt.close()
    # hill climbing over the GMapping OOPE: exact mode == the reference; the checked default mode walks its accept path
    m, scan = pc.final_map(g, st, "gmapping"), pc.golden_scan(g, st, po.TRIG_RAW)
    upload(pkg, ctx, m, scan)
    ref = pc.trace(g, st + "_gmapping_raw_hc6_")
    mt = pkg.Matcher(ctx, "HC", pkg.spe_cfg(oope=pkg.OOPE_GMAPPING, sum_order=1, pose_trig=pkg.POSE_TRIG_RAW_EXACT), HC6)
    ctx.gm_cache_reset()
    assert_trace_equal(mt.process_scan(0, init, trace=True), ref)
    mt.close()
    gm_default_modes(pkg, ctx, po, oracle, m, scan, init, ref, st)


def gm_default_modes(pkg, ctx, po, oracle, m, scan, init, ref, station):
    """the checked default mode of the GMapping OOPE in modes 2, 1, 0: the exact accept trace; scores bit-equal where the
    match was redone in the exact mode, within the allowance elsewhere"""
    ocfg = po.make_cfg(oope=po.OOPE_GMAPPING)
    for mode in (2, 1, 0):
        mt = pkg.Matcher(ctx, "HC", pkg.spe_cfg(oope=pkg.OOPE_GMAPPING), HC6)
        mt.set_device_chain(mode)
        ctx.gm_cache_reset()
        t = mt.process_scan(0, init, trace=True)
        what = "gmapping default mode %d at %s" % (mode, station)
        if mt.stats()["steps_rescored"] > 0:
            print(what + ": a comparison inside the unsettled band, the match was redone in the exact mode")
            assert_trace_equal(t, ref)
        else:
            default_trace_equals(t, ref, oracle, po, m, raw_scan(scan), ocfg, station, near_rtol=1e-10, what=what)
        if mode == 2:
            assert mt.resident_stats()["gave_up"] == 0
        mt.close()


@pytest.mark.parametrize("station", ps.ALL)
def test_gmapping_oope_chain_at_every_station(pkg, ctx, po, oracle, variant, station):
    """hc_resident_gm / hc_chain's GMapping form / host-driven: chain == host-driven bit for bit, cache included; exact ==
    the oracle; default (checked) == the exact accept trace."""
    sc = pc.scene(station, **pc.SYNTH_KINDS["gm"])
    m, scan = sc["map"], sc["scan"]
    upload(pkg, ctx, m, scan)
    cfg = pkg.spe_cfg(oope=pkg.OOPE_GMAPPING)
    runs = {}
    for mode in (2, 1, 0):
        mt = pkg.Matcher(ctx, "HC", cfg, HC6)
        mt.set_device_chain(mode)
        mt.set_tie_check(0)
        out, init = [], sc["init_pose"]
        for rep in range(2):
            ctx.gm_cache_reset() if rep == 0 else ctx.gm_cache_set(*out[-1][1])
            t = mt.process_scan(0, init, trace=True)
            out.append((t, ctx.gm_cache_get()))
            init = init + np.array([0.011, -0.006, 0.003])
        runs[mode] = out
        mt.close()
    for mode in (2, 1):
        for (a, ca), (b, cb) in zip(runs[mode], runs[0]):
            assert_trace_equal(a, b)
            assert ca == cb
    ref = oracle.process_scan(oracle.enumerator(po.SM_HC, HC6), m, raw_scan(scan), po.make_cfg(oope=po.OOPE_GMAPPING), sc["init_pose"],
                              cache=po.Oracle.new_gm_cache())
    assert ref["accepted"][1:].any()
    mt = pkg.Matcher(ctx, "HC", pkg.spe_cfg(oope=pkg.OOPE_GMAPPING, sum_order=1, pose_trig=pkg.POSE_TRIG_RAW_EXACT), HC6)
    ctx.gm_cache_reset()
    assert_trace_equal(mt.process_scan(0, sc["init_pose"], trace=True), ref)
    mt.close()
    gm_default_modes(pkg, ctx, po, oracle, m, scan, sc["init_pose"], ref, station)


# ---- closed-form tails --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prm", [HC128, HC128_TINY], ids=["steps0.1", "steps1e-9"])
@pytest.mark.parametrize("station", ps.ALL)
def test_closed_form_tails_at_every_station(pkg, ctx, po, oracle, station, prm):
    """SLAMHIP_OPT_INERT_TAIL 2, 1 and 0: assert-equal traces, and the calls ended in closed form against a count read off
    the ORACLE's trace -- its trailing calls whose pose IS the best pose.  Level 1 (identical poses) can skip none but
    those, and it looks for them at the root of a super-step: a super-step speculates on at most kHcMaxInst = 64 rounds
    (csrc/hc_chain.h), so up to 6 x 64 calls of the oracle's tail may have been scored before it is noticed, never more.
    The certificate of level 2 may skip more (poses that differ but cannot move an end point), never fewer.  A tail is
    required only where the oracle's trace has one: far out with |h| < 0.5 the heading's ulp stays small while x and y
    stop moving, identical poses come later -- the reference's behaviour."""
    sc = pc.scene(station, **pc.SYNTH_KINDS["occ"])
    tab = upload(pkg, ctx, sc["map"], sc["scan"])
    ref = oracle.process_scan(oracle.enumerator(po.SM_HC, prm), sc["map"], tab, po.make_cfg(), sc["init_pose"])
    tail = pc.oracle_tail(ref)
    res = {}
    for level in (2, 1, 0):
        ctx.set_option(pkg.OPT_INERT_TAIL, level)
        try:
            mt = pkg.Matcher(ctx, "HC", pkg.spe_cfg(), prm)
            res[level] = (mt.process_scan(0, sc["init_pose"], trace=True), mt.stats())
            assert mt.resident_stats() == dict(matches=1, gave_up=0)
            mt.close()
        finally:
            ctx.set_option(pkg.OPT_INERT_TAIL, 2)
    print("closed-form tail at %s %r: oracle %d of %d calls, level 2 %d, level 1 %d" % (
        station, prm, tail, ref["n_calls"], res[2][1]["calls_closed_form"], res[1][1]["calls_closed_form"]))
    for level in (2, 1):
        assert_trace_equal(res[level][0], res[0][0])
        assert res[level][1]["scorer_calls"] == res[0][1]["scorer_calls"] == ref["n_calls"]
    default_trace_equals(res[0][0], ref, oracle, po, sc["map"], tab, po.make_cfg(), station, what="tail")
    c2, c1, c0 = (res[lv][1]["calls_closed_form"] for lv in (2, 1, 0))
    assert c0 == 0 and c1 <= tail and c2 >= c1
    if tail > 6 * 64:
        assert c1 >= tail - 6 * 64, "level 1 scored %d calls the oracle shows to be the best pose itself" % (tail - c1)


# ---- the certificate, next to cell edges --------------------------------------------------------------------------------------
@pytest.mark.parametrize("station", ["Q3", "F1"])
def test_certificate_with_end_points_placed_next_to_cell_edges_far_out(pkg, ctx, station):
    """tests/test_gpu_hc_chain.py's provocation of the certificate's bound with its poses moved to Q3 and F1: a map of
    random occupancies, scans of 1 ... 12 beams whose first end points are PLACED 4 ... 1e9 ulps OF THE END-POINT COORDINATE
    from a cell edge (a fixed 1e-13 m is below one ulp out there), hill climbers with steps on either side of that
    distance.  100 matches at SLAMHIP_OPT_INERT_TAIL 2 and 0: traces assert-equal."""
    from synth import CELL_OCC, MapData
    (kx, ky), _ = ps.STATIONS[station]
    rs = np.random.RandomState(2024 + kx % 97)
    scale = 0.1
    shift = ps.shift_m(station, scale)
    m = MapData(CELL_OCC, rs.rand(300, 300), (150 - kx, 150 - ky), scale, [0.5])
    ctx.upload_map(0, m)
    n_closed = n_acc_late = 0
    for it in range(100):
        nb = int(rs.choice([1, 2, 3, 6, 12]))
        pose = np.array([rs.uniform(-3, 3), rs.uniform(-3, 3), rs.uniform(-3.1, 3.1)]) + shift
        ang = rs.uniform(-2.3, 2.3, nb)
        rng = rs.uniform(0.5, 12.0, nb)
        if it % 3 == 0:
            rng[0] = rs.uniform(10.0, 25.0)  # (a long beam: the rotation candidates' lever)
        for b in range(min(nb, 2)):
            c, s = np.cos(pose[2] + ang[b]), np.sin(pose[2] + ang[b])
            ulps = 10.0 ** rs.uniform(np.log10(4.0), 9.0) * rs.choice([-1.0, 1.0])
            if rs.rand() < 0.5 and abs(c) > 0.2:
                e = pose[0] + rng[b] * c
                edge = np.round(e / scale) * scale
                rng[b] = (edge + ulps * np.spacing(abs(e)) - pose[0]) / c
            elif abs(s) > 0.2:
                e = pose[1] + rng[b] * s
                edge = np.round(e / scale) * scale
                rng[b] = (edge + ulps * np.spacing(abs(e)) - pose[1]) / s
            rng[b] = abs(rng[b])
        cos_a, sin_a = pkg.beam_trig(ang)
        ctx.scan_upload(rng, cos_a, sin_a, np.full(nb, 1.0 / nb), np.ones(nb))
        prm = [int(rs.choice([60, 128])), 10.0 ** rs.uniform(-7, -2), 10.0 ** rs.uniform(-7, -2)]
        res = {}
        for level in (2, 0):
            ctx.set_option(pkg.OPT_INERT_TAIL, level)
            try:
                mm = pkg.Matcher(ctx, "HC", pkg.spe_cfg(), prm)
                res[level] = (mm.process_scan(0, pose, trace=True), mm.stats())
                assert mm.resident_stats()["gave_up"] == 0
                mm.close()
            finally:
                ctx.set_option(pkg.OPT_INERT_TAIL, 2)
        (a, sa), (b_, sb) = res[2], res[0]
        assert_trace_equal(a, b_)
        assert a["prob"] == b_["prob"] and np.array_equal(a["delta"], b_["delta"]) and a["n_calls"] == b_["n_calls"]
        n_closed += sa["calls_closed_form"] > 0
        n_acc_late += int(np.count_nonzero(a["accepted"][1:]) > 0)
    print("certificate at %s: %d of 100 matches ended in closed form, %d accepted a candidate" % (station, n_closed, n_acc_late))
    assert n_closed >= 50 and n_acc_late >= 10


# ---- the raw route ------------------------------------------------------------------------------------------------------------
def scan_download(ctx):
    fn = ctx.L.slamhip_scan_download
    dp = C.POINTER(C.c_double)
    fn.argtypes = [C.c_void_p, C.c_int, dp, C.POINTER(C.c_int)]
    n = C.c_int(-1)
    assert fn(ctx.h, 0, None, C.byref(n)) == 0
    out = np.full((5, max(n.value, 1)), np.nan)
    assert fn(ctx.h, out.shape[1], out.ctypes.data_as(dp), C.byref(n)) == 0
    return out[:, :n.value].view(np.uint64)


@pytest.mark.parametrize("station", ps.ALL)
def test_raw_scan_route_at_every_station(pkg, ctx, po, oracle, station):
    """process_raw_scan = the oracle's filter_scan + the oracle's match, at the station."""
    sc = pc.scene(station, raw=True, **pc.SYNTH_KINDS["occ"])
    m = sc["map"]
    r, a, occ = sc["raw"]
    occ = occ.copy()
    occ[4::9] = 0  # (max-range readings: the filter has something to drop)
    ctx.upload_map(0, m)
    kept = oracle.filter_scan(m, r, a, occ, sc["init_pose"])
    assert 100 < len(kept) == occ.sum() < r.size
    fs = po.ScanData(r[kept], a[kept])
    tab = table_scan(fs, *pkg.beam_trig(fs.angle))
    ref = oracle.process_scan(oracle.enumerator(po.SM_HC, HC6), m, tab, po.make_cfg(), sc["init_pose"])
    strict = pkg.Matcher(ctx, "HC", pkg.spe_cfg(**STRICT), HC6)
    match = strict.make_raw_process_scan(0, r, a, is_occ=occ)
    n, prob = match(sc["init_pose"])
    assert n == len(kept) and prob == ref["prob"] and np.array_equal(np.array(list(match.delta)), ref["delta"])
    blk = scan_download(ctx).view(np.float64)
    np.testing.assert_array_equal(blk[0], fs.range)
    np.testing.assert_array_equal(blk[3], fs.weight)
    strict.close()
    rows = pc.probe(oracle, m, tab, po.make_cfg(), sc["init_pose"] + ref["delta"])
    for opt in (1, 0):
        ctx.set_option(pkg.OPT_RAW_PROLOGUE, opt)
        try:
            mt = pkg.Matcher(ctx, "HC", pkg.spe_cfg(), HC6)
            match = mt.make_raw_process_scan(0, r, a, is_occ=occ)
            n, prob = match(sc["init_pose"])
            assert n == len(kept) and np.array_equal(np.array(list(match.delta)), ref["delta"])
            assert mt.stats()["scorer_calls"] == ref["n_calls"] and mt.resident_stats() == dict(matches=1, gave_up=0)
            pc.compare_non_exact(np.array([prob]), rows, po.OOPE_OBSTACLE, station, "raw route")
            mt.close()
        finally:
            ctx.set_option(pkg.OPT_RAW_PROLOGUE, 1)


@pytest.mark.parametrize("station", ["Q2", "F2"])
def test_raw_prologue_forms_far_out(pkg, ctx, station):
    """tests/test_gpu_raw_prologue.py's comparison at Q2 and F2: the chain assembling the raw scan in its own prologue
    against the assembly kernel in front of it -- scan block, points kept, delta, probability, scorer calls as bit patterns
    -- for 1 / 255 / 256 / 257 / 1025 / all beams kept, workgroups of 256 and 1024 threads, both providers."""
    sc = pc.scene(station, cell_model=0, scale=0.1, n_beams=1080, raw=True)
    r, a, _occ = sc["raw"]
    n_raw = r.size
    inc, a_min = a[1] - a[0], a[0]
    acc, v = [], a_min
    while len(acc) < n_raw:  # the cached provider's own angles: every table index is exact
        acc.append(v)
        v += inc
    a = np.array(acc)
    r = np.minimum(r, 25.0)
    ctx.upload_map(0, sc["map"])
    rs = np.random.RandomState(5)
    ms = {}
    for nt in (256, 1024):
        for opt in (1, 0):
            ms[nt, opt] = pkg.Matcher(ctx, "HC", pkg.spe_cfg(), [40, 0.1, 0.1])
            ms[nt, opt].set_device_chain(2, nt)
    try:
        for nt in (256, 1024):
            for k, trig, weighting in ((1, "raw", "even"), (255, "cached", "viny"), (256, "raw", "ahr"), (257, "cached", "even"),
                                       (1025, "raw", "viny"), (n_raw, "cached", "ahr")):
                occ = np.zeros(n_raw, np.int32)
                occ[rs.choice(n_raw, k, replace=False)] = 1
                out = {}
                for opt in (1, 0):
                    ctx.set_option(pkg.OPT_RAW_PROLOGUE, opt)
                    before = ctx.get_option(pkg.OPT_RAW_PROLOGUE_MATCHES)
                    match = ms[nt, opt].make_raw_process_scan(0, r, a, is_occ=occ, factor=0.5 + np.arange(n_raw) / n_raw,
                                                              trig_mode=pkg.TRIG_CACHED if trig == "cached" else pkg.TRIG_RAW,
                                                              a_min=a_min, a_max=a_min + inc * n_raw + inc, a_inc=inc, weighting=weighting)
                    kept, prob = match(sc["init_pose"])
                    assert ctx.get_option(pkg.OPT_RAW_PROLOGUE_MATCHES) - before == opt
                    out[opt] = dict(kept=kept, prob=np.float64(prob).view(np.uint64), delta=np.array(list(match.delta)).view(np.uint64),
                                    scan=scan_download(ctx), calls=ms[nt, opt].stats()["scorer_calls"])
                assert out[1]["kept"] == out[0]["kept"] == k
                for key in out[1]:
                    assert np.array_equal(out[1][key], out[0][key]), (nt, k, key)
        for m_ in ms.values():
            assert m_.resident_stats()["gave_up"] == 0
    finally:
        ctx.set_option(pkg.OPT_RAW_PROLOGUE, 1)
        for m_ in ms.values():
            m_.close()


# ---- mixed batches: one job per station, each on its own map, in ONE call -----------------------------------------------------
def station_jobs(pkg, ctx, raw=False):
    """job k stands at station k, on map k; scales alternate, so no two neighbours share origin, scale, pose or scan"""
    jobs = []
    for k, st in enumerate(ps.ALL):
        kw = dict(cell_model=0, scale=(0.1, 0.05)[k % 2], n_beams=(360, 450, 720)[k % 3])
        sc = pc.scene(st, raw=raw, **kw)
        ctx.upload_map(k, sc["map"])
        if raw:
            r, a, occ = sc["raw"]
            jobs.append(dict(map_id=k, range=r, angle=a, is_occ=occ, init_pose=sc["init_pose"], weighting=("even", "viny")[k % 2]))
        else:
            c, s = pkg.beam_trig(sc["scan"].angle)
            jobs.append(dict(map_id=k, range=sc["scan"].range, cos_a=c, sin_a=s, weight=sc["scan"].weight, init_pose=sc["init_pose"]))
    return jobs


def lone_match(ctx, mt, job):
    ctx.scan_upload(job["range"], job["cos_a"], job["sin_a"], job["weight"], np.ones(np.size(job["range"])))
    return mt.process_scan(job["map_id"], job["init_pose"], trace=True)


def test_mixed_batch_of_matches_one_per_station(pkg, ctx):
    """process_scan_batch with K = 7 jobs, one per station: job k is, bit for bit, the lone call at its station -- in the
    listed order and reversed.  A job reading its neighbour's table row (origin, scale, pose, scan) lands in another
    quadrant."""
    jobs = station_jobs(pkg, ctx)
    lone = pkg.Matcher(ctx, "HC", pkg.spe_cfg(), HC6)
    want = [lone_match(ctx, lone, j) for j in jobs]
    assert len({(w["n_calls"],) + tuple(w["delta"]) for w in want}) >= 4  # (the stations' matches differ: a swap would show)
    mb = pkg.Matcher(ctx, "HC", pkg.spe_cfg(), HC6)
    for order in (list(range(len(jobs))), list(range(len(jobs)))[::-1]):
        got = mb.process_scan_batch([jobs[k] for k in order], trace=True)
        for i, k in enumerate(order):
            assert_trace_equal(got[i], want[k])
            assert mb.batch_stats(i)["on_device_chain"], (order, i)
    lone.close()
    mb.close()


def test_mixed_batch_of_raw_scans_one_per_station(pkg, ctx):
    """process_raw_scan_batch: filter + assembly + match of K = 7 raw scans, one per station, in one call."""
    jobs = station_jobs(pkg, ctx, raw=True)
    want = []
    for j in jobs:
        lone = pkg.Matcher(ctx, "HC", pkg.spe_cfg(), HC6)
        match = lone.make_raw_process_scan(j["map_id"], j["range"], j["angle"], is_occ=j["is_occ"], weighting=j["weighting"])
        kept, prob = match(j["init_pose"])
        want.append(dict(kept=kept, prob=prob, delta=np.array(list(match.delta)), scan=scan_download(ctx), calls=lone.stats()["scorer_calls"]))
        lone.close()
    assert len({(w["calls"],) + tuple(w["delta"]) for w in want}) >= 4
    mb = pkg.Matcher(ctx, "HC", pkg.spe_cfg(), HC6)
    for order in (list(range(len(jobs))), list(range(len(jobs)))[::-1]):
        got = mb.process_raw_scan_batch([jobs[k] for k in order], trace=True)
        for i, k in enumerate(order):
            assert got[i]["kept"] == want[k]["kept"] and got[i]["prob"] == want[k]["prob"], (order, i)
            np.testing.assert_array_equal(got[i]["delta"], want[k]["delta"])
            assert got[i]["n_calls"] == want[k]["calls"]
            np.testing.assert_array_equal(mb.batch_scan_download(i).view(np.uint64), want[k]["scan"])
    mb.close()


def test_mixed_batch_on_monte_carlo_engine_streams(pkg, ctx):
    """set_mc_streams: K = 7 engines, station k on stream k in both calls (the second call lists the jobs in reverse and
    maps them back to their streams); each job is the lone matcher with its seed, first and second match."""
    jobs = station_jobs(pkg, ctx)
    seeds = [666666 + 17 * k for k in range(len(jobs))]
    lones = [pkg.Matcher(ctx, "MC", pkg.spe_cfg(), [s] + MC[1:]) for s in seeds]
    mb = pkg.Matcher(ctx, "MC", pkg.spe_cfg(), MC)
    mb.set_mc_streams(seeds)
    for call, order in enumerate((list(range(len(jobs))), list(range(len(jobs)))[::-1])):
        mb.set_mc_job_streams(order if call else None)
        got = mb.process_scan_batch([jobs[k] for k in order], trace=True)
        for i, k in enumerate(order):
            assert_trace_equal(got[i], lone_match(ctx, lones[k], jobs[k]))
    assert [mb.mc_stream_info(k)["matches"] for k in range(len(jobs))] == [2] * len(jobs)
    for m_ in lones + [mb]:
        m_.close()


# ---- map updates --------------------------------------------------------------------------------------------------------------
def bind_fresh(pkg, ctx, g, st, name, map_id):
    cell_model, rule = pc.CLASSES[name]
    w, h, origin = pc.window_geometry(g, st)
    try:
        ctx.map_release(map_id)
    except pkg.SlamHipError:
        pass  # (nothing bound under this id)
    ctx.map_bind(map_id, cell_model, w, h, origin, float(g["scale"]), g["%s_%s_unknown" % (st, name)][:pc.STRIDE[cell_model]])
    return cell_model, rule, w, h


def device_adder(g, name, est):
    kw, ex = pc.adder_args(g, name, est)
    return dict(kw, **(dict(estimator=1, shift_amount=ex["shift_amount"]) if est else {}))


def check_snapshot(ctx, g, st, name, est, k, map_id, raw, cell_model, rule, w, h):
    """a snapshot against the golden at the bars of tests/test_gpu_mapupdate*.py: raw provider bit for bit; cached-provider
    arithmetic: const estimator bit for bit but GMapping's obstacle means (1e-13), area estimator 1e-11; counters exact"""
    if not pc.has_snapshot(g, st, name, est, k):
        return 0
    t = pc.tag(st, name, est, k)
    got, want = ctx.map_download_window(map_id, 0, 0, w, h, pc.STRIDE[cell_model]), g[t + "payload"]
    if raw:
        np.testing.assert_array_equal(got, want, err_msg=t)
    elif est:
        np.testing.assert_allclose(got, want, rtol=1e-11, atol=1e-13, err_msg=t)
    elif name == "gmapping":
        np.testing.assert_array_equal(got[..., 0], want[..., 0], err_msg=t)
        np.testing.assert_allclose(got[..., 1:], want[..., 1:], rtol=1e-13, atol=1e-15, err_msg=t)
    else:
        np.testing.assert_array_equal(got, want, err_msg=t)
    if rule in pc.AUX_STRIDE:
        np.testing.assert_array_equal(ctx.map_download_aux(map_id, 0, 0, w, h, pc.AUX_STRIDE[rule]), g[t + "aux"], err_msg=t)
    return 1


def debug_check(ctx, fn_name, map_id):
    valid, bad = C.c_int(-1), C.c_longlong(-1)
    assert getattr(ctx.L, fn_name)(ctx.h, map_id, C.byref(valid), C.byref(bad)) == 0
    return valid.value, bad.value


@pytest.mark.parametrize("name,est", pc.UPDATE_RUNS, ids=pc.UPDATE_IDS)
@pytest.mark.parametrize("station", ps.Q_STATIONS)
def test_map_updates_against_the_reference_golden(pkg, tctx, variant, g, station, name, est):
    """The golden's three appends into a fresh window bound at the station, under SLAMHIP_OPT_K6_PATH 0, 1 and 2, with the
    provider's arithmetic uploaded (cos a, sin a) and with the raw provider itself.  After the last append the stored TBM
    plane / GMapping masks equal the derived ones and the scores equal a fresh upload's."""
    ctx, st = tctx, station
    r, a, occ = g[st + "_raw_range"], g[st + "_raw_angle"], g[st + "_raw_occ"]
    c, s = pkg.beam_trig(a)
    kw = device_adder(g, name, est)
    try:
        for path in (0, 1, 2):
            ctx.set_option(pkg.OPT_K6_PATH, path)
            for raw in (False, True):
                cell_model, rule, w, h = bind_fresh(pkg, ctx, g, st, name, 2)
                checked = 0
                for k in range(3):
                    pose = g[st + "_append_poses"][k]
                    if raw:
                        nu = ctx.map_append_scan_raw(2, rule, pose, r, a, occ, **kw)
                    else:
                        nu = ctx.map_append_scan(2, rule, pose, r, c, s, occ, **kw)
                    assert nu > 1000
                    checked += check_snapshot(ctx, g, st, name, est, k, 2, raw, cell_model, rule, w, h)
                assert checked == (1 if (name, est) == ("tbm", 1) else 3)
        # the derived state behind the last history (raw provider, radix pipeline)
        if name != "mean" and est == 0:
            scan = pc.golden_scan(g, st, 0)
            cfg = pkg.spe_cfg(oope=pkg.OOPE_GMAPPING) if name == "gmapping" else pkg.spe_cfg()
            cc, ss = pkg.beam_trig(scan.angle)
            ctx.scan_upload(scan.range, cc, ss, scan.weight)
            poses = g[st + "_gm_poses" if name == "gmapping" else st + "_poses"]
            ctx.gm_cache_reset()
            got = ctx.score_poses(2, cfg, poses)
            fn = "slamhip_map_debug_nbr_masks" if name == "gmapping" else "slamhip_map_debug_prob_plane"
            assert debug_check(ctx, fn, 2) == (1, 0)
            cells = ctx.map_download_window(2, 0, 0, w, h, pc.STRIDE[cell_model])
            info = ctx.map_info(2)
            ctx.map_bind(3, cell_model, w, h, info["origin"], info["scale"], g["%s_%s_unknown" % (st, name)][:pc.STRIDE[cell_model]])
            ctx.map_upload_window(3, 0, 0, cells)
            ctx.gm_cache_reset()
            np.testing.assert_array_equal(got, ctx.score_poses(3, cfg, poses))
            ctx.map_release(3)
            assert len(np.unique(got)) > 40
    finally:
        ctx.set_option(pkg.OPT_K6_PATH, 0)
        ctx.map_release(2)


@pytest.mark.parametrize("name,est", pc.UPDATE_RUNS, ids=pc.UPDATE_IDS)
def test_map_update_batch_of_the_four_quadrants(pkg, ctx, variant, g, name, est):
    """map_append_scan_batch with the four Q maps in ONE call per append: every snapshot against the golden, raw provider
    (`angle` jobs) and uploaded arithmetic; the jobs listed backwards in the second append."""
    kw = device_adder(g, name, est)
    batch_kw = dict(estimator=1, shift_amount=kw.pop("shift_amount")) if est else {}
    kw.pop("estimator", None)
    for raw in (True, False):
        geo = {st: bind_fresh(pkg, ctx, g, st, name, 2 + i) for i, st in enumerate(ps.Q_STATIONS)}
        rule = pc.CLASSES[name][1]
        checked = 0
        for k in range(3):
            jobs = []
            for i, st in enumerate(ps.Q_STATIONS):
                j = dict(map_id=2 + i, pose=g[st + "_append_poses"][k], range=g[st + "_raw_range"], is_occ=g[st + "_raw_occ"], **kw)
                if raw:
                    j["angle"] = g[st + "_raw_angle"]
                else:
                    j["cos_a"], j["sin_a"] = pkg.beam_trig(g[st + "_raw_angle"])
                jobs.append(j)
            if k == 1:
                jobs = jobs[::-1]
            nu, status = ctx.map_append_scan_batch(rule, jobs, **batch_kw)
            assert not status.any() and (np.asarray(nu) > 1000).all()
            assert ctx.map_update_batch_stats()["jobs_shared"] == 4
            for i, st in enumerate(ps.Q_STATIONS):
                checked += check_snapshot(ctx, g, st, name, est, k, 2 + i, raw, *geo[st])
        assert checked == 4 * (1 if (name, est) == ("tbm", 1) else 3)
    for i in range(4):
        ctx.map_release(2 + i)


@pytest.mark.parametrize("name,est", pc.UPDATE_RUNS, ids=pc.UPDATE_IDS)
def test_map_updates_at_f1_against_the_oracle(pkg, ctx, oracle, variant, g, name, est):
    """1e5 ... 2e5 m out, where the reference's maps cannot follow: the golden scene's raster and adder at station F1, three
    appends with the raw provider under the three pipelines, against the map-update oracle -- bit for bit."""
    from pyoracle import GridMapData
    from pyoracle_mapupdate import append_scan_ex
    st = "F1"
    (kx, ky), _ = ps.STATIONS[st]
    sc = ps.place(st, size=int(g["raster"]), scale=float(g["scale"]), n_beams=int(g["n_beams"]), raw=True)
    r, a, occ = sc["raw"]
    rs = np.random.RandomState(ps.SEEDS[st])
    occ = occ.copy()
    occ[rs.rand(r.size) < 0.08] = 0
    poses = np.array([sc["local"] + rs.randn(3) * [0.01, 0.01, 0.002] for _ in range(3)]) + sc["shift"]
    cell_model, rule = pc.CLASSES[name]
    w, h = [int(v) for v in g["window"]]
    origin = (w // 2 - kx, h // 2 - ky)
    unk = g["Q1_%s_unknown" % name][:pc.STRIDE[cell_model]]
    okw, oex = pc.adder_args(g, name, est)
    om = GridMapData(cell_model, np.tile(unk, (h, w, 1)).astype(np.float64), origin, float(g["scale"]), unk)
    oaux = np.zeros((h, w, pc.AUX_STRIDE[rule])) if rule in pc.AUX_STRIDE else None
    want = []
    for k in range(3):
        n = append_scan_ex(oracle, om, oaux, rule, poses[k], r, a, occ, **okw, **oex)
        want.append((n, om.payload.copy(), None if oaux is None else oaux.copy()))
    assert (om.payload != unk).any(axis=2).sum() > 1000
    kw = device_adder(g, name, est)
    try:
        for path in (0, 1, 2):
            ctx.set_option(pkg.OPT_K6_PATH, path)
            ctx.map_bind(2, cell_model, w, h, origin, float(g["scale"]), unk)
            for k in range(3):
                assert ctx.map_append_scan_raw(2, rule, poses[k], r, a, occ, **kw) == want[k][0]
                np.testing.assert_array_equal(ctx.map_download_window(2, 0, 0, w, h, pc.STRIDE[cell_model]), want[k][1])
                if oaux is not None:
                    np.testing.assert_array_equal(ctx.map_download_aux(2, 0, 0, w, h, pc.AUX_STRIDE[rule]), want[k][2])
            ctx.map_release(2)
    finally:
        ctx.set_option(pkg.OPT_K6_PATH, 0)
