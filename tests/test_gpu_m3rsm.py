"""GPU suite (-m gpu): the multi-resolution matcher (BF_M3RSM) on the device -- the expand kernel (csrc/m3rsm.hip) against
slamhip_pyramid_score_matches on the rectangles a host split makes, and whole matches (csrc/m3rsm_engine.cpp over expand
launches) against tests/golden/m3rsm.npz: the compiled reference's BruteForceMultiResolutionScanMatcher with the full
trace of its scorer calls.  Strict mode (beam-order sum, host pose trig) is compared bit for bit, trace included."""
import numpy as np
import pytest
from m3rsm_cases import N_SCENES, SCENE_NAMES, SLOTS, golden_scene, host_slots

import __graft_entry__ as ge

pytestmark = pytest.mark.gpu

DEFAULT_RTOL = 1e-12  # the pyramid tests' bar for the default mode (canonical tree sum, device sincos)
FINE, FIRST = 0, 1
OOPE_MAX = 1


@pytest.fixture(scope="module")
def pkg():
    p = ge.load_package()
    assert p.OOPE_MAX == OOPE_MAX
    return p


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def cfg_of(pkg, s, strict):
    return pkg.spe_cfg(oope=pkg.OOPE_MAX, oie=s.oie, sum_order=pkg.SUM_SEQUENTIAL if strict else pkg.SUM_TREE256,
                       pose_trig=pkg.POSE_TRIG_HOST if strict else pkg.POSE_TRIG_DEVICE)


class Scene:
    """a golden scene resident on the device: map, scan, pyramid, and matchers over them"""

    def __init__(self, pkg, ctx, i):
        self.pkg, self.ctx, self.s = pkg, ctx, golden_scene(i)
        s = self.s
        ctx.upload_map(FINE, s)
        ctx.scan_upload(s.scan[:, 0], s.scan[:, 1], s.scan[:, 2], s.scan[:, 3], s.scan[:, 4])
        self.pyr = pkg.Pyramid(ctx, FINE, s.oie, FIRST)
        self.matchers = []

    def matcher(self, strict, limits=None):
        lim = self.s.limits if limits is None else limits
        m = self.pkg.Matcher(self.ctx, "BF_M3RSM", cfg_of(self.pkg, self.s, strict), [self.pyr, *lim])
        self.matchers.append(m)
        return m

    def close(self):
        for m in self.matchers:
            m.close()
        self.pyr.close()
        self.ctx.map_release(FINE)


@pytest.fixture
def scene(pkg, ctx, request):
    sc = Scene(pkg, ctx, SCENE_NAMES.index(request.param) if isinstance(request.param, str) else request.param)
    yield sc
    sc.close()


# ---- 1. the expand kernel ----------------------------------------------------------------------------
STEP = 0.05
PARENTS = np.array([
    (-0.4, 0.4, -0.4, 0.4),     # a square box: four quarters, all the way down
    (0.0, 0.04, -0.1, 0.1),     # oblong: only the horizontal side branches (split_horz)
    (-0.3, 0.1, 0.2, 0.23),     # oblong the other way (split_vert)
    (0.0, 0.04, 0.0, 0.03),     # no side branches: the five crucial points
    (0.1, 0.1, -0.2, -0.2),     # a point: no children
    (0.3, 0.1, 0.0, 1.0),       # reversed: no children
    (0.0, 0.05, 0.0, 0.05),     # both sides exactly the step: still four quarters
    (0.0, 0.05, 0.0, 0.04),     # one side exactly the step: it alone branches
    (-0.07, 0.07, -0.21, 0.21),  # a step that does not divide the range
])


def synthetic_scan(n, seed):
    rs = np.random.RandomState(seed)
    ang = rs.uniform(-np.pi, np.pi, n)
    return rs.uniform(0.3, 1.3, n), np.cos(ang), np.sin(ang), np.full(n, 1.0 / n), np.ones(n)


@pytest.mark.parametrize("n_beams", [1, 63, 65, 257])  # a lone beam, one wave less / more one beam, a second pass of the workgroup
@pytest.mark.parametrize("scene", ["occ_square", "tbm_square"], indirect=True)
def test_expand_matches_equals_score_matches_on_host_splits(pkg, ctx, scene, n_beams):
    s = scene.s
    ctx.scan_upload(*synthetic_scan(n_beams, 7 + n_beams))
    rs = np.random.RandomState(3)
    for n in (1, 130):  # 130 x 155 slots: more workgroups than the device holds at once
        rect = PARENTS[[0]] if n == 1 else PARENTS[np.arange(n) % len(PARENTS)]
        rot = rs.uniform(-0.1, 0.1, n)
        for depth in (1, 2, 3):
            want_rect = np.stack([host_slots(r, STEP, depth) for r in rect])
            there = ~np.isnan(want_rect[..., 0])
            if n == 130:  # every kind of node occurs, and empty slots next to full ones
                per = there[:len(PARENTS)].sum(axis=1)
                assert per[0] == {1: 4, 2: 20, 3: 84}[depth] and per[4] == 0 and per[5] == 0 and per[3] == 5 and per[1] >= 2
            for sum_order in (pkg.SUM_TREE256, pkg.SUM_SEQUENTIAL):
                for trig in (pkg.POSE_TRIG_DEVICE, pkg.POSE_TRIG_HOST):
                    cfg = pkg.spe_cfg(oope=pkg.OOPE_MAX, oie=s.oie, sum_order=sum_order, pose_trig=trig)
                    got_rect, got_score, got_level = scene.pyr.expand_matches(cfg, s.pose, rot, rect, STEP, depth)
                    assert got_rect.shape == (n, SLOTS[depth], 4)
                    np.testing.assert_array_equal(bits(got_rect[there]), bits(want_rect[there]))
                    assert np.all(np.isnan(got_rect[~there])) and np.all(np.isnan(got_score[~there])) and np.all(got_level[~there] == -1)
                    slot_rot = np.broadcast_to(rot[:, None], there.shape)[there]
                    want_score, want_level = scene.pyr.score_matches(cfg, s.pose, slot_rot, want_rect[there])
                    np.testing.assert_array_equal(bits(got_score[there]), bits(want_score))
                    np.testing.assert_array_equal(got_level[there], want_level)
                    assert np.all(np.isfinite(want_score)) and np.all(want_level >= 0)


def test_expand_matches_refuses_bad_arguments(pkg, ctx):
    sc = Scene(pkg, ctx, 0)
    try:
        cfg = cfg_of(pkg, sc.s, False)
        for step, depth in ((0.0, 1), (-0.05, 1), (np.nan, 1), (0.05, 0), (0.05, 4)):
            with pytest.raises(pkg.SlamHipError):
                sc.pyr.expand_matches(cfg, sc.s.pose, [0.0], PARENTS[:1], step, depth)
        with pytest.raises(pkg.SlamHipError):
            sc.pyr.expand_matches(cfg, sc.s.pose, [0.0], [(0, np.inf, 0, 1)], 0.05, 1)
        with pytest.raises(pkg.SlamHipError):
            sc.pyr.expand_matches(pkg.spe_cfg(oope=pkg.OOPE_OBSTACLE, oie=sc.s.oie), sc.s.pose, [0.0], PARENTS[:1], 0.05, 1)
        r, sc_, lv = sc.pyr.expand_matches(cfg, sc.s.pose, [], np.zeros((0, 4)), 0.05, 2)
        assert r.shape == (0, 30, 4)
    finally:
        sc.close()


# ---- 2, 3. whole matches against the compiled reference ------------------------------------------------
@pytest.mark.parametrize("scene", SCENE_NAMES, indirect=True)
def test_strict_mode_is_the_references_match_call_for_call(scene):
    s = scene.s
    m = scene.matcher(strict=True)
    ended = []
    r = process_with_end_observer(scene.pkg, m, s.pose, ended)
    trace = m.m3rsm_trace()
    print("%s: %d calls, prob %.17g (reference %.17g)" % (s.name, len(trace), r["prob"], s.prob))
    np.testing.assert_array_equal(bits(trace), bits(s.trace))
    np.testing.assert_array_equal(bits(r["delta"]), bits(s.delta))
    assert r["prob"] == s.prob
    st = m.stats()
    assert st["scorer_calls"] == len(s.trace) and st["launches"] >= 2 and st["poses_evaluated"] > 0
    # on_matching_end once, with the result; nothing else (the reference's matcher emits no on_scan_test)
    assert len(ended) == 1 and ended[0][0] == "end" and ended[0][1] == tuple(s.delta) and ended[0][2] == s.prob


def process_with_end_observer(pkg, m, pose, events):
    import ctypes as C

    def on_test(_u, p, sc):
        events.append(("test",))

    def on_update(_u, p, sc):
        events.append(("update",))

    def on_end(_u, d, sc):
        events.append(("end", (d[0], d[1], d[2]), sc))

    obs = pkg.Observer(None, pkg.OBS_FN(on_test), pkg.OBS_FN(on_update), pkg.OBS_FN(on_end))
    pkg._check(m.L.slamhip_matcher_set_observer(m.h, C.byref(obs)))
    m._obs_cleared = False
    ip, d3, prob = (C.c_double * 3)(*[float(v) for v in pose]), (C.c_double * 3)(), C.c_double()
    pkg._check(m.L.slamhip_matcher_process_scan(m.h, FINE, ip, d3, C.byref(prob)))
    pkg._check(m.L.slamhip_matcher_set_observer(m.h, None))
    m._obs_cleared = True
    return dict(prob=prob.value, delta=np.array(list(d3)))


@pytest.mark.parametrize("scene", SCENE_NAMES, indirect=True)
def test_default_mode_finds_the_references_match(scene):
    s = scene.s
    m = scene.matcher(strict=False)
    r = m.process_scan(FINE, s.pose)
    print("%s: prob %.17g (reference %.17g, rel %.3g), %d calls (reference %d)"
          % (s.name, r["prob"], s.prob, abs(r["prob"] / s.prob - 1), m.stats()["scorer_calls"], len(s.trace)))
    np.testing.assert_array_equal(r["delta"], s.delta)
    assert abs(r["prob"] - s.prob) <= DEFAULT_RTOL * abs(s.prob)


# ---- 4. the result does not depend on the speculation's shape ---------------------------------------------
@pytest.mark.parametrize("scene", ["occ_step07", "cred_square"], indirect=True)
def test_traces_do_not_depend_on_width_and_depth(scene):
    s = scene.s
    seen = {}
    for width, depth in ((1, 1), (8, 2), (128, 1), (128, 3)):
        m = scene.matcher(strict=True)
        m.set_m3rsm_speculation(width, depth)
        r = m.process_scan(FINE, s.pose)
        st = m.stats()
        trace = m.m3rsm_trace()
        duplicates = len(trace) - len({row[:5].tobytes() for row in trace})
        print("%s W %3d D %d: %5d launches, %6d candidates scored for %5d calls (%d of them repeats)"
              % (s.name, width, depth, st["launches"], st["poses_evaluated"], st["scorer_calls"], duplicates))
        assert st["poses_evaluated"] >= st["scorer_calls"] - duplicates
        seen[width, depth] = (trace, r, st)
        np.testing.assert_array_equal(bits(trace), bits(s.trace))
        np.testing.assert_array_equal(bits(r["delta"]), bits(s.delta))
        assert r["prob"] == s.prob
    assert seen[1, 1][2]["launches"] > seen[8, 2][2]["launches"] > seen[128, 1][2]["launches"] >= seen[128, 3][2]["launches"]
    # without the expand kernel (0, 0): a score_matches launch per popped match, the same trace
    m.set_m3rsm_speculation(0, 0)
    r = m.process_scan(FINE, s.pose)
    np.testing.assert_array_equal(bits(m.m3rsm_trace()), bits(s.trace))
    assert r["prob"] == s.prob and m.stats()["launches"] == seen[1, 1][2]["launches"]
    assert m.stats()["poses_evaluated"] == seen[1, 1][2]["poses_evaluated"]
    with pytest.raises(scene.pkg.SlamHipError):
        m.set_m3rsm_speculation(0, 1)
    with pytest.raises(scene.pkg.SlamHipError):
        m.set_m3rsm_speculation(8, 4)


# ---- 5. raw scans -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["occ_square"], indirect=True)
def test_process_raw_scan_is_filter_upload_plus_process_scan(scene):
    s, ctx = scene.s, scene.ctx
    rng, ang = s.scan[:, 0].copy(), np.arctan2(s.scan[:, 2], s.scan[:, 1])
    occ = np.ones(rng.size, np.int32)
    occ[::7] = 0
    one, two = scene.matcher(strict=False), scene.matcher(strict=False)
    match = one.make_raw_process_scan(FINE, rng, ang, is_occ=occ)
    up = ctx.make_raw_scan(FINE, rng, ang, is_occ=occ)
    for k in range(2):
        pose = s.pose + k * np.array([0.01, -0.02, 0.005])
        kept1, prob1 = match(pose)
        trace1 = one.m3rsm_trace()
        kept2 = up(pose)
        r2 = two.process_scan(FINE, pose)
        assert kept1 == kept2 and 0 < kept1 < rng.size
        assert prob1 == r2["prob"] and np.array_equal(np.array(list(match.delta)), r2["delta"]) and np.isfinite(prob1)
        np.testing.assert_array_equal(bits(trace1), bits(two.m3rsm_trace()))
        assert one.stats()["scorer_calls"] == two.stats()["scorer_calls"] > 0 and one.stats()["launches"] >= 2
    empty = one.make_raw_process_scan(FINE, rng, ang, is_occ=np.zeros_like(occ))
    kept, prob = empty(s.pose)
    assert kept == 0 and np.isnan(prob) and list(empty.delta) == [0.0, 0.0, 0.0]
    assert one.stats()["launches"] == 0 and one.stats()["scorer_calls"] == 0


# ---- 6. refresh ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["tbm_square"], indirect=True)
def test_match_after_refresh_equals_match_over_a_fresh_pyramid(scene):
    s, ctx, pkg = scene.s, scene.ctx, scene.pkg
    m = scene.matcher(strict=True)
    before = m.process_scan(FINE, s.pose)
    # the scan written into the map from a pose next to the walls' true place: walls move, impacts change on every level
    pose = s.pose + np.array([0.25, -0.15, 0.06])
    assert ctx.map_append_scan(FINE, pkg.RULE_TBM, pose, s.scan[:, 0], s.scan[:, 1], s.scan[:, 2]) > 0
    scene.pyr.refresh(0, 0, s.width, s.height)
    after = m.process_scan(FINE, s.pose)
    trace_after = m.m3rsm_trace()
    assert len(trace_after) != len(s.trace) or not np.array_equal(bits(trace_after), bits(s.trace))  # the map did change
    m.close()
    scene.matchers.remove(m)
    scene.pyr.close()
    scene.pyr = pkg.Pyramid(ctx, FINE, s.oie, FIRST)
    fresh = scene.matcher(strict=True)
    want = fresh.process_scan(FINE, s.pose)
    np.testing.assert_array_equal(bits(trace_after), bits(fresh.m3rsm_trace()))
    np.testing.assert_array_equal(bits(after["delta"]), bits(want["delta"]))
    assert after["prob"] == want["prob"] and np.isfinite(before["prob"])


# ---- 7. errors ----------------------------------------------------------------------------------------------
def test_errors(pkg, ctx):
    sc = Scene(pkg, ctx, 0)
    s = sc.s
    other = pkg.Context(0)
    try:
        lim = list(s.limits)
        good = pkg.spe_cfg(oope=pkg.OOPE_MAX, oie=s.oie)
        for bad_cfg in (pkg.spe_cfg(oope=pkg.OOPE_OBSTACLE, oie=s.oie),              # the 1-cell OOPE
                        pkg.spe_cfg(oope=pkg.OOPE_GMAPPING, oie=s.oie),              # the GMapping OOPE
                        pkg.spe_cfg(oope=pkg.OOPE_MAX, oie=pkg.OIE_OCCUPANCY)):      # not the pyramid's OIE
            with pytest.raises(pkg.SlamHipError, match="error -1"):
                pkg.Matcher(ctx, "BF_M3RSM", bad_cfg, [sc.pyr, *lim])
        with pytest.raises(pkg.SlamHipError, match="another context"):
            pkg.Matcher(other, "BF_M3RSM", good, [sc.pyr, *lim])
        for k in (3, 4):  # steps that are not positive
            for v in (0.0, -0.01):
                with pytest.raises(pkg.SlamHipError, match="error -1"):
                    pkg.Matcher(ctx, "BF_M3RSM", good, [sc.pyr, *lim[:k], v, *lim[k + 1:]])
        m = sc.matcher(strict=True)
        with pytest.raises(pkg.SlamHipError, match="error -1"):
            m.process_scan(FIRST, s.pose)  # a level's id is not the fine map's
        ok = m.process_scan(FINE, s.pose)
        assert ok["prob"] == s.prob
        m.reset_state()
        # the fine map re-bound behind the pyramid: a stale pyramid is a state error; rebuild, and the matcher works again
        ctx.map_release(FINE)
        ctx.upload_map(FINE, s)
        stale = False
        try:
            m.process_scan(FINE, s.pose)
        except pkg.SlamHipError as e:
            stale = "error -4" in str(e)
        if not stale:  # (the allocator handed the same block back: same payload pointer, same geometry -- grow the map)
            ctx.map_release(FINE)
            ctx.map_bind(FINE, s.cell_model, s.width + 2, s.height, (s.origin[0] + 1, s.origin[1]), s.scale, s.unknown)
            with pytest.raises(pkg.SlamHipError, match="error -4"):
                m.process_scan(FINE, s.pose)
            ctx.map_release(FINE)
            ctx.upload_map(FINE, s)
        sc.pyr.rebuild()
        again = m.process_scan(FINE, s.pose)
        np.testing.assert_array_equal(bits(m.m3rsm_trace()), bits(s.trace))
        assert again["prob"] == s.prob and np.array_equal(again["delta"], s.delta)
    finally:
        other.close()
        sc.close()
