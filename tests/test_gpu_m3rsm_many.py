"""GPU suite (-m gpu): the multi-resolution matcher (BF_M3RSM) with several requests in one search -- the multi-request
launches (csrc/map_pyramid.hip k_pyr_score_many, csrc/m3rsm.hip k_m3rsm_expand_many) against the single-request entry
points on every request alone, and whole shared searches (m3rsm::run_many over those launches) against
tests/golden/m3rsm_many.npz: the compiled reference's M3RSMEngine given several scan matching requests, with the full
trace of its scorer calls.  Strict mode (beam-order sum, host pose trig) is compared bit for bit, trace included."""
import types

import numpy as np
import pytest
from m3rsm_many_cases import SCENE_NAMES, golden_scene
from test_gpu_m3rsm import PARENTS, STEP, synthetic_scan

import __graft_entry__ as ge

pytestmark = pytest.mark.gpu

DEFAULT_RTOL = 1e-12  # the pyramid tests' bar for the default mode (canonical tree sum, device sincos)
SLOTS = {1: 5, 2: 30, 3: 155}


@pytest.fixture(scope="module")
def pkg():
    return ge.load_package()


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def cfg_of(pkg, oie, strict):
    return pkg.spe_cfg(oope=pkg.OOPE_MAX, oie=oie, sum_order=pkg.SUM_SEQUENTIAL if strict else pkg.SUM_TREE256,
                       pose_trig=pkg.POSE_TRIG_HOST if strict else pkg.POSE_TRIG_DEVICE)


class Scene:
    """a golden scene resident on the device: map j is map id 10 j with its levels behind it, request k's scan in slot k"""

    def __init__(self, pkg, ctx, s):
        self.pkg, self.ctx, self.s = pkg, ctx, s
        self.maps = s.maps
        self.pyr, self.matchers = [], []
        for j, m in enumerate(self.maps):
            ctx.upload_map(10 * j, m)
            self.pyr.append(pkg.Pyramid(ctx, 10 * j, s.oie, 10 * j + 1))
        for k, r in enumerate(s.requests):
            ctx.scan_store(k, r.scan[:, 0], r.scan[:, 1], r.scan[:, 2], r.scan[:, 3], r.scan[:, 4])
        self.table = [(self.pyr[r.map], k, r.pose) for k, r in enumerate(s.requests)]

    def matcher(self, strict, pyr=0):
        m = self.pkg.Matcher(self.ctx, "BF_M3RSM", cfg_of(self.pkg, self.s.oie, strict), [self.pyr[pyr], *self.s.limits])
        self.matchers.append(m)
        return m

    def lone(self, m, k):
        """request k alone through process_scan of a matcher over its pyramid"""
        r = self.s.requests[k]
        self.ctx.scan_select(k)
        return m.process_scan(10 * r.map, r.pose)

    def close(self):
        for m in self.matchers:
            m.close()
        for p in self.pyr:
            p.close()
        for j in range(len(self.maps)):
            self.ctx.map_release(10 * j)


@pytest.fixture
def scene(pkg, ctx, request):
    sc = Scene(pkg, ctx, golden_scene(SCENE_NAMES.index(request.param)))
    yield sc
    sc.close()


# ---- 1. the kernels ---------------------------------------------------------------------------------------
def kernel_scene(pkg, ctx, n_mid):
    """three requests with 1, n_mid and 257 beams over two pyramids with a different number of levels: the 37 x 29 map of
    occ_m2m at 0.05 and a 9 x 9 window cut out of its 33 x 33 map at 0.1"""
    g = golden_scene(SCENE_NAMES.index("occ_m2m"))
    big, src = g.maps[1], g.maps[0]
    small = types.SimpleNamespace(cell_model=src.cell_model, scale=src.scale, origin=(4, 5), unknown=src.unknown,
                                  payload=np.ascontiguousarray(src.payload[1:10, 2:11]), width=9, height=9)
    s = types.SimpleNamespace(oie=g.oie, limits=g.limits, maps=[big, small], requests=[])
    for k, (mi, n, pose) in enumerate(((0, 1, (0.21, -0.33, 0.4)), (1, n_mid, (0.05, 0.02, -0.7)), (0, 257, (0.3, -0.2, 2.9)))):
        scan = np.column_stack(synthetic_scan(n, 11 + n))
        scan[:, 0] *= 0.35 if mi == 1 else 0.6  # (the ranges stay inside the maps)
        s.requests.append(types.SimpleNamespace(map=mi, pose=np.array(pose), scan=scan))
    sc = Scene(pkg, ctx, s)
    n_levels = [len(p.info()) for p in sc.pyr]
    assert n_levels[0] != n_levels[1], n_levels
    return sc


@pytest.mark.parametrize("n_mid", [63, 65])  # one wave less / more one beam; 1 and 257 beams (a second pass) ride along
def test_request_launches_equal_the_single_request_launches(pkg, ctx, n_mid):
    sc = kernel_scene(pkg, ctx, n_mid)
    try:
        s = sc.s
        rs = np.random.RandomState(5)
        for n in (1, 130):  # 130 x 155 slots: more workgroups than the device holds at once
            rect = PARENTS[[0]] if n == 1 else PARENTS[np.arange(n) % len(PARENTS)]
            rot = rs.uniform(-0.1, 0.1, n)
            req = np.array([2]) if n == 1 else (np.arange(n) * 7 + np.arange(n) // 9) % 3  # parents interleaved across requests
            if n == 130:  # every request meets every kind of parent
                assert {(int(a), int(b)) for a, b in zip(req, np.arange(n) % len(PARENTS))} == {(a, b) for a in range(3) for b in range(len(PARENTS))}
            for sum_order in (pkg.SUM_TREE256, pkg.SUM_SEQUENTIAL):
                for trig in (pkg.POSE_TRIG_DEVICE, pkg.POSE_TRIG_HOST):
                    cfg = pkg.spe_cfg(oope=pkg.OOPE_MAX, oie=s.oie, sum_order=sum_order, pose_trig=trig)
                    for depth in (1, 2, 3):
                        got_rect, got_score, got_level = pkg.Pyramid.expand_requests(ctx, cfg, sc.table, req, rot, rect, STEP, depth)
                        assert got_rect.shape == (n, SLOTS[depth], 4)
                        scored = 0
                        for k, (pyr, slot, pose) in enumerate(sc.table):
                            mine = req == k
                            if not mine.any():
                                continue
                            ctx.scan_select(slot)
                            want_rect, want_score, want_level = pyr.expand_matches(cfg, pose, rot[mine], rect[mine], STEP, depth)
                            np.testing.assert_array_equal(bits(got_rect[mine]), bits(want_rect))
                            np.testing.assert_array_equal(bits(got_score[mine]), bits(want_score))
                            np.testing.assert_array_equal(got_level[mine], want_level)
                            scored += int(np.isfinite(want_score).sum())
                        assert scored > 0
                    # the bounds launch: the proper rectangles of the batch as candidates
                    ok = (rect[:, 0] <= rect[:, 1]) & (rect[:, 2] <= rect[:, 3])
                    got_score, got_level = pkg.Pyramid.score_requests(ctx, cfg, sc.table, req[ok], rot[ok], rect[ok])
                    for k, (pyr, slot, pose) in enumerate(sc.table):
                        mine = req[ok] == k
                        if not mine.any():
                            continue
                        ctx.scan_select(slot)
                        want_score, want_level = pyr.score_matches(cfg, pose, rot[ok][mine], rect[ok][mine])
                        np.testing.assert_array_equal(bits(got_score[mine]), bits(want_score))
                        np.testing.assert_array_equal(got_level[mine], want_level)
                        assert np.all(np.isfinite(want_score)) and np.all(want_level >= 0)
        # the two pyramids do answer on levels the other does not have
        _, lv = pkg.Pyramid.score_requests(ctx, cfg, sc.table, [0, 1], [0.0, 0.0], [(-3, 3, -3, 3)] * 2)
        assert lv[0] != lv[1]
    finally:
        sc.close()


# ---- 2, 3. whole shared searches against the compiled reference -------------------------------------------
def match_with_end_observer(pkg, m, table, events):
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
    r = m.m3rsm_match_many(table)
    pkg._check(m.L.slamhip_matcher_set_observer(m.h, None))
    m._obs_cleared = True
    return r


@pytest.mark.parametrize("scene", SCENE_NAMES, indirect=True)
def test_strict_mode_is_the_references_shared_search_call_for_call(scene):
    s = scene.s
    for width, depth in ((1, 1), (32, 3), (0, 0)):
        m = scene.matcher(strict=True)
        m.set_m3rsm_speculation(width, depth)
        ended = []
        r = match_with_end_observer(scene.pkg, m, scene.table, ended)
        trace = m.m3rsm_trace_many()
        st = m.stats()
        print("%s W %d D %d: %d calls in %d launches, %d candidates scored, winner %d, prob %.17g (reference %.17g)"
              % (s.name, width, depth, len(trace), st["launches"], st["poses_evaluated"], r["request"], r["prob"], s.prob))
        np.testing.assert_array_equal(bits(trace), bits(s.trace))
        assert r["request"] == s.winner
        np.testing.assert_array_equal(bits(r["delta"]), bits(s.delta))
        assert r["prob"] == s.prob
        assert st["scorer_calls"] == len(s.trace) and st["launches"] >= 2 and st["poses_evaluated"] > 0
        assert len(ended) == 1 and ended[0][0] == "end" and ended[0][1] == tuple(s.delta) and ended[0][2] == s.prob


@pytest.mark.parametrize("scene", SCENE_NAMES, indirect=True)
def test_default_mode_finds_the_references_winner(scene):
    s = scene.s
    m = scene.matcher(strict=False)
    r = m.m3rsm_match_many(scene.table)
    print("%s: winner %d, prob %.17g (reference %.17g, rel %.3g), %d calls (reference %d)"
          % (s.name, r["request"], r["prob"], s.prob, abs(r["prob"] / s.prob - 1), m.stats()["scorer_calls"], len(s.trace)))
    assert r["request"] == s.winner
    np.testing.assert_array_equal(r["delta"], s.delta)
    assert abs(r["prob"] - s.prob) <= DEFAULT_RTOL * abs(s.prob)


# ---- 4. one request; the lone matches; process_scan afterwards ------------------------------------------------
@pytest.mark.parametrize("scene", ["occ_m2m"], indirect=True)
def test_one_request_is_process_scan_and_the_winner_is_the_best_lone_match(scene):
    s = scene.s
    lone = []
    for k, rq in enumerate(s.requests):
        m = scene.matcher(strict=True, pyr=rq.map)
        before = scene.lone(m, k)
        trace = m.m3rsm_trace()
        st = m.stats()
        # the reference's lone match of this request
        np.testing.assert_array_equal(bits(before["delta"]), bits(s.lone[k, :3]))
        assert before["prob"] == s.lone[k, 3] and st["scorer_calls"] == s.lone[k, 4]
        one = m.m3rsm_match_many([scene.table[k]])
        t8 = m.m3rsm_trace_many()
        assert one["request"] == 0 and one["prob"] == before["prob"] and np.all(t8[:, 0] == 0)
        np.testing.assert_array_equal(bits(one["delta"]), bits(before["delta"]))
        np.testing.assert_array_equal(bits(t8[:, 1:]), bits(trace))
        st1 = m.stats()
        assert {q: st1[q] for q in ("scorer_calls", "poses_evaluated", "launches")} == {q: st[q] for q in ("scorer_calls", "poses_evaluated", "launches")}
        # process_scan on the same matcher is unchanged afterwards
        after = scene.lone(m, k)
        np.testing.assert_array_equal(bits(m.m3rsm_trace()), bits(trace))
        assert after["prob"] == before["prob"] and np.array_equal(after["delta"], before["delta"])
        lone.append(before)
    m = scene.matcher(strict=True)
    r = m.m3rsm_match_many(scene.table)
    best = int(np.argmax([q["prob"] for q in lone]))
    assert r["request"] == best and r["prob"] == lone[best]["prob"] and np.array_equal(r["delta"], lone[best]["delta"])
    assert m.stats()["scorer_calls"] < sum(s.lone[:, 4])  # the shared cut bites


# ---- 5. refresh ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["occ_m2m"], indirect=True)
def test_match_after_refresh_of_one_pyramid_equals_match_over_fresh_pyramids(scene):
    s, ctx, pkg = scene.s, scene.ctx, scene.pkg
    m = scene.matcher(strict=True)
    before = m.m3rsm_match_many(scene.table)
    assert before["request"] == s.winner
    # request 2's scan, shortened so that no beam leaves the window, written into map 1 from a pose beside its own: walls
    # appear inside the room, impacts change on every level of ONE pyramid
    rq = s.requests[2]
    pose = rq.pose + np.array([0.04, -0.03, 0.02])
    assert ctx.map_append_scan(10, pkg.RULE_LAST, pose, 0.8 * rq.scan[:, 0], rq.scan[:, 1], rq.scan[:, 2]) > 0
    mp = s.maps[1]
    scene.pyr[1].refresh(0, 0, mp.width, mp.height)
    after = m.m3rsm_match_many(scene.table)
    trace_after = m.m3rsm_trace_many()
    assert len(trace_after) != len(s.trace) or not np.array_equal(bits(trace_after), bits(s.trace))  # the map did change
    m.close()
    scene.matchers.remove(m)
    for j in (0, 1):
        scene.pyr[j].close()
        scene.pyr[j] = pkg.Pyramid(ctx, 10 * j, s.oie, 10 * j + 1)
    scene.table = [(scene.pyr[r.map], k, r.pose) for k, r in enumerate(s.requests)]
    fresh = scene.matcher(strict=True)
    want = fresh.m3rsm_match_many(scene.table)
    np.testing.assert_array_equal(bits(trace_after), bits(fresh.m3rsm_trace_many()))
    assert after["request"] == want["request"] and after["prob"] == want["prob"]
    np.testing.assert_array_equal(bits(after["delta"]), bits(want["delta"]))


# ---- 6. errors ------------------------------------------------------------------------------------------
def test_errors(pkg, ctx):
    sc = Scene(pkg, ctx, golden_scene(SCENE_NAMES.index("occ_m2m")))
    tbm = golden_scene(SCENE_NAMES.index("tbm_pair"))
    other = pkg.Context(0)
    try:
        s = sc.s
        m = sc.matcher(strict=True)
        cfg = cfg_of(pkg, s.oie, True)
        good = sc.table
        p0, slot0, pose0 = good[0]

        def refused(table, code="error -1"):
            with pytest.raises(pkg.SlamHipError, match=code):
                m.m3rsm_match_many(table)
            with pytest.raises(pkg.SlamHipError, match=code):
                pkg.Pyramid.score_requests(ctx, cfg, table, [0], [0.0], [(0, 0, 0, 0)])
            with pytest.raises(pkg.SlamHipError, match=code):
                pkg.Pyramid.expand_requests(ctx, cfg, table, [0], [0.0], [(0, 0.2, 0, 0.2)], 0.05, 1)

        refused([])                                                   # n_requests < 1
        refused([good[0], (None, 1, pose0)])                          # a null pyramid
        other.upload_map(0, s.maps[0])
        foreign = pkg.Pyramid(other, 0, s.oie, 1)
        refused([good[0], (foreign, 1, pose0)])                       # a pyramid of another context
        foreign.close()
        ctx.upload_map(40, tbm.maps[0])
        mixed = pkg.Pyramid(ctx, 40, tbm.oie, 41)
        refused([good[0], (mixed, 1, pose0)])                         # mixed cell models
        mixed.close()
        ctx.map_release(40)
        other_oie = pkg.Pyramid(ctx, 0, pkg.OIE_OCCUPANCY, 41)
        refused([good[0], (other_oie, 1, pose0)])                     # mixed OIEs
        refused([(other_oie, 1, pose0), good[0]])                     # ... and not the cfg's
        other_oie.close()
        refused([good[0], (p0, 77, pose0)])                           # a scan slot nobody stored
        refused([good[0], (p0, -1, pose0)])
        for bad in (np.nan, np.inf):
            refused([good[0], (p0, slot0, (pose0[0], bad, pose0[2]))])  # a pose that is not finite
        for request, rect in (([4], [(0, 0, 0, 0)]), ([-1], [(0, 0, 0, 0)]), ([0], [(0, np.inf, 0, 1)])):
            with pytest.raises(pkg.SlamHipError, match="error -1"):
                pkg.Pyramid.score_requests(ctx, cfg, good, request, [0.0], rect)
            with pytest.raises(pkg.SlamHipError, match="error -1"):
                pkg.Pyramid.expand_requests(ctx, cfg, good, request, [0.0], rect, 0.05, 1)
        for step, depth in ((0.0, 1), (np.nan, 1), (0.05, 0), (0.05, 4)):
            with pytest.raises(pkg.SlamHipError, match="error -1"):
                pkg.Pyramid.expand_requests(ctx, cfg, good, [0], [0.0], [(0, 0.2, 0, 0.2)], step, depth)
        r, sc_, lv = pkg.Pyramid.expand_requests(ctx, cfg, good, [], [], np.zeros((0, 4)), 0.05, 2)
        assert r.shape == (0, 30, 4)
        hc = pkg.Matcher(ctx, "HC", pkg.spe_cfg(), [6, 0.1, 0.1])
        with pytest.raises(pkg.SlamHipError, match="error -1"):
            hc.m3rsm_match_many(good)                                 # not a multi-resolution matcher
        hc.close()
        ok = m.m3rsm_match_many(good)
        assert ok["request"] == s.winner and ok["prob"] == s.prob
        # map 1 re-bound behind its pyramid: a stale pyramid is a state error; rebuild, and the search works again
        ctx.map_release(10)
        mp = s.maps[1]
        ctx.map_bind(10, mp.cell_model, mp.width + 2, mp.height, (mp.origin[0] + 1, mp.origin[1]), mp.scale, mp.unknown)
        refused(good, "error -4")
        ctx.map_release(10)
        ctx.upload_map(10, mp)
        sc.pyr[1].rebuild()
        again = m.m3rsm_match_many(good)
        np.testing.assert_array_equal(bits(m.m3rsm_trace_many()), bits(s.trace))
        assert again["request"] == s.winner and again["prob"] == s.prob and np.array_equal(again["delta"], s.delta)
    finally:
        other.close()
        sc.close()
