"""GPU suite (-m gpu): K INDEPENDENT multi-resolution matches in one call (slamhip_matcher_m3rsm_match_each: m3rsm::run_each
over the multi-request launches) against a lone matcher's process_scan per request -- delta, probability, the committed
calls and the counters, bit for bit in strict and in default mode -- on the resident golden scenes of
tests/golden/m3rsm_many.npz, set up as tests/test_gpu_m3rsm_many.py sets them up."""
import ctypes as C

import numpy as np
import pytest
from m3rsm_many_cases import SCENE_NAMES, golden_scene
from test_gpu_m3rsm_many import Scene, bits, kernel_scene

import __graft_entry__ as ge

pytestmark = pytest.mark.gpu

SHAPES = ((1, 1), (3, 2), (32, 3))  # speculation: parents per search and round, generations


@pytest.fixture(scope="module")
def pkg():
    return ge.load_package()


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


@pytest.fixture
def scene(pkg, ctx, request):
    sc = Scene(pkg, ctx, golden_scene(SCENE_NAMES.index(request.param)))
    yield sc
    sc.close()


def lone_match(sc, strict, shape, pyr_index, map_id, slot, pose):
    """what a lone matcher over the request's pyramid makes of it: result, committed calls, counters"""
    m = sc.matcher(strict=strict, pyr=pyr_index)
    m.set_m3rsm_speculation(*shape)
    sc.ctx.scan_select(slot)
    r = m.process_scan(map_id, pose)
    st = m.stats()
    out = dict(delta=r["delta"], prob=r["prob"], trace=m.m3rsm_trace(), scorer_calls=st["scorer_calls"],
               poses_evaluated=st["poses_evaluated"], super_steps=st["launches"] - 1)
    m.close()
    sc.matchers.remove(m)
    return out


def assert_request_is_lone(m, k, got, want):
    np.testing.assert_array_equal(bits(got["delta"]), bits(want["delta"]))
    np.testing.assert_array_equal(bits([got["prob"]]), bits([want["prob"]]))
    np.testing.assert_array_equal(bits(m.m3rsm_trace_each(k)), bits(want["trace"]))
    st = m.m3rsm_each_stats(k)
    assert {q: st[q] for q in ("scorer_calls", "poses_evaluated", "super_steps")} == \
        {q: want[q] for q in ("scorer_calls", "poses_evaluated", "super_steps")}
    assert st["branching_pops"] >= st["super_steps"] >= 1


def check_table(sc, strict, shape, table, lone):
    """match_each over `table` with 1 and 8 threads: every request the lone match, the call's own stats"""
    m = sc.matcher(strict=strict)
    m.set_m3rsm_speculation(*shape)
    seen = []
    for threads in (1, 8):
        m.set_m3rsm_threads(threads)
        got = m.m3rsm_match_each(table)
        assert len(got) == len(table)
        for k in range(len(table)):
            assert_request_is_lone(m, k, got[k], lone[k])
        st = m.stats()
        steps = [q["super_steps"] for q in lone]
        assert st["scorer_calls"] == sum(q["scorer_calls"] for q in lone)
        assert st["poses_evaluated"] == sum(q["poses_evaluated"] for q in lone)
        assert st["launches"] == 1 + max(steps) < sum(1 + v for v in steps)  # a round per super-step of the longest search
        seen.append((got, [m.m3rsm_trace_each(k) for k in range(len(table))], st["launches"]))
    for k in range(len(table)):
        np.testing.assert_array_equal(bits(seen[0][0][k]["delta"]), bits(seen[1][0][k]["delta"]))
        np.testing.assert_array_equal(bits([seen[0][0][k]["prob"]]), bits([seen[1][0][k]["prob"]]))
        np.testing.assert_array_equal(bits(seen[0][1][k]), bits(seen[1][1][k]))
    assert seen[0][2] == seen[1][2]
    with pytest.raises(sc.pkg.SlamHipError, match="error -1"):
        m.m3rsm_trace_each(len(table))
    with pytest.raises(sc.pkg.SlamHipError, match="error -1"):
        m.m3rsm_each_stats(-1)
    return m


# ---- 1. every request is its lone match -----------------------------------------------------------------
@pytest.mark.parametrize("strict", [True, False], ids=["strict", "default"])
@pytest.mark.parametrize("scene", SCENE_NAMES, indirect=True)
def test_each_request_gets_its_lone_match(scene, strict):
    s = scene.s
    for shape in SHAPES:
        lone = [lone_match(scene, strict, shape, rq.map, 10 * rq.map, k, rq.pose) for k, rq in enumerate(s.requests)]
        # request 0 listed a second time, at the end: the same answer twice
        table, want = scene.table + [scene.table[0]], lone + [lone[0]]
        check_table(scene, strict, shape, table, want)
        print("%s %s W %d D %d: super-steps per request %s" % (s.name, "strict" if strict else "default", *shape,
                                                                [q["super_steps"] for q in lone]))
        if strict:  # the lone matches are the reference's (tests/golden/m3rsm_many.npz keeps them per request)
            for k, q in enumerate(lone):
                np.testing.assert_array_equal(bits(q["delta"]), bits(s.lone[k, :3]))
                assert q["prob"] == s.lone[k, 3] and q["scorer_calls"] == s.lone[k, 4]


# ---- 2. pyramids of different depth, scans of 1, 65 and 257 beams -------------------------------------------
@pytest.mark.parametrize("strict", [True, False], ids=["strict", "default"])
def test_five_requests_over_two_pyramids_with_1_65_and_257_beams(pkg, ctx, strict):
    sc = kernel_scene(pkg, ctx, 65)
    try:
        (p0, s0, q0), (p1, s1, q1), (p2, s2, q2) = sc.table
        # (pyramid, slot, pose): the three of the scene, then two of its scans from other poses
        table = [(p0, s0, q0), (p1, s1, q1), (p2, s2, q2), (p1, s1, q1 + np.array([0.03, -0.02, 0.01])),
                 (p0, s2, q2 + np.array([-0.05, 0.04, -0.02]))]
        index = {id(p): j for j, p in enumerate(sc.pyr)}
        for shape in SHAPES:
            lone = [lone_match(sc, strict, shape, index[id(p)], 10 * index[id(p)], slot, pose) for p, slot, pose in table]
            check_table(sc, strict, shape, table, lone)
            steps = [q["super_steps"] for q in lone]
            print("W %d D %d: super-steps per request %s" % (*shape, steps))
            if shape == (1, 1):
                assert len(set(steps)) > 1  # searches end in different rounds: the drop-out path runs
    finally:
        sc.close()


# ---- 3. observer ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["occ_m2m"], indirect=True)
def test_observer_hears_every_request_in_order(scene):
    pkg, events = scene.pkg, []

    def on_other(_u, p, sc):
        events.append(("other",))

    def on_end(_u, d, sc):
        events.append(("end", (d[0], d[1], d[2]), sc))

    m = scene.matcher(strict=True)
    obs = pkg.Observer(None, pkg.OBS_FN(on_other), pkg.OBS_FN(on_other), pkg.OBS_FN(on_end))
    pkg._check(m.L.slamhip_matcher_set_observer(m.h, C.byref(obs)))
    m._obs_cleared = False
    got = m.m3rsm_match_each(scene.table)
    pkg._check(m.L.slamhip_matcher_set_observer(m.h, None))
    m._obs_cleared = True
    assert events == [("end", tuple(r["delta"]), r["prob"]) for r in got]
    assert len({r["prob"] for r in got}) == len(got)  # (so the order is told apart)
    assert [r["prob"] for r in got] == list(scene.s.lone[:, 3])


# ---- 4. refusals ------------------------------------------------------------------------------------------
def test_errors(pkg, ctx):
    sc = Scene(pkg, ctx, golden_scene(SCENE_NAMES.index("occ_m2m")))
    tbm = golden_scene(SCENE_NAMES.index("tbm_pair"))
    other = pkg.Context(0)
    try:
        s = sc.s
        m = sc.matcher(strict=True)
        good = sc.table
        p0, slot0, pose0 = good[0]

        def still_matches():
            got = m.m3rsm_match_each(good)
            assert [r["prob"] for r in got] == list(s.lone[:, 3])
            for k, r in enumerate(got):
                np.testing.assert_array_equal(bits(r["delta"]), bits(s.lone[k, :3]))

        def refused(table, code="error -1"):
            with pytest.raises(pkg.SlamHipError, match=code):
                m.m3rsm_match_each(table)
            assert m.stats()["launches"] == 0  # found before anything is launched

        still_matches()
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
        still_matches()
        hc = pkg.Matcher(ctx, "HC", pkg.spe_cfg(), [6, 0.1, 0.1])
        with pytest.raises(pkg.SlamHipError, match="error -1"):
            hc.m3rsm_match_each(good)                                 # not a multi-resolution matcher
        with pytest.raises(pkg.SlamHipError, match="error -1"):
            hc.set_m3rsm_threads(2)
        hc.close()
        m.set_m3rsm_speculation(0, 0)                                 # the per-pop route has no batched form
        refused(good)
        m.set_m3rsm_speculation(32, 3)
        for threads in (-1, 17):
            with pytest.raises(pkg.SlamHipError, match="error -1"):
                m.set_m3rsm_threads(threads)
        m.set_m3rsm_threads(0)
        still_matches()
        # map 1 re-bound behind its pyramid: a stale pyramid is a state error; rebuild, and the call works again
        ctx.map_release(10)
        mp = s.maps[1]
        ctx.map_bind(10, mp.cell_model, mp.width + 2, mp.height, (mp.origin[0] + 1, mp.origin[1]), mp.scale, mp.unknown)
        refused(good, "error -4")
        ctx.map_release(10)
        ctx.upload_map(10, mp)
        sc.pyr[1].rebuild()
        still_matches()
        # the two batch calls of the other matchers keep refusing this one
        with pytest.raises(pkg.SlamHipError, match="not batched"):
            m.process_scan_batch([dict(map_id=0, scan_slot=0, init_pose=good[0][2])] * 2)
    finally:
        other.close()
        sc.close()
