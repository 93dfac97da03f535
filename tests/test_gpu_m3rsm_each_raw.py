"""GPU suite (-m gpu): K RAW scans in, K multi-resolution matches (slamhip_matcher_m3rsm_match_each_raw: the host filter per
request through RawBatchStage, ONE k_scan_assemble_table launch for all six-row blocks, the lock-step searches of
m3rsm_match_each over those blocks) against a lone slamhip_matcher_process_raw_scan per request on a matcher over the
request's pyramid -- delta, probability, kept count, committed calls and counters, bit for bit -- and against the stored
route (host filter + scan_store (+ angles) + m3rsm_match_each).  Scenes as tests/test_gpu_m3rsm_many.py::kernel_scene sets
them up: two pyramids of different depth."""
import ctypes as C

import numpy as np
import pytest
from pyramid_cases import placed_lone_scene
from test_gpu_m3rsm_each import SHAPES, assert_request_is_lone
from test_gpu_m3rsm_many import bits, kernel_scene
from test_gpu_raw_batch import download, filtered, lone_raw, scanner, table_uploads

import __graft_entry__ as ge

pytestmark = pytest.mark.gpu

WEIGHTINGS = ("even", "viny", "ahr")
CFGS = ("strict", "default", "raw_exact")


@pytest.fixture(scope="module")
def pkg():
    return ge.load_package()


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


@pytest.fixture
def sc(pkg, ctx):
    s = kernel_scene(pkg, ctx, 65)
    yield s
    s.close()


def cfg_of(pkg, oie, form):
    if form == "raw_exact" and pkg.libm_variant() < 0:
        pytest.skip("this host's libm is neither build restated in csrc/libm_exact.h")
    kw = dict(strict=dict(sum_order=pkg.SUM_SEQUENTIAL, pose_trig=pkg.POSE_TRIG_HOST), default=dict(),
              raw_exact=dict(sum_order=pkg.SUM_SEQUENTIAL, pose_trig=pkg.POSE_TRIG_RAW_EXACT))[form]
    return pkg.spe_cfg(oope=pkg.OOPE_MAX, oie=oie, **kw)


def request(pkg, sc, pyr, n_raw, k, pose, trig, weighting, seed, skip_rate=0, max_range=-1.0, bounded=False, factor=False,
            reach=None):
    """a raw request over pyramid `pyr` of the scene whose filter keeps exactly k points: ranges up to `reach`, the
    filter's other rules as given, then is_occ = 0 on every point behind the k-th the other rules keep"""
    m = sc.s.maps[pyr]
    rs = np.random.RandomState(seed)
    s = scanner(n_raw)
    reach = reach if reach is not None else (0.3 if pyr == 1 else 0.55)
    rng = 0.05 + reach * rs.rand(n_raw)
    job = dict(pyramid=sc.pyr[pyr], map_id=10 * pyr, range=rng, angle=s["angle"], is_occ=None,
               factor=0.5 + rs.rand(n_raw) if factor else None, trig_mode=pkg.TRIG_CACHED if trig == "cached" else pkg.TRIG_RAW,
               a_min=s["a_min"], a_max=s["a_max"], a_inc=s["a_inc"], skip_rate=skip_rate, max_range=max_range, bounded=bounded,
               weighting=weighting, init_pose=np.asarray(pose, dtype=np.float64), world=dict(map=m), pyr_index=pyr)
    _, kept = filtered(pkg, job)
    assert kept.size >= k, (kept.size, k)
    occ = np.zeros(n_raw, np.int32)
    occ[kept[:k]] = 1
    job["is_occ"] = occ
    job["others_drop"] = n_raw - kept.size  # what skip_rate / max_range / the rim dropped before is_occ
    return job


def four_requests(pkg, sc, trig, weighting, n_mid=65):
    """1, n_mid and 257 kept points (a beam below / above a wave, a second pass), each filter rule at work: is_occ alone;
    skip_rate 3 and max_range on the small pyramid; the rim of the bounded big map, with factors; and the big pyramid
    listed a second time"""
    rq = [request(pkg, sc, 0, 300, 1, (0.21, -0.33, 0.4), trig, weighting, 1),
          request(pkg, sc, 1, 600, n_mid, (0.05, 0.02, -0.7), trig, weighting, 2, skip_rate=3, max_range=0.3),
          request(pkg, sc, 0, 900, 257, (0.3, -0.2, 2.9), trig, weighting, 3, bounded=True, factor=True, reach=1.2),
          request(pkg, sc, 0, 300, 40, (0.1, -0.1, 1.0), trig, weighting, 4, factor=True)]
    assert rq[0]["others_drop"] == 0 and rq[1]["others_drop"] > 400 and rq[2]["others_drop"] > 50
    return rq


def matcher(pkg, ctx, sc, cfg, pyr, shape):
    m = pkg.Matcher(ctx, "BF_M3RSM", cfg, [sc.pyr[pyr], *sc.s.limits])
    m.set_m3rsm_speculation(*shape)
    return m


def lone(pkg, ctx, sc, cfg, shape, job, scan=False):
    """the lone raw match of the request: result, committed calls, counters (and the context's scan block after it)"""
    m = matcher(pkg, ctx, sc, cfg, job["pyr_index"], shape)
    r = lone_raw(pkg, m, job, trace=False)
    st = m.stats()
    out = dict(delta=r["delta"], prob=r["prob"], kept=r["kept"], trace=m.m3rsm_trace() if r["kept"] else np.zeros((0, 7)),
               scorer_calls=st["scorer_calls"], poses_evaluated=st["poses_evaluated"], super_steps=max(st["launches"] - 1, 0))
    if scan and r["kept"]:
        out["block"] = download(ctx)
    m.close()
    return out


def assert_is_lone(m, k, got, want):
    assert got["kept"] == want["kept"]
    if want["kept"] == 0:
        assert np.isnan(got["prob"]) and np.isnan(want["prob"]) and not got["delta"].any() and not want["delta"].any()
        assert m.m3rsm_trace_each(k).shape == (0, 7)
        assert m.m3rsm_each_stats(k) == dict(scorer_calls=0, poses_evaluated=0, super_steps=0, branching_pops=0)
        return
    assert_request_is_lone(m, k, got, want)


# ---- 1. every request is its lone raw match ------------------------------------------------------------------------
@pytest.mark.parametrize("trig", ["raw", "cached"])
@pytest.mark.parametrize("weighting", WEIGHTINGS)
@pytest.mark.parametrize("form", CFGS)
def test_every_request_is_its_lone_raw_match(pkg, ctx, sc, form, weighting, trig):
    cfg = cfg_of(pkg, sc.s.oie, form)
    for shape, n_mid in zip(SHAPES, (63, 65, 65)):
        rq = four_requests(pkg, sc, trig, weighting, n_mid)
        want = [lone(pkg, ctx, sc, cfg, shape, j, scan=True) for j in rq]
        assert [w["kept"] for w in want] == [1, n_mid, 257, 40]
        m = matcher(pkg, ctx, sc, cfg, 0, shape)
        seen = []
        for threads in (1, 8):
            m.set_m3rsm_threads(threads)
            got = m.m3rsm_match_each_raw(rq)
            for k in range(len(rq)):
                assert_is_lone(m, k, got[k], want[k])
            # 6. one assembly launch, the root layers' launch, a round per super-step of the longest search
            steps = [w["super_steps"] for w in want]
            st = m.stats()
            assert st["launches"] == 1 + 1 + max(steps) < sum(1 + v for v in steps)
            assert st["scorer_calls"] == sum(w["scorer_calls"] for w in want)
            seen.append([(bits(g["delta"]).tolist(), bits([g["prob"]]).tolist(), bits(m.m3rsm_trace_each(k)).tolist())
                         for k, g in enumerate(got)])
        assert seen[0] == seen[1]
        # the blocks in HBM are the lone call's scan blocks, the sixth row the kept points' angles
        for k, j in enumerate(rq):
            rows, ang = m.m3rsm_each_scan_download(k)
            np.testing.assert_array_equal(rows.view(np.uint64), want[k]["block"], err_msg="request %d" % k)
            np.testing.assert_array_equal(bits(ang), bits(j["angle"][j["is_occ"] == 1]))
        # the stored route: the public host filter, weights and beam trig, scan_store (+ angles), match_each
        table = []
        for k, j in enumerate(rq):
            f, kept = filtered(pkg, j)
            ctx.scan_store(10 + k, f["range"], f["cos_a"], f["sin_a"], f["weight"],
                           f["factor"] if f["factor"] is not None else np.ones(kept.size))
            if form == "raw_exact":
                ctx.scan_store_angles(10 + k, j["angle"][kept])
            table.append((j["pyramid"], 10 + k, j["init_pose"]))
        stored = m.m3rsm_match_each(table)
        for k in range(len(rq)):
            assert_request_is_lone(m, k, stored[k], want[k])
        assert m.stats()["launches"] == st["launches"] - 1
        m.close()


# ---- 2. empty requests -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["strict", "default"])
def test_empty_requests(pkg, ctx, sc, form):
    cfg, shape = cfg_of(pkg, sc.s.oie, form), SHAPES[1]
    rq = four_requests(pkg, sc, "raw", "viny")
    empty = dict(rq[1], is_occ=np.zeros(600, np.int32))
    want = [lone(pkg, ctx, sc, cfg, shape, j) for j in rq]
    assert lone(pkg, ctx, sc, cfg, shape, empty)["kept"] == 0
    events = []

    def on_other(_u, p, s):
        events.append(("other",))

    def on_end(_u, d, s):
        events.append((d[0], d[1], d[2], s))

    m = matcher(pkg, ctx, sc, cfg, 0, shape)
    obs = pkg.Observer(None, pkg.OBS_FN(on_other), pkg.OBS_FN(on_other), pkg.OBS_FN(on_end))
    pkg._check(m.L.slamhip_matcher_set_observer(m.h, C.byref(obs)))
    m._obs_cleared = False
    got = m.m3rsm_match_each_raw([rq[0], empty, rq[1], rq[2], empty])
    gone = dict(kept=0, prob=np.nan, delta=np.zeros(3))
    for k, w in enumerate([want[0], gone, want[1], want[2], gone]):
        assert_is_lone(m, k, got[k], w)
    # the observer: on_matching_end once per request that has a match, in request order
    assert events == [(*g["delta"], g["prob"]) for g in got if g["kept"]]
    assert m.m3rsm_each_scan_download(1)[0].shape == (5, 0)
    launches = m.stats()["launches"]
    assert launches == 2 + max(w["super_steps"] for w in want[:3])
    # every request empty: nothing is launched, nobody is called
    del events[:]
    got = m.m3rsm_match_each_raw([empty, empty])
    for k in (0, 1):
        assert_is_lone(m, k, got[k], gone)
    st = m.stats()
    assert (st["scorer_calls"], st["poses_evaluated"], st["launches"]) == (0, 0, 0) and events == []
    with pytest.raises(pkg.SlamHipError, match="error -1"):
        m.m3rsm_trace_each(2)
    # one request alone takes the same path
    got = m.m3rsm_match_each_raw([rq[2]])
    assert_is_lone(m, 0, got[0], want[2])
    assert m.stats()["launches"] == 2 + want[2]["super_steps"]
    pkg._check(m.L.slamhip_matcher_set_observer(m.h, None))
    m._obs_cleared = True
    m.close()


# ---- 3. the caller's scans are left alone ----------------------------------------------------------------------------
def test_the_callers_scans_are_left_alone(pkg, ctx, sc):
    cfg, shape = cfg_of(pkg, sc.s.oie, "strict"), SHAPES[2]
    rq = four_requests(pkg, sc, "cached", "ahr")
    r2 = sc.s.requests[2]  # the scene's stored scans: slot k holds request k's
    ctx.scan_select(2)
    before_block = download(ctx)
    ml = matcher(pkg, ctx, sc, cfg, 0, shape)
    before = ml.process_scan(0, r2.pose)
    before_trace = ml.m3rsm_trace()
    m = matcher(pkg, ctx, sc, cfg, 0, shape)
    m.m3rsm_match_each_raw(rq)
    np.testing.assert_array_equal(download(ctx), before_block)  # the selected slot is still selected and holds its scan
    after = ml.process_scan(0, r2.pose)
    np.testing.assert_array_equal(bits(after["delta"]), bits(before["delta"]))
    assert after["prob"] == before["prob"]
    np.testing.assert_array_equal(bits(ml.m3rsm_trace()), bits(before_trace))
    for k, r in enumerate(sc.s.requests):  # every stored slot
        ctx.scan_select(k)
        np.testing.assert_array_equal(download(ctx), bits(r.scan.T).view(np.uint64))
    # an uploaded scan stays the current one
    ctx.scan_upload(r2.scan[:, 0], r2.scan[:, 1], r2.scan[:, 2], r2.scan[:, 3], r2.scan[:, 4])
    m.m3rsm_match_each_raw(rq[:2])
    np.testing.assert_array_equal(download(ctx), before_block)
    up = ml.process_scan(0, r2.pose)
    assert up["prob"] == before["prob"]
    m.close()
    ml.close()


# ---- 4. tables go up once per scanner ---------------------------------------------------------------------------------
def test_tables_go_up_once_per_scanner(pkg):
    own = pkg.Context(0)
    s = kernel_scene(pkg, own, 65)
    try:
        cfg = cfg_of(pkg, s.s.oie, "default")
        rq = four_requests(pkg, s, "cached", "viny")  # scanners of 300, 600 and 900 beams: three tables
        m = matcher(pkg, own, s, cfg, 0, SHAPES[2])
        t0 = table_uploads(own)
        first = m.m3rsm_match_each_raw(rq)
        assert table_uploads(own) == t0 + 3
        again = m.m3rsm_match_each_raw([rq[3], rq[1], rq[0]])  # the same scanners, other requests: nothing goes up
        assert table_uploads(own) == t0 + 3
        assert [g["prob"] for g in again] == [first[3]["prob"], first[1]["prob"], first[0]["prob"]]
        other = dict(rq[0], trig_mode=pkg.TRIG_RAW)  # the same angles under the other provider: another scanner
        m.m3rsm_match_each_raw([other, rq[1]])
        assert table_uploads(own) == t0 + 4
        m.close()
    finally:
        s.close()
        own.close()


# ---- 5. errors launch nothing -----------------------------------------------------------------------------------------
def test_errors_launch_nothing(pkg, ctx, sc):
    from m3rsm_many_cases import SCENE_NAMES, golden_scene
    cfg = cfg_of(pkg, sc.s.oie, "strict")
    rq = four_requests(pkg, sc, "cached", "even")
    good = rq[:3]
    m = matcher(pkg, ctx, sc, cfg, 0, SHAPES[2])
    m.m3rsm_match_each_raw(good)
    state = [(bits(m.m3rsm_trace_each(k)).tolist(), m.m3rsm_each_stats(k)) for k in range(3)]
    blocks = [m.m3rsm_each_scan_download(k)[0].view(np.uint64).tolist() for k in range(3)]
    uploads = table_uploads(ctx)

    def refused(requests, code="error -1", by=m):
        with pytest.raises(pkg.SlamHipError, match=code):
            by.m3rsm_match_each_raw(requests)
        # the call before still answers: its traces, its counters, its blocks
        assert [(bits(m.m3rsm_trace_each(k)).tolist(), m.m3rsm_each_stats(k)) for k in range(3)] == state
        assert [m.m3rsm_each_scan_download(k)[0].view(np.uint64).tolist() for k in range(3)] == blocks
        with pytest.raises(pkg.SlamHipError, match="error -1"):
            m.m3rsm_trace_each(3)

    other = pkg.Context(0)
    try:
        refused([])                                                               # n_requests < 1
        refused([good[0], dict(good[1], pyramid=None)])                           # a null pyramid
        other.upload_map(0, sc.s.maps[0])
        foreign = pkg.Pyramid(other, 0, sc.s.oie, 1)
        refused([good[0], dict(good[1], pyramid=foreign)])                        # a pyramid of another context
        foreign.close()
        tbm = golden_scene(SCENE_NAMES.index("tbm_pair"))
        ctx.upload_map(40, tbm.maps[0])
        mixed = pkg.Pyramid(ctx, 40, tbm.oie, 41)
        refused([good[0], dict(good[1], pyramid=mixed)])                          # mixed cell models
        mixed.close()
        ctx.map_release(40)
        other_oie = pkg.Pyramid(ctx, 0, pkg.OIE_OCCUPANCY, 41)
        refused([good[0], dict(good[1], pyramid=other_oie)])                      # mixed OIEs
        refused([dict(good[1], pyramid=other_oie), good[0]])                      # ... and not the cfg's
        other_oie.close()
        for bad in (np.nan, np.inf):
            refused([good[0], dict(good[1], init_pose=np.array([0.0, bad, 0.0]))])  # a pose that is not finite
        # what the lone raw call and RawBatchStage::prepare refuse of a scan
        refused([good[0], dict(good[1], range=np.zeros(0), angle=np.zeros(0), is_occ=None)])  # n <= 0
        refused([good[0], dict(good[1], trig_mode=7)])                            # neither provider
        refused([good[0], dict(good[1], a_min=good[1]["a_min"] + 1.0)])           # an angle outside the cached provider's table
        assert table_uploads(ctx) == uploads
        m.set_m3rsm_speculation(0, 0)                                             # the per-pop route has no batched form
        refused(good)
        m.set_m3rsm_speculation(*SHAPES[2])
        m.set_m3rsm_rotation_slots(True)                                          # the lone raw call refuses these too
        refused(good)
        m.set_m3rsm_rotation_slots(False)
        hc = pkg.Matcher(ctx, "HC", pkg.spe_cfg(), [6, 0.1, 0.1])
        refused(good, by=hc)                                                      # not a multi-resolution matcher
        hc.close()
        # map 10 re-bound behind its pyramid: a stale pyramid is a state error; rebuild, and the call works again
        mp = sc.s.maps[1]
        ctx.map_release(10)
        ctx.map_bind(10, mp.cell_model, mp.width + 2, mp.height, (mp.origin[0] + 1, mp.origin[1]), mp.scale, mp.unknown)
        refused(good, "error -4")
        ctx.map_release(10)
        ctx.upload_map(10, mp)
        sc.pyr[1].rebuild()
        got = m.m3rsm_match_each_raw(good)
        assert [(bits(m.m3rsm_trace_each(k)).tolist(), m.m3rsm_each_stats(k)) for k in range(3)] == state
        assert [g["kept"] for g in got] == [1, 65, 257]
        # the two batch calls of the other matchers keep refusing this one
        with pytest.raises(pkg.SlamHipError, match="not batched"):
            m.process_raw_scan_batch([dict(j, map_id=10 * j["pyr_index"]) for j in good])
        with pytest.raises(pkg.SlamHipError, match="not batched"):
            m.process_scan_batch([dict(map_id=0, scan_slot=0, init_pose=good[0]["init_pose"])] * 2)
    finally:
        other.close()
        m.close()


# ---- 7. far from the origin -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", CFGS)
def test_a_request_far_from_the_world_origin(pkg, ctx, form):
    s = placed_lone_scene("N1")  # tests/placed_scenes.py station N1, as tests/golden/placed_pyramid.npz keeps it
    # the window's cell nearest to the world origin, in cells (external x in [-origin_x, width - origin_x), y alike)
    near = [0 if -o <= 0 < n - o else min(abs(-o), abs(n - 1 - o)) for o, n in zip(s.origin, (s.width, s.height))]
    assert np.hypot(*near) >= 1000, (s.origin, s.width, s.height)
    cfg, shape = cfg_of(pkg, s.oie, form), SHAPES[2]
    ctx.upload_map(60, s)
    far = pkg.Pyramid(ctx, 60, s.oie, 61)
    try:
        angle = np.arctan2(s.scan[:, 2], s.scan[:, 1])
        order = np.argsort(angle, kind="stable")
        occ = np.ones(angle.size, np.int32)
        occ[::7] = 0
        job = dict(pyramid=far, map_id=60, range=s.scan[order, 0], angle=angle[order], is_occ=occ, factor=None, trig_mode=pkg.TRIG_RAW,
                   a_min=0.0, a_max=0.0, a_inc=1.0, skip_rate=0, max_range=-1.0, bounded=True, weighting="viny",
                   init_pose=s.pose, world=dict(map=s))
        beside = dict(job, init_pose=s.pose + np.array([0.03, -0.02, 0.01]), is_occ=None, weighting="even")
        m = pkg.Matcher(ctx, "BF_M3RSM", cfg, [far, *s.limits])
        m.set_m3rsm_speculation(*shape)
        want = []
        for j in (beside, job):
            ml = pkg.Matcher(ctx, "BF_M3RSM", cfg, [far, *s.limits])
            ml.set_m3rsm_speculation(*shape)
            r = lone_raw(pkg, ml, j, trace=False)
            st = ml.stats()
            want.append(dict(delta=r["delta"], prob=r["prob"], kept=r["kept"], trace=ml.m3rsm_trace(), scorer_calls=st["scorer_calls"],
                             poses_evaluated=st["poses_evaluated"], super_steps=st["launches"] - 1))
            ml.close()
            assert r["kept"] > 10 and np.isfinite(r["prob"]) and len(want[-1]["trace"]) > 20
        got = m.m3rsm_match_each_raw([beside, job])
        for k in (0, 1):
            assert_is_lone(m, k, got[k], want[k])
        m.close()
    finally:
        far.close()
        ctx.map_release(60)


# ---- 8. the one device stage under both of its users ------------------------------------------------------------------
HC_PRM = [24, 0.1, 0.1]


def route_matcher(pkg, ctx, sc, route):
    """the chains' batch (an HC matcher over map 0) or the fleet call (a BF_M3RSM matcher over pyramid 0, built on map 0)"""
    if route == "chain":
        return pkg.Matcher(ctx, "HC", pkg.spe_cfg(), HC_PRM)
    return matcher(pkg, ctx, sc, cfg_of(pkg, sc.s.oie, "default"), 0, SHAPES[2])


def route_lone(pkg, ctx, sc, route, job):
    """the job's lone raw call on a fresh matcher of the route's kind, and the context's scan block after it"""
    m = route_matcher(pkg, ctx, sc, route)
    r = lone_raw(pkg, m, job, trace=False)
    out = dict(delta=r["delta"], prob=r["prob"], kept=r["kept"], block=download(ctx) if r["kept"] else None)
    m.close()
    return out


def route_call(route, m, jobs):
    got = m.process_raw_scan_batch(jobs) if route == "chain" else m.m3rsm_match_each_raw(jobs)
    if route == "chain":
        assert all(m.batch_stats(c)["on_device_chain"] for c in range(len(jobs)))  # (nobody went through the lone call)
    return got


def route_block(route, m, k):
    """job k's block of the last call: (five rows, the sixth row or None)"""
    return (m.batch_scan_download(k), None) if route == "chain" else m.m3rsm_each_scan_download(k)


def same_result(got, want):
    return (got["kept"] == want["kept"] and np.array_equal(bits(got["delta"]), bits(want["delta"]))
            and np.array_equal(bits([got["prob"]]), bits([want["prob"]])))


@pytest.mark.parametrize("weighting", WEIGHTINGS)
def test_both_routes_write_the_same_block(pkg, ctx, sc, weighting):
    """three raw scans on map 0 whose kept counts lie around a 256-thread workgroup (and the stride's rounding to 8
    doubles: 256, 256, 264): one with a kept list from skip_rate 2, one of the raw provider, one with factors"""
    rq = [request(pkg, sc, 0, 600, 255, (0.21, -0.33, 0.4), "cached", weighting, 21, skip_rate=2),
          request(pkg, sc, 0, 300, 256, (0.1, -0.1, 1.0), "raw", weighting, 22),
          request(pkg, sc, 0, 300, 257, (0.3, -0.2, 2.9), "cached", weighting, 23, factor=True)]
    assert rq[0]["others_drop"] == 300 and rq[1]["others_drop"] == rq[2]["others_drop"] == 0
    hc, m = route_matcher(pkg, ctx, sc, "chain"), route_matcher(pkg, ctx, sc, "fleet")
    try:
        chain, fleet = route_call("chain", hc, rq), route_call("fleet", m, rq)
        assert [g["kept"] for g in chain] == [g["kept"] for g in fleet] == [255, 256, 257]
        for k, j in enumerate(rq):
            five, _ = route_block("chain", hc, k)
            rows, angle = route_block("fleet", m, k)
            assert five.shape == rows.shape == (5, 255 + k)
            np.testing.assert_array_equal(bits(rows), bits(five), err_msg="rows 0-4 of job %d" % k)
            np.testing.assert_array_equal(bits(angle), bits(j["angle"][j["is_occ"] == 1]), err_msg="sixth row of job %d" % k)
            np.testing.assert_array_equal(bits(rows[0]), bits(j["range"][j["is_occ"] == 1]))
    finally:
        hc.close()
        m.close()


@pytest.mark.parametrize("route", ["chain", "fleet"])
def test_arenas_that_regrow_between_calls(pkg, ctx, sc, route):
    """a small call, one that outgrows both arenas' floors (65536 bytes pinned, 16384 doubles in HBM), the small one again"""
    rows = 5 if route == "chain" else 6
    rs = np.random.RandomState(31)
    pose = lambda: np.array([*rs.uniform(-0.3, 0.3, 2), rs.uniform(-3.0, 3.0)])  # noqa: E731
    small = [request(pkg, sc, 0, 300, 40, pose(), "cached", "viny", 41, factor=True),
             request(pkg, sc, 0, 300, 65, pose(), "cached", "ahr", 42)]
    large = [request(pkg, sc, 0, 900, 891 + i, pose(), "cached", WEIGHTINGS[i % 3], 50 + i, factor=True) for i in range(10)]
    want_small = [route_lone(pkg, ctx, sc, route, j) for j in small]
    want_large = [route_lone(pkg, ctx, sc, route, j) for j in large]
    m = route_matcher(pkg, ctx, sc, route)
    try:
        first = route_call(route, m, small)
        second = route_call(route, m, large)
        block0 = route_block(route, m, 0)
        third = route_call(route, m, small)
        # the second call did outgrow what the first one had allocated, the first one did not
        for got, grows in ((first, False), (second, True)):
            kept = np.array([g["kept"] for g in got])
            assert (8 * kept.sum() > 65536) == grows, kept
            assert (rows * ((kept + 7) & ~7).sum() > 16384) == grows, kept
        for got, want in ((first, want_small), (second, want_large), (third, want_small)):
            assert [g["kept"] for g in got] == [w["kept"] for w in want] and all(w["kept"] > 0 for w in want)
            for k, (g, w) in enumerate(zip(got, want)):
                assert same_result(g, w), (k, g, w)
        for g, f in zip(third, first):
            assert same_result(g, f)
        # after the second call job 0's block is that call's: the lone call's scan block, and the kept angles behind it
        np.testing.assert_array_equal(block0[0].view(np.uint64), want_large[0]["block"])
        if route == "fleet":
            np.testing.assert_array_equal(bits(block0[1]), bits(large[0]["angle"][large[0]["is_occ"] == 1]))
        # ... and after the third, that one's (the arenas stay as large as they have grown)
        for k, w in enumerate(want_small):
            np.testing.assert_array_equal(route_block(route, m, k)[0].view(np.uint64), w["block"])
    finally:
        m.close()
