"""GPU suite (-m gpu): the multi-resolution matcher (BF_M3RSM) under the reference's DEFAULT trig provider --
SLAMHIP_POSE_TRIG_RAW_EXACT through the pyramid's bound and expand launches (csrc/map_pyramid.hip, csrc/m3rsm.hip: a table
of glibc's cos / sin((rotation + heading) + angle) per distinct rotation, filled by one launch in front of the scoring
one) -- against tests/golden/m3rsm_rawtrig.npz: the compiled reference's BruteForceMultiResolutionScanMatcher with the
scan under RawTrigonometryProvider, every scorer call.  Strict mode (beam-order sum) is compared bit for bit."""
import numpy as np
import pytest
from m3rsm_cases import SLOTS, host_slots
from m3rsm_rawtrig_cases import EDGE_NAMES, LIBM_VARIANT, SCENE_NAMES, bits, golden_scene
from test_gpu_m3rsm import PARENTS, STEP
from test_gpu_pyramid import golden_set, poses_of, upload_set

import __graft_entry__ as ge

pytestmark = pytest.mark.gpu

DEFAULT_RTOL = 1e-12  # tests/test_gpu_libm_exact.py's bar for the canonical sum over the raw provider's end points
FINE, FIRST = 0, 1
ERR_INVALID, ERR_STATE = "error -1", "error -4"


@pytest.fixture(scope="module")
def pkg():
    return ge.load_package()


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def variant(pkg):
    v = pkg.libm_variant()
    if v < 0:
        pytest.skip("this host's libm is neither build of glibc's sin / cos / exp: no exact modes here")
    print("libm variant %d (the golden was made under %d)" % (v, LIBM_VARIANT))
    return v


def raw_cfg(pkg, s, strict=True, oope=None):
    return pkg.spe_cfg(oope=pkg.OOPE_MAX if oope is None else oope, oie=s.oie,
                       sum_order=pkg.SUM_SEQUENTIAL if strict else pkg.SUM_TREE256, pose_trig=pkg.POSE_TRIG_RAW_EXACT)


def upload_scan(ctx, s, angles=True):
    ctx.scan_upload(s.scan[:, 0], s.scan[:, 1], s.scan[:, 2], s.scan[:, 3], s.scan[:, 4])
    if angles:
        ctx.scan_set_angles(s.angle)


class Scene:
    """a golden scene resident on the device: map, scan with its angles, pyramid, and matchers over them"""

    def __init__(self, pkg, ctx, name, fine=FINE):
        self.pkg, self.ctx, self.s, self.fine = pkg, ctx, golden_scene(name), fine
        ctx.upload_map(fine, self.s)
        upload_scan(ctx, self.s)
        self.pyr = pkg.Pyramid(ctx, fine, self.s.oie, fine + 1)
        self.matchers = []

    def matcher(self, strict=True, shape=None, pyr=None):
        m = self.pkg.Matcher(self.ctx, "BF_M3RSM", raw_cfg(self.pkg, self.s, strict), [pyr or self.pyr, *self.s.limits])
        if shape is not None:
            m.set_m3rsm_speculation(*shape)
        self.matchers.append(m)
        return m

    def close(self):
        for m in self.matchers:
            m.close()
        self.pyr.close()
        self.ctx.map_release(self.fine)


@pytest.fixture
def scene(pkg, ctx, variant, request):
    sc = Scene(pkg, ctx, request.param)
    yield sc
    sc.close()


# ---- 1. bounds against the golden ------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", SCENE_NAMES, indirect=True)
def test_bounds_are_the_raw_providers_call_for_call(scene):
    s, pkg = scene.s, scene.pkg
    rot, rect, want, want_level = s.trace[:, 0], s.trace[:, 1:5], s.trace[:, 5], s.trace[:, 6]
    got, level = scene.pyr.score_matches(raw_cfg(pkg, s), s.pose, rot, rect)
    bad = np.nonzero(bits(got) != bits(want))[0]
    print("%s: %d calls, %d distinct rotations, %d scores differ" % (s.name, len(rot), len(np.unique(rot)), len(bad)))
    np.testing.assert_array_equal(level, want_level)
    np.testing.assert_array_equal(got, want)
    dflt, level = scene.pyr.score_matches(raw_cfg(pkg, s, strict=False), s.pose, rot, rect)
    np.testing.assert_array_equal(level, want_level)
    np.testing.assert_allclose(dflt, want, rtol=DEFAULT_RTOL, atol=0)
    if s.edge:  # ... and not the cached provider's: HOST trig gives other bits on the calls the fixture was made for
        n = min(len(s.trace), len(s.trace_cached))
        host = pkg.spe_cfg(oope=pkg.OOPE_MAX, oie=s.oie, sum_order=pkg.SUM_SEQUENTIAL, pose_trig=pkg.POSE_TRIG_HOST)
        other, _ = scene.pyr.score_matches(host, s.pose, rot[:n], rect[:n])
        assert np.any(bits(other) != bits(want[:n]))


# ---- 2. bounds against slamhip_score_poses on the level: no golden, no libm variant in it -----------------------------
@pytest.mark.parametrize("j,n", [(12, 1), (13, 63), (16, 65), (34, 206), (46, 206)])
def test_score_matches_equals_score_poses_on_the_level(pkg, ctx, variant, j, n):
    s = golden_set(j)
    m, pyr = upload_set(pkg, ctx, s)
    ctx.scan_set_angles(np.arctan2(s.scan[:, 2], s.scan[:, 1]))
    rot206, rect206 = pkg.m3rsm_root_candidates((1.0, 1.0, 2 * 0.087), 0.0017)
    rot = np.concatenate([s.cand[s.n_roots - 2:, 0], rot206])[:n]
    rect = np.concatenate([s.cand[s.n_roots - 2:, 1:5], rect206])[:n]
    ids = pyr.level_map_ids()
    poses = poses_of(s.pose, rot, rect)
    seen_levels = set()
    for oope in (pkg.OOPE_MAX, pkg.OOPE_MEAN, pkg.OOPE_OVERLAP):
        for sum_order in (pkg.SUM_TREE256, pkg.SUM_SEQUENTIAL):
            mode = dict(oope=oope, oie=m.oie, sum_order=sum_order, pose_trig=pkg.POSE_TRIG_RAW_EXACT)
            got, level = pyr.score_matches(pkg.spe_cfg(area=(9, 9, 9, 9), **mode), s.pose, rot, rect)
            assert got.shape == (n,) and np.all((level >= 0) & (level < len(ids)))
            want = np.array([ctx.score_poses(ids[level[i]], pkg.spe_cfg(area=rect[i], **mode), poses[i:i + 1])[0] for i in range(n)])
            np.testing.assert_array_equal(bits(got), bits(want), err_msg=str((oope, sum_order)))
            seen_levels |= set(level.tolist())
    if n > 1:
        assert len(seen_levels) >= 3  # mixed levels in one launch
    pyr.close()
    ctx.map_release(FINE)


# ---- 3. whole matches against the compiled reference --------------------------------------------------------------
def assert_is_golden(s, r, trace):
    np.testing.assert_array_equal(bits(trace), bits(s.trace))
    np.testing.assert_array_equal(bits(r["delta"]), bits(s.delta))
    assert r["prob"] == s.prob
    if s.edge:
        assert len(trace) != len(s.trace_cached) or np.any(bits(trace) != bits(s.trace_cached))


@pytest.mark.parametrize("scene", SCENE_NAMES, indirect=True)
def test_strict_mode_is_the_references_match_under_its_default_provider(scene):
    s = scene.s
    launches = {}
    for shape in ((1, 1), (32, 3), (0, 0)):
        m = scene.matcher(shape=shape)
        r = m.process_scan(FINE, s.pose)
        st = m.stats()
        print("%s W %d D %d: %d calls, %d launches, prob %.17g (reference %.17g)"
              % (s.name, *shape, st["scorer_calls"], st["launches"], r["prob"], s.prob))
        assert_is_golden(s, r, m.m3rsm_trace())
        assert st["scorer_calls"] == len(s.trace) and st["launches"] >= 2
        launches[shape] = st["launches"]
    # the raw provider adds no super-step: the launch counts are the HOST-trig matcher's on the same trace shape
    assert launches[0, 0] == launches[1, 1] > launches[32, 3]
    # the same through process_raw_scan: the kept points' angles reach the bounds by themselves
    m = scene.matcher(shape=(32, 3))
    match = m.make_raw_process_scan(FINE, s.scan[:, 0], s.angle, trig_mode=scene.pkg.TRIG_RAW)
    kept, prob = match(s.pose)
    assert kept == len(s.angle)
    assert_is_golden(s, dict(delta=np.array(list(match.delta)), prob=prob), m.m3rsm_trace())


@pytest.mark.parametrize("scene", EDGE_NAMES, indirect=True)
def test_default_sum_finds_the_raw_providers_match(scene):
    s = scene.s
    r = scene.matcher(strict=False).process_scan(FINE, s.pose)
    np.testing.assert_array_equal(r["delta"], s.delta)
    assert abs(r["prob"] - s.prob) <= DEFAULT_RTOL * abs(s.prob)


# ---- 4. the expand kernels ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["edge_occ", "tbm_square"], indirect=True)
def test_expand_matches_equals_score_matches_on_host_splits(scene):
    s, pkg = scene.s, scene.pkg
    rots = np.array([0.0, -1 / 64, 1 / 64, 0.03125, -0.0])  # (-0.0 and 0.0: two bit patterns, two rows, one direction)
    for n in (1, 23):
        rect = PARENTS[np.arange(n) % len(PARENTS)]
        rot = rots[(np.arange(n) * 3) % len(rots)]
        for depth in (1, 2, 3):
            want_rect = np.stack([host_slots(r, STEP, depth) for r in rect])
            there = ~np.isnan(want_rect[..., 0])
            for strict in (False, True):
                cfg = raw_cfg(pkg, s, strict)
                got_rect, got_score, got_level = scene.pyr.expand_matches(cfg, s.pose, rot, rect, STEP, depth)
                assert got_rect.shape == (n, SLOTS[depth], 4)
                np.testing.assert_array_equal(bits(got_rect[there]), bits(want_rect[there]))
                assert np.all(np.isnan(got_rect[~there])) and np.all(np.isnan(got_score[~there])) and np.all(got_level[~there] == -1)
                slot_rot = np.broadcast_to(rot[:, None], there.shape)[there]
                want_score, want_level = scene.pyr.score_matches(cfg, s.pose, slot_rot, want_rect[there])
                np.testing.assert_array_equal(bits(got_score[there]), bits(want_score))
                np.testing.assert_array_equal(got_level[there], want_level)
                assert np.all(np.isfinite(want_score)) and np.all(want_level >= 0)


# ---- 5. the multi-request forms -------------------------------------------------------------------------------------
class Three:
    """three OCC scenes -- 67, 1 and 67 beams -- resident together: a map and pyramid each (ids 0, 10, 20), the scans and
    their angles in slots 0, 1, 2"""
    NAMES = ("occ_square", "occ_1beam", "edge_occ")

    def __init__(self, pkg, ctx, angles=True):
        self.pkg, self.ctx = pkg, ctx
        self.scenes = [Scene(pkg, ctx, name, fine=10 * k) for k, name in enumerate(self.NAMES)]
        for k, sc in enumerate(self.scenes):
            s = sc.s
            ctx.scan_store(k, s.scan[:, 0], s.scan[:, 1], s.scan[:, 2], s.scan[:, 3], s.scan[:, 4])
            if angles:
                ctx.scan_store_angles(k, s.angle)
        self.table = [(sc.pyr, k, sc.s.pose) for k, sc in enumerate(self.scenes)]

    def close(self):
        for sc in self.scenes:
            sc.close()


@pytest.fixture
def three(pkg, ctx, variant):
    t = Three(pkg, ctx)
    yield t
    t.close()


def lone_match(three, k, strict, shape, limits):
    sc = three.scenes[k]
    m = three.pkg.Matcher(three.ctx, "BF_M3RSM", raw_cfg(three.pkg, sc.s, strict), [sc.pyr, *limits])
    m.set_m3rsm_speculation(*shape)
    three.ctx.scan_select(k)  # (the slot's angles become the current scan's)
    r = m.process_scan(sc.fine, sc.s.pose)
    st = m.stats()
    out = dict(delta=r["delta"], prob=r["prob"], trace=m.m3rsm_trace(), scorer_calls=st["scorer_calls"],
               poses_evaluated=st["poses_evaluated"], super_steps=st["launches"] - 1)
    m.close()
    return out


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "default"])
def test_match_each_gives_every_request_its_lone_raw_match(three, strict):
    limits = three.scenes[0].s.limits  # (one matcher, one set of limits: the 33 x 33 scene's)
    shape = (32, 3)
    lone = [lone_match(three, k, strict, shape, limits) for k in range(3)]
    if strict:  # request 0 under its own limits: the golden match
        np.testing.assert_array_equal(bits(lone[0]["trace"]), bits(three.scenes[0].s.trace))
    m = three.pkg.Matcher(three.ctx, "BF_M3RSM", raw_cfg(three.pkg, three.scenes[0].s, strict), [three.scenes[0].pyr, *limits])
    m.set_m3rsm_speculation(*shape)
    for threads in (1, 4):
        m.set_m3rsm_threads(threads)
        got = m.m3rsm_match_each(three.table)
        for k in range(3):
            np.testing.assert_array_equal(bits(got[k]["delta"]), bits(lone[k]["delta"]))
            np.testing.assert_array_equal(bits([got[k]["prob"]]), bits([lone[k]["prob"]]))
            np.testing.assert_array_equal(bits(m.m3rsm_trace_each(k)), bits(lone[k]["trace"]))
            st = m.m3rsm_each_stats(k)
            assert {q: st[q] for q in ("scorer_calls", "poses_evaluated", "super_steps")} == \
                {q: lone[k][q] for q in ("scorer_calls", "poses_evaluated", "super_steps")}
        assert m.stats()["launches"] == 1 + max(q["super_steps"] for q in lone)
    m.close()


def test_match_many_returns_the_request_of_the_larger_lone_probability(three):
    limits = three.scenes[0].s.limits
    lone = [lone_match(three, k, True, (32, 3), limits) for k in (0, 2)]
    best = int(np.argmax([q["prob"] for q in lone]))
    assert lone[0]["prob"] != lone[1]["prob"]
    m = three.pkg.Matcher(three.ctx, "BF_M3RSM", raw_cfg(three.pkg, three.scenes[0].s), [three.scenes[0].pyr, *limits])
    for shape in ((32, 3), (0, 0)):
        m.set_m3rsm_speculation(*shape)
        got = m.m3rsm_match_many([three.table[0], three.table[2]])
        assert got["request"] == best and got["prob"] == lone[best]["prob"]
        np.testing.assert_array_equal(bits(got["delta"]), bits(lone[best]["delta"]))
    m.close()


def test_score_and_expand_requests_equal_the_single_request_calls(three):
    pkg, ctx = three.pkg, three.ctx
    rs = np.random.RandomState(5)
    n = 40
    request = rs.randint(0, 3, n).astype(np.int32)
    rot = rs.choice(np.array([0.0, 1 / 64, -1 / 64, 0.0174, -0.05]), n)
    rect = PARENTS[[0, 1, 2, 3, 4, 6, 7, 8]][rs.randint(0, 8, n)]  # (no reversed one: score_requests refuses it)
    for strict in (False, True):
        cfg = raw_cfg(pkg, three.scenes[0].s, strict)
        score, level = pkg.Pyramid.score_requests(ctx, cfg, three.table, request, rot, rect)
        xr, xs, xl = pkg.Pyramid.expand_requests(ctx, cfg, three.table, request, rot, rect, STEP, 2)
        for k, sc in enumerate(three.scenes):
            sel = request == k
            assert sel.any()
            ctx.scan_select(k)
            want, want_level = sc.pyr.score_matches(cfg, sc.s.pose, rot[sel], rect[sel])
            np.testing.assert_array_equal(bits(score[sel]), bits(want))
            np.testing.assert_array_equal(level[sel], want_level)
            wr, ws, wl = sc.pyr.expand_matches(cfg, sc.s.pose, rot[sel], rect[sel], STEP, 2)
            np.testing.assert_array_equal(bits(xr[sel]), bits(wr))
            np.testing.assert_array_equal(bits(xs[sel]), bits(ws))
            np.testing.assert_array_equal(xl[sel], wl)
            assert np.any(np.isfinite(ws))


# ---- 6. errors --------------------------------------------------------------------------------------------------------
def test_raw_exact_says_what_it_needs_and_launches_nothing(pkg, ctx, variant):
    t = Three(pkg, ctx, angles=False)
    try:
        sc = t.scenes[0]
        s = sc.s
        cfg = raw_cfg(pkg, s)
        m = sc.matcher(shape=(32, 3))
        upload_scan(ctx, s)
        m.process_scan(sc.fine, s.pose)
        before = m.stats()
        assert before["launches"] >= 2
        ctx.profile_enable(True)
        ctx.profile_read()
        # the current scan without angles: the pyramid's calls and the lone match, both routes
        upload_scan(ctx, s, angles=False)
        rot, rect = s.trace[:4, 0], s.trace[:4, 1:5]
        with pytest.raises(pkg.SlamHipError, match=ERR_STATE + ".*scan_set_angles"):
            sc.pyr.score_matches(cfg, s.pose, rot, rect)
        with pytest.raises(pkg.SlamHipError, match=ERR_STATE + ".*scan_set_angles"):
            sc.pyr.expand_matches(cfg, s.pose, rot, rect, STEP, 1)
        for shape in ((32, 3), (0, 0)):
            m.set_m3rsm_speculation(*shape)
            with pytest.raises(pkg.SlamHipError, match=ERR_STATE + ".*scan_set_angles"):
                m.process_scan(sc.fine, s.pose)
            assert m.stats()["launches"] == before["launches"] and m.stats()["scorer_calls"] == before["scorer_calls"]
        # slots without angles: the multi-request calls and the matches over them
        m.set_m3rsm_speculation(32, 3)
        req = np.zeros(4, np.int32)
        with pytest.raises(pkg.SlamHipError, match=ERR_STATE + ".*scan_store_angles"):
            pkg.Pyramid.score_requests(ctx, cfg, t.table, req, rot, rect)
        with pytest.raises(pkg.SlamHipError, match=ERR_STATE + ".*scan_store_angles"):
            pkg.Pyramid.expand_requests(ctx, cfg, t.table, req, rot, rect, STEP, 1)
        with pytest.raises(pkg.SlamHipError, match=ERR_STATE + ".*scan_store_angles"):
            m.m3rsm_match_each(t.table)
        with pytest.raises(pkg.SlamHipError, match=ERR_STATE + ".*scan_store_angles"):
            m.m3rsm_match_many(t.table)
        assert m.stats()["launches"] == 0
        assert ctx.profile_read()[1] == 0  # not one scoring launch since the profile was reset
        ctx.profile_enable(False)
        # one slot of three with angles is not enough; all three are
        ctx.scan_store_angles(0, s.angle)
        with pytest.raises(pkg.SlamHipError, match=ERR_STATE):
            pkg.Pyramid.score_requests(ctx, cfg, t.table, req, rot, rect)
        for k in (1, 2):
            ctx.scan_store_angles(k, t.scenes[k].s.angle)
        score, _ = pkg.Pyramid.score_requests(ctx, cfg, t.table, req, rot, rect)
        np.testing.assert_array_equal(score, s.trace[:4, 5])
        # a wrong count, an empty slot
        with pytest.raises(pkg.SlamHipError, match=ERR_INVALID):
            ctx.scan_store_angles(0, s.angle[:-1])
        with pytest.raises(pkg.SlamHipError, match=ERR_INVALID):
            ctx.scan_store_angles(7, s.angle)
        # scan_store into the slot drops its angles; scan_select of a slot with angles brings them along
        ctx.scan_select(0)
        got, _ = sc.pyr.score_matches(cfg, s.pose, rot, rect)
        np.testing.assert_array_equal(got, s.trace[:4, 5])
        ctx.scan_store(0, s.scan[:, 0], s.scan[:, 1], s.scan[:, 2], s.scan[:, 3], s.scan[:, 4])
        with pytest.raises(pkg.SlamHipError, match=ERR_STATE + ".*scan_store_angles"):
            pkg.Pyramid.score_requests(ctx, cfg, t.table, req, rot, rect)
        ctx.scan_select(0)
        with pytest.raises(pkg.SlamHipError, match=ERR_STATE + ".*scan_set_angles"):
            sc.pyr.score_matches(cfg, s.pose, rot, rect)
        # the other modes never ask
        host = pkg.spe_cfg(oope=pkg.OOPE_MAX, oie=s.oie, pose_trig=pkg.POSE_TRIG_HOST)
        assert np.all(np.isfinite(sc.pyr.score_matches(host, s.pose, rot, rect)[0]))
    finally:
        ctx.profile_enable(False)
        t.close()
