"""GPU suite: the co-resident hill-climbing chain (csrc/hc_resident.hip) with the term vector's fingerprint made by the
waves that do not sum (workgroups of 512 and 1024 threads), and its sweep when it has to poll more than once.
Neither may change a bit of what a match reports:
  * the co-resident launch (set_device_chain 2), the chain of kernels (1) and the host-driven matcher (0) give the same
    pose delta, probability, scorer-call count and observer's trace AS BIT PATTERNS -- over the beam counts at which the
    fingerprint shares of the non-summing waves begin, end and are empty, workgroup sizes, cell models, the tie check
    on and off, the inert tail on and off; for batches (the pair form, and nine chains) and a window OOPE;
  * the fingerprint is still looked at: a designed two-beam table on which a candidate's term vector is the base
    pose's with its two terms exchanged -- the same sum to the last bit, another vector -- must be scored once more in
    beam order (steps_rescored > 0) and end as the beam-order matcher does;
  * re-polls really run: a testing hook makes one workgroup ~2 us late with its granule in chosen super-steps; the
    sweeps of those super-steps take at least two polls (the poll counter in the debugging stamps) and results and
    traces are those of the undelayed run.  A delay, not a missing workgroup: nothing gives up."""
import ctypes as C
import types

import numpy as np
import pytest
from landscape_cases import HC_ORIGIN, HC_W, S, case_map, cell_pose, lvl
from synth import CELL_OCC, CELL_TBM, cast_scan, make_scene

import __graft_entry__ as ge

pytestmark = pytest.mark.gpu

# kept-beam counts: one beam; around one wave, one summing stride (256), 320 (the shares of a 512-thread workgroup's four
# non-summing waves: 80 each), around 512 and 1024 threads; the headline's 1080
BEAMS = (1, 63, 64, 65, 255, 256, 257, 320, 511, 513, 1023, 1025, 1080)
PRM = [20, 0.1, 0.1]


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
    """a context of libslamhip_testing.so -- the build with the test hooks compiled in"""
    c = pkg.Context(0, testing=True)
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).reshape(-1).view(np.uint64)


def assert_same_bits(t, want):
    """pose delta, probability, number of scorer calls and the observer's trace, as bit patterns"""
    assert t["n_calls"] == want["n_calls"]
    for key in ("delta", "prob", "poses", "scores"):
        assert np.array_equal(bits(t[key]), bits(want[key])), key
    assert np.array_equal(np.asarray(t["accepted"]), np.asarray(want["accepted"]))


def upload(pkg, ctx, sc, scan=None):
    s = scan if scan is not None else sc["scan"]
    ctx.upload_map(0, sc["map"])
    cos_a, sin_a = pkg.beam_trig(s.angle)
    ctx.scan_upload(s.range, cos_a, sin_a, s.weight, s.factor)


def matcher(pkg, ctx, mode, threads=0, tie=1, cfg=None, prm=PRM):
    m = pkg.Matcher(ctx, "HC", cfg if cfg is not None else pkg.spe_cfg(), prm)
    m.set_device_chain(mode, threads)
    m.set_tie_check(tie)
    return m


_scenes = {}


def scene_of(cell):
    """one scene per cell model, made once; its scan thinned to n beams by a fixed draw"""
    if cell not in _scenes:
        _scenes[cell] = make_scene(cell_model=cell, size=400, scale=0.1, n_beams=1080, seed=7,
                                   weighting="even" if cell == CELL_OCC else "viny")
    return _scenes[cell]


def thinned(sc, n):
    s = sc["scan"]
    keep = np.sort(np.random.RandomState(3 + n).choice(s.n, min(n, s.n), replace=False))
    return types.SimpleNamespace(range=s.range[keep], angle=s.angle[keep], weight=s.weight[keep], factor=s.factor[keep], n=keep.size)


_refs = {}


def host_reference(pkg, ctx, cell, n, tie):
    """the host-driven matcher's match (it knows no inert tail and no workgroups): computed once, left unchanged"""
    key = (cell, n, tie)
    if key not in _refs:
        h = matcher(pkg, ctx, 0, tie=tie)
        t = h.process_scan(0, scene_of(cell)["init_pose"], trace=True)
        t["scorer_calls"] = h.stats()["scorer_calls"]
        h.close()
        for a in (t["poses"], t["scores"], t["accepted"], t["delta"]):
            a.setflags(write=False)
        _refs[key] = t
    return _refs[key]


@pytest.mark.parametrize("cell", [CELL_OCC, CELL_TBM], ids=["OCC", "TBM"])
@pytest.mark.parametrize("threads", [256, 512, 1024])
def test_three_forms_give_the_same_bits(pkg, ctx, threads, cell):
    sc = scene_of(cell)
    for n in BEAMS:
        upload(pkg, ctx, sc, thinned(sc, n))
        for tie in (1, 0):
            want = host_reference(pkg, ctx, cell, n, tie)
            for inert in (0, 2):
                ctx.set_option(pkg.OPT_INERT_TAIL, inert)
                try:
                    for mode in (2, 1):
                        m = matcher(pkg, ctx, mode, threads, tie)
                        t = m.process_scan(0, sc["init_pose"], trace=True)
                        assert_same_bits(t, want)
                        assert m.stats()["scorer_calls"] == want["scorer_calls"] == t["n_calls"]
                        if mode == 2:
                            assert m.resident_stats() == dict(matches=1, gave_up=0) and m.stats()["kernels_launched"] == 1
                        q = m.process_scan(0, sc["init_pose"])  # no observer
                        assert np.array_equal(bits(q["delta"]), bits(want["delta"])) and np.array_equal(bits(q["prob"]), bits(want["prob"]))
                        m.close()
                finally:
                    ctx.set_option(pkg.OPT_INERT_TAIL, 2)


def batch_jobs(pkg, ctx, k, n_beams):
    """k jobs on two maps: scans of n_beams beams cast from jittered poses, initial poses with growing errors"""
    worlds = []
    for mi, size in enumerate((400, 300)):
        sc = make_scene(cell_model=CELL_OCC, size=size, scale=0.1, n_beams=n_beams, seed=5 + mi)
        ctx.upload_map(mi, sc["map"])
        worlds.append(sc)
    rs = np.random.RandomState(100 + k)
    jobs = []
    for j in range(k):
        sc = worlds[j % 2]
        true = sc["true_pose"] + rs.randn(3) * [0.15, 0.15, 0.05]
        rng, ang = cast_scan(sc["gt"], 0.1, true, n_beams, seed=42 + j)
        cos_a, sin_a = pkg.beam_trig(ang)
        err = np.array([0.07, -0.04, 0.03]) * (3.0 * j / max(k - 1, 1))
        jobs.append(dict(map_id=j % 2, range=rng, cos_a=cos_a, sin_a=sin_a, weight=np.full(rng.size, 1.0 / rng.size),
                         factor=None, init_pose=true + err))
    return jobs


@pytest.mark.parametrize("k", [3, 9])
def test_batches_give_the_same_bits(pkg, ctx, k):
    """three chains (workgroups of 512 threads that score two poses each) and nine, on 90 beams: every job as its lone
    host-driven match"""
    jobs = batch_jobs(pkg, ctx, k, 90)
    got = {}
    for mode in (2, 1):
        mb = matcher(pkg, ctx, mode)
        got[mode] = mb.process_scan_batch(jobs, trace=True)
        st = [mb.batch_stats(j) for j in range(k)]
        assert all(s["on_device_chain"] for s in st)
        got[mode, "calls"] = [s["scorer_calls"] for s in st]
        if mode == 2:
            assert mb.resident_stats() == dict(matches=1, gave_up=0) and mb.stats()["kernels_launched"] == 1
        mb.close()
    host = matcher(pkg, ctx, 0)
    for j, job in enumerate(jobs):
        ctx.scan_upload(job["range"], job["cos_a"], job["sin_a"], job["weight"], np.ones(job["range"].size))
        want = host.process_scan(job["map_id"], job["init_pose"], trace=True)
        for mode in (2, 1):
            assert_same_bits(got[mode][j], want)
            assert got[mode, "calls"][j] == want["n_calls"] == host.stats()["scorer_calls"]
    host.close()
    ctx.map_release(1)


def test_window_oope_gives_the_same_bits(pkg, ctx):
    sc = make_scene(cell_model=CELL_OCC, size=400, scale=0.1, n_beams=90, seed=5)
    upload(pkg, ctx, sc)
    cfg = pkg.spe_cfg(oope=pkg.OOPE_MAX, area=(-0.12, 0.12, -0.08, 0.08))
    host = matcher(pkg, ctx, 0, cfg=cfg)
    want = host.process_scan(0, sc["init_pose"], trace=True)
    for mode in (2, 1):
        m = matcher(pkg, ctx, mode, cfg=cfg)
        assert_same_bits(m.process_scan(0, sc["init_pose"], trace=True), want)
        assert m.stats()["scorer_calls"] == host.stats()["scorer_calls"] == want["n_calls"]
        if mode == 2:
            assert m.resident_stats() == dict(matches=1, gave_up=0) and m.stats()["kernels_launched"] == 1
        m.close()
    host.close()


# ---- the fingerprint is still looked at --------------------------------------------------------------------------------
def exchanged_terms_table():
    """Two beams along +x, of range 0 and of two cells, weight 1/2 each; columns alike in every row.  Around the start
    column i0 the columns hold  low, A, B, B, A, low ...: the base pose reads (A, B), the candidate one cell -- and
    later half a cell -- further in +x reads (B, A): A/2 + B/2 in both orders of both sums, to the last bit, from a
    different term vector.  -x reads (low, B), a clear rejection; the steps in y and the rotations (the far beam's end
    moves by a fifth of a cell in y, a hundredth in x) stay in their cells: identical vectors.  The start pose sits at
    0.7 / 0.5 of its cell, so that no halved step puts an end point on a cell edge."""
    i0 = 8
    t = np.full((HC_W, HC_W), lvl(0))
    a, b = lvl(3), lvl(5)
    t[:, i0], t[:, i0 + 1], t[:, i0 + 2], t[:, i0 + 3] = a, b, b, a
    c = types.SimpleNamespace(payload=np.ascontiguousarray(t), origin=HC_ORIGIN)
    return c, cell_pose(HC_ORIGIN, i0, 8, 0.7, 0.5)


@pytest.mark.parametrize("threads", [512, 1024])
def test_exchanged_terms_are_told_apart_by_the_fingerprint(pkg, ctx, threads):
    import pyoracle as po
    c, init = exchanged_terms_table()
    ctx.upload_map(0, case_map(c, po))
    ctx.scan_upload([0.0, 2 * S], [1.0, 1.0], [0.0, 0.0], [0.5, 0.5])
    prm = [6, S, 0.1]
    seq = pkg.Matcher(ctx, "HC", pkg.spe_cfg(sum_order=1), prm)  # the beam-order matcher
    want = seq.process_scan(0, init, trace=True)
    assert want["n_calls"] > 6 * 6 and not np.any(want["accepted"][1:])  # the design: ties and rejections only
    m = matcher(pkg, ctx, 2, threads, tie=1, prm=prm)
    t = m.process_scan(0, init, trace=True)
    st = m.stats()
    assert m.resident_stats() == dict(matches=1, gave_up=0) and st["kernels_launched"] == 1
    assert st["steps_rescored"] > 0  # equal sums of different vectors: only the fingerprints say so
    assert_same_bits(t, want)
    assert st["scorer_calls"] == want["n_calls"]
    # ... and without the check nobody looks: nothing is scored twice
    raw = matcher(pkg, ctx, 2, threads, tie=0, prm=prm)
    assert_same_bits(raw.process_scan(0, init, trace=True), want)
    assert raw.stats()["steps_rescored"] == 0
    for x in (seq, m, raw):
        x.close()


# ---- re-polls really run -----------------------------------------------------------------------------------------------
BOOKKEEPING = 0xffff  # the delay hook's name for the launch's last workgroup


def late(workgroup, every, phase):
    """argument of slamhip_matcher_debug_resident_mute that delays instead of muting: workgroup `workgroup` (BOOKKEEPING:
    the last one) spends ~2 us in front of its granule's store in the super-steps k with k % every == phase"""
    return -((BOOKKEEPING if workgroup == BOOKKEEPING else workgroup + 1) + 65536 * (every + 16 * phase))


@pytest.mark.parametrize("workgroup", [0, 126, 251, BOOKKEEPING], ids=["first", "middle", "last", "bookkeeping"])
def test_a_late_granule_costs_a_re_poll_and_changes_nothing(pkg, tctx, workgroup):
    ctx = tctx
    sc = make_scene(cell_model=CELL_OCC, size=400, scale=0.1, n_beams=720, seed=5)
    upload(pkg, ctx, sc)
    L = pkg.load(testing=True)
    L.slamhip_matcher_debug_resident_mute.argtypes = [C.c_void_p, C.c_int]
    L.slamhip_matcher_debug_resident_mute.restype = C.c_int
    L.slamhip_matcher_debug_stamps.argtypes = [C.c_void_p, C.POINTER(C.c_longlong)]
    m = matcher(pkg, ctx, 2, 1024, prm=[128, 0.1, 0.1])
    want = m.process_scan(0, sc["init_pose"], trace=True)
    calls = m.stats()["scorer_calls"]
    L.slamhip_matcher_debug_stamps(m.h, None)
    assert L.slamhip_matcher_debug_resident_mute(m.h, late(workgroup, 2, 1)) == 0  # super-steps 1, 3, 5, ...
    got = m.process_scan(0, sc["init_pose"], trace=True)
    assert L.slamhip_matcher_debug_resident_mute(m.h, 0) == 0
    assert_same_bits(got, want)
    assert m.stats()["scorer_calls"] == calls
    assert m.resident_stats() == dict(matches=2, gave_up=0) and m.stats()["kernels_launched"] == 1
    buf = (C.c_longlong * 512)()
    L.slamhip_matcher_debug_stamps(m.h, buf)
    st = np.array(list(buf)).reshape(64, 8)
    # spare stamp 6 of the super-steps from the fourth on: polls of workgroup 1's sweep | granules missing behind the first << 32
    rows = [k for k in range(3, 64) if st[k, 6] != 0]
    polls = {k: int(st[k, 6]) & 0xffffffff for k in rows}
    print("REPOLL late workgroup %s: polls per sweep %r, missing behind the first poll %r"
          % (workgroup, polls, {k: int(st[k, 6]) >> 32 for k in rows}))
    delayed = [k for k in rows if k % 2 == 1]
    assert len(delayed) >= 2, rows  # the match is long enough to show it
    assert all(polls[k] >= 2 for k in delayed), polls
    assert all(int(st[k, 6]) >> 32 >= 1 for k in delayed)
    m.close()
