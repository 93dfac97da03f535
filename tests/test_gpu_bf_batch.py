"""GPU suite: K brute-force sweeps per call, every job on its own enumerator stream (slamhip_matcher_set_bf_streams;
csrc/bf_batch.hip: score, scan, decide with grid.y = job) -- BruteForceScanMatcher::process_scan once per robot, every
robot owning its matcher and with it a BruteForcePoseEnumerator that latches its base pose at the first next() of its life
(brute_force_scan_matcher.h:27-40).

The bar throughout is bit equality, assert_trace_equal / assert_array_equal without a tolerance: job j of a batch against a
LONE pkg.Matcher(ctx, "BF", ...) per stream, fed that stream's jobs in order, and -- on the designed landscapes, which the
oracle covers -- against the CPU oracle's enumerator.  What may not matter: the batch size, the other jobs of the batch,
the route a job took (shared launches / lone call on its stream).

Apart from the designed ambiguous job (4), the 4097-beam job (3) and the fall-back configurations (8) no job may leave
the shared launches: every test asserts on_device_chain for all of its jobs.  The random scenes are chosen so that the
LONE sweep settles them on the device (its kernels_launched == 4: poses, sweep, scan, decide), which check_batch asserts
of every lone match it runs."""
import numpy as np
import placed_scenes as ps
import pyoracle as po
import pytest
import test_gpu_mc_batch as mcb
import test_gpu_raw_batch as rb
from landscape_cases import case_map, cases_of, oracle_matches
from synth import CELL_GMAPPING, CELL_OCC, CELL_TBM, cast_scan, make_scene

import __graft_entry__ as ge

pytestmark = pytest.mark.gpu

R9 = [-0.2, 0.2, 0.05, -0.2, 0.2, 0.05, -0.06, 0.06, 0.02]  # 9 x 9 x 7: K = 3 makes two poses per scoring workgroup
# (the raw worlds' one-beam job scores single cells: on these ranges, with these weightings and 257 kept beams in job 1, the
# LONE sweep settles every job of the raw tests on the device -- checked once on the card, asserted in the tests)
R9_RAW = [-0.2, 0.2, 0.05, -0.2, 0.2, 0.05, -0.04, 0.04, 0.02]
STRICT = dict(sum_order=1, pose_trig=1)  # SLAMHIP_SUM_SEQUENTIAL, SLAMHIP_POSE_TRIG_HOST
BF = cases_of("BF")
same_trace, close_all = mcb.same_trace, mcb.close_all


def n_poses(m9):
    """1 + nx ny nt of a range9, by the enumerator's own accumulation"""
    def axis(lo, to, step, below):
        n, v = 0, lo
        while True:
            if not below and not v <= to:
                return n
            n += 1
            if below and not v < to:
                return n
            v += step
    return 1 + axis(*m9[0:3], True) * axis(*m9[3:6], True) * axis(*m9[6:9], False)


@pytest.fixture(scope="module")
def pkg():
    return ge.load_package()


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def matchers(pkg, ctx, k, r9=R9, cfg=None, streams=True):
    cfg = cfg or (lambda: pkg.spe_cfg())
    mb = pkg.Matcher(ctx, "BF", cfg(), r9)
    if streams:
        mb.set_bf_streams(k)
    return mb, [pkg.Matcher(ctx, "BF", cfg(), r9) for _ in range(k)]


def same_info(a, b):
    assert a["base_set"] == b["base_set"] and a["matches"] == b["matches"], (a, b)
    np.testing.assert_array_equal(a["base"], b["base"])


def check_batch(ctx, mb, lones, jobs, got, stream_of=None, chains=True, lone_kernels=4, r9=R9, lone_fn=None):
    """every job against its stream's lone matcher: trace, counters, route, the stream's record against the lone
    matcher's own enumerator"""
    calls = 0
    for j, (g, job) in enumerate(zip(got, jobs)):
        s = j if stream_of is None else stream_of[j]
        want = (lone_fn or mcb.lone)(ctx, lones[s], job)
        same_trace(g, want)
        st = mb.batch_stats(j)
        on = chains if isinstance(chains, bool) else chains[j]
        assert st["on_device_chain"] == on, j
        assert st["scorer_calls"] == want["n_calls"] == lones[s].stats()["scorer_calls"] == n_poses(r9), j
        if lone_kernels is not None and on:  # (the condition on the inputs: the lone sweep settles them on the device)
            assert lones[s].stats()["kernels_launched"] == lone_kernels, j
        same_info(mb.bf_stream_info(s), lones[s].bf_stream_info(-1))
        calls += st["scorer_calls"]
    assert mb.stats()["scorer_calls"] == calls


# ---- 1. three calls on K streams: the base stays latched
@pytest.mark.parametrize("cell,weighting,plane,slots", [(CELL_OCC, "even", 1, False), (CELL_TBM, "viny", 1, True),
                                                        (CELL_TBM, "even", 0, False), (CELL_OCC, "viny", 1, True)])
def test_three_calls_on_three_streams_keep_the_latched_bases(pkg, ctx, cell, weighting, plane, slots):
    k = 3
    jobs = mcb.scenes(pkg, ctx, cell, weighting, k)
    ctx.set_option(pkg.OPT_TBM_PLANE, plane)
    mb, lones = matchers(pkg, ctx, k)
    try:
        first = None
        for call in range(3):
            # another initial pose for every stream in every call: calls 2 and 3 enumerate around call 1's
            turn = [dict(j, init_pose=j["init_pose"] + np.array([0.013, -0.021, 0.004]) * call) for j in jobs]
            if first is None:
                first = [np.array(j["init_pose"], dtype=np.float64) for j in turn]
            sent = turn
            if slots:  # (stored scans instead of arrays)
                sent = []
                for j, job in enumerate(turn):
                    ctx.scan_store(40 + j, job["range"], job["cos_a"], job["sin_a"], job["weight"])
                    sent.append(dict(map_id=job["map_id"], scan_slot=40 + j, init_pose=job["init_pose"]))
            got = mb.process_scan_batch(sent, trace=True)
            check_batch(ctx, mb, lones, turn, got)
            assert mb.chain_stats()["kernels_launched"] == 3
            for j in range(k):
                info = mb.bf_stream_info(j)
                assert info["base_set"] and info["matches"] == call + 1
                np.testing.assert_array_equal(info["base"], first[j])
                if call:  # (the candidates lie around call 1's pose, not this call's)
                    np.testing.assert_array_equal(got[j]["poses"][1], first[j] + [R9[0], R9[3], R9[6]])
        # a lone call on the batch matcher: its OWN enumerator, still unlatched until now
        own = mb.bf_stream_info(-1)
        assert not own["base_set"] and own["matches"] == 0
        fresh = pkg.Matcher(ctx, "BF", pkg.spe_cfg(), R9)
        same_trace(mcb.lone(ctx, mb, jobs[1]), mcb.lone(ctx, fresh, jobs[1]))
        own = mb.bf_stream_info(-1)
        assert own["base_set"] and own["matches"] == 1
        np.testing.assert_array_equal(own["base"], jobs[1]["init_pose"])
        fresh.close()
        # without an observer: the lone matchers' next match
        got = mb.process_scan_batch(jobs)
        for j, g in enumerate(got):
            w = mcb.lone(ctx, lones[j], jobs[j], trace=False)
            assert g["prob"] == w["prob"] and np.array_equal(g["delta"], w["delta"])
            assert mb.batch_stats(j)["on_device_chain"]
    finally:
        ctx.set_option(pkg.OPT_TBM_PLANE, 1)
        close_all(mb, lones)


# ---- 2. the arg-max's edges on designed landscapes, as jobs of one batch
_refs = {}


def ref_of(c, oracle):
    if c.name not in _refs:
        _refs[c.name] = oracle_matches(c, oracle, po)
    return _refs[c.name]


def landscape_job(c, map_id, init=None, weight=1.0):
    return dict(map_id=map_id, range=[c.rng], cos_a=[1.0], sin_a=[0.0], weight=[weight], factor=[1.0],
                init_pose=c.inits[0] if init is None else init)


def landscape_lone(ctx, m, job):
    ctx.scan_upload(job["range"], job["cos_a"], job["sin_a"], job["weight"], job["factor"])
    return m.process_scan(job["map_id"], job["init_pose"], trace=True)


@pytest.mark.parametrize("names", [("n1025-max_at_1024", "n1025-tie_1024_1025", "n1025-staircase", "n1025-initial_is_max",
                                    "n1025-nan_everything", "n1025-max_at_1025"),
                                   ("n1024-max_at_1024", "n1024-tie_1023_1024", "n1024-staircase", "n1024-initial_is_max")],
                         ids=["1+1025", "1+1024"])
def test_argmax_edges_as_jobs_of_one_batch(pkg, ctx, oracle, names):
    """All jobs of a matcher share its ranges, so the tables of 1 + 1025 poses (the maximum on the last candidate of block
    0, a tie across the seam 1024 | 1025, a staircase over it, the initial pose as the maximum: best index 0, nothing
    accepted) are one batch and the tables of exactly 1 + 1024 poses another.  One more job scores a table through a scan
    of zero total weight: every score NaN, nothing accepted."""
    cases = [c for n in names for c in BF if c.name == n]
    assert len(cases) == len(names) and len({c.shape for c in cases}) == 1
    for k, c in enumerate(cases):
        ctx.upload_map(k, case_map(c, po))
    jobs = [landscape_job(c, k) for k, c in enumerate(cases)] + [landscape_job(cases[0], 0, weight=0.0)]
    k = len(jobs)
    for strict in (False, True):
        cfg = (lambda: pkg.spe_cfg(**STRICT)) if strict else None
        mb, lones = matchers(pkg, ctx, k, r9=cases[0].params, cfg=cfg)
        try:
            for call in range(2):
                got = mb.process_scan_batch(jobs, trace=True)
                check_batch(ctx, mb, lones, jobs, got, chains=not strict, lone_kernels=None if strict else 4,
                            r9=cases[0].params, lone_fn=landscape_lone)
                for j, c in enumerate(cases):  # the goldens' source: the oracle's enumerator
                    same_trace(got[j], ref_of(c, oracle)[0])
                assert np.isnan(got[-1]["prob"]) and not got[-1]["delta"].any() and got[-1]["accepted"][1:].sum() == 0
                assert np.isnan(got[-1]["scores"]).all()
                j0 = names.index([n for n in names if n.endswith("initial_is_max")][0])
                assert not got[j0]["delta"].any() and got[j0]["accepted"][1:].sum() == 0
        finally:
            close_all(mb, lones)
    for k in range(1, len(cases)):
        ctx.map_release(k)


# ---- 3. beam counts at the scorer's edges in one batch
def test_beam_counts_at_the_scorers_edges_in_one_batch(pkg, ctx):
    mcb.scenes(pkg, ctx, CELL_OCC, "even", 2)  # (the maps)
    counts = [1, 255, 256, 257, 1280, 1281, 4096]
    sc = mcb.worlds_of(CELL_OCC, "even")[0]
    rng0, ang0 = cast_scan(sc["gt"], 0.05, sc["true_pose"], 4097, seed=9)
    assert rng0.size >= 4097 - 64  # (beams that hit nothing are dropped by the caster)

    def job_of(n, j):
        idx = np.resize(np.arange(rng0.size), n) if n > rng0.size else np.linspace(0, rng0.size - 1, n).astype(int)
        rng, ang = rng0[idx], ang0[idx]
        cos_a, sin_a = pkg.beam_trig(ang)
        return dict(map_id=0, range=rng, cos_a=cos_a, sin_a=sin_a, weight=np.full(n, 1.0 / n), factor=None,
                    init_pose=sc["true_pose"] + np.array([0.05, -0.03, 0.02]) * (1 + j % 3))

    jobs = [job_of(n, j) for j, n in enumerate(counts)]
    k = len(jobs)
    mb, lones = matchers(pkg, ctx, k + 1)
    try:
        got = mb.process_scan_batch(jobs, trace=True)  # (1281 and 4096 beams: the generic instantiation for all seven)
        check_batch(ctx, mb, lones, jobs, got)
        assert mb.chain_stats()["kernels_launched"] == 3
        # pairs: a short scan beside a long one under the max-KB instantiations and under the generic one
        for a, b in ((0, 1), (0, 2), (1, 3), (0, 4), (3, 4), (0, 5), (4, 5), (0, 6), (2, 6)):
            mb.set_bf_job_streams([a, b])
            got = mb.process_scan_batch([jobs[a], jobs[b]], trace=True)
            check_batch(ctx, mb, lones, [jobs[a], jobs[b]], got, stream_of=[a, b])
        # 4097 beams: that job alone leaves the shared launches, on its own stream
        sid = [0, 1, 7, 2, 3]
        jobs2 = jobs[:2] + [job_of(4097, 1)] + jobs[2:4]
        mb.set_bf_job_streams(sid)
        got = mb.process_scan_batch(jobs2, trace=True)
        check_batch(ctx, mb, lones, jobs2, got, stream_of=sid, chains=[True, True, False, True, True])
        assert mb.chain_stats()["kernels_launched"] == 3
    finally:
        close_all(mb, lones)


# ---- 4. an ambiguous job leaves alone
def test_an_ambiguous_job_leaves_alone(pkg, ctx, oracle):
    hard = [c for c in BF if c.settles != "device" and c.shape == (64, 32, 1)][0]
    easy = [c for c in BF if c.name in ("n2048-max_at_1024", "n2048-staircase")]
    assert len(easy) == 2 and all(c.settles == "device" for c in easy)
    cases = [easy[0], hard, easy[1]]
    for k, c in enumerate(cases):
        ctx.upload_map(k, case_map(c, po))
    jobs = [landscape_job(c, k) for k, c in enumerate(cases)]
    mb, lones = matchers(pkg, ctx, 3, r9=hard.params)
    try:
        for call in range(2):
            got = mb.process_scan_batch(jobs, trace=True)
            check_batch(ctx, mb, lones, jobs, got, chains=[True, False, True], r9=hard.params, lone_fn=landscape_lone)
            assert lones[1].stats()["kernels_launched"] == 0  # (the lone sweep left the device as well)
            for j, c in enumerate(cases):
                same_trace(got[j], ref_of(c, oracle)[0])
            assert [mb.bf_stream_info(j)["matches"] for j in range(3)] == [call + 1] * 3
    finally:
        close_all(mb, lones)
        for k in (1, 2):
            ctx.map_release(k)


# ---- 5. observer
def test_observer_sequences_come_per_job_in_job_order(pkg, ctx):
    k = 3
    jobs = mcb.scenes(pkg, ctx, CELL_OCC, "viny", k)
    mb, lones = matchers(pkg, ctx, k)
    try:
        blk = mb.make_batch(jobs)
        events = []
        obs = pkg.Observer(None, pkg.OBS_FN(lambda _u, p, s: events.append(("test", p[0], p[1], p[2], s))),
                           pkg.OBS_FN(lambda _u, p, s: events.append(("update", p[0], p[1], p[2], s))),
                           pkg.OBS_FN(lambda _u, d, s: events.append(("end", d[0], d[1], d[2], s))))
        import ctypes as C
        assert mb.L.slamhip_matcher_set_observer(mb.h, C.byref(obs)) == 0
        mb._obs_cleared = False
        fn = mb.L.slamhip_matcher_process_scan_batch
        deltas, probs = np.zeros((k, 3)), np.zeros(k)
        dp = C.POINTER(C.c_double)
        assert fn(mb.h, k, blk["arr"], deltas.ctypes.data_as(dp), probs.ctypes.data_as(dp)) == 0
        assert mb.L.slamhip_matcher_set_observer(mb.h, None) == 0
        mb._obs_cleared = True
        ends = [i for i, e in enumerate(events) if e[0] == "end"]
        assert len(ends) == k and ends[-1] == len(events) - 1
        at = 0
        for j, end in enumerate(ends):  # job j's events: every test, the updates behind their tests, on_matching_end
            want = mcb.lone(ctx, lones[j], jobs[j])
            seq = []
            for p, s, acc in zip(want["poses"], want["scores"], want["accepted"]):
                seq.append(("test", p[0], p[1], p[2], s))
                if acc:
                    seq.append(("update", p[0], p[1], p[2], s))
            seq.append(("end", want["delta"][0], want["delta"][1], want["delta"][2], want["prob"]))
            assert events[at:end + 1] == seq, j
            assert mb.batch_stats(j)["on_device_chain"]
            at = end + 1
    finally:
        close_all(mb, lones)


# ---- 6. the raw form
raw_worlds = mcb.raw_worlds  # (the module-scoped fixture: the worlds of tests/test_gpu_raw_batch.py with both scanners' scans)


@pytest.mark.parametrize("cell,weighting,trig", [(CELL_OCC, "viny", "raw"), (CELL_TBM, "ahr", "cached"), (CELL_OCC, "ahr", "raw"),
                                                 (CELL_TBM, "viny", "cached")])
def test_raw_batch_equals_lone_raw_calls(pkg, ctx, raw_worlds, cell, weighting, trig):
    rb.upload(ctx, raw_worlds, cell)
    ws = raw_worlds[cell]
    three = rb.three_jobs(pkg, ws, trig, weighting, 257)
    empty = rb.raw_job(pkg, ws[1], 1, rb.N_B, trig, weighting, is_occ=np.zeros(rb.N_B, np.int32))
    jobs = [three[0], three[1], empty, three[2]]
    k = len(jobs)
    mb, lones = matchers(pkg, ctx, k, r9=R9_RAW)
    try:
        got = mb.process_raw_scan_batch(jobs, trace=True)
        assert mb.chain_stats()["kernels_launched"] == 4
        for j, (g, job) in enumerate(zip(got, jobs)):
            want = rb.lone_raw(pkg, lones[j], job)
            assert g["kept"] == want["kept"], j
            st = mb.batch_stats(j)
            if j == 2:  # nothing kept: NaN, zero delta, no observer call, the stream still unlatched
                assert want["kept"] == 0 and np.isnan(g["prob"]) and not g["delta"].any() and g["n_calls"] == 0
                assert st == dict(scorer_calls=0, poses_evaluated=0, super_steps=0, on_device_chain=False)
                info = mb.bf_stream_info(2)
                assert not info["base_set"] and info["matches"] == 0
            else:
                same_trace(g, want)
                assert st["on_device_chain"] and st["scorer_calls"] == want["n_calls"] == n_poses(R9_RAW)
                assert lones[j].stats()["kernels_launched"] == 4, j
                np.testing.assert_array_equal(rb.bits(mb.batch_scan_download(j)), rb.download(ctx), err_msg="scan block of job %d" % j)
            same_info(mb.bf_stream_info(j), lones[j].bf_stream_info(-1))
        # the NEXT call: stream 2 meets a scan that keeps points and latches at THIS call's pose; the others stay
        second = dict(three[1], init_pose=three[1]["init_pose"] + [0.05, 0.02, -0.01])
        jobs2 = [dict(three[0], init_pose=three[0]["init_pose"] + [0.02, 0.0, 0.01]), three[1], second, three[2]]
        got = mb.process_raw_scan_batch(jobs2, trace=True)
        for j, (g, job) in enumerate(zip(got, jobs2)):
            want = rb.lone_raw(pkg, lones[j], job)
            assert g["kept"] == want["kept"] and mb.batch_stats(j)["on_device_chain"], j
            same_trace(g, want)
            same_info(mb.bf_stream_info(j), lones[j].bf_stream_info(-1))
        np.testing.assert_array_equal(mb.bf_stream_info(2)["base"], second["init_pose"])
        np.testing.assert_array_equal(mb.bf_stream_info(0)["base"], three[0]["init_pose"])
        # one non-empty job: the lone raw call on that job's stream
        mb.set_bf_job_streams([3, 1])
        got = mb.process_raw_scan_batch([empty, jobs[1]], trace=True)
        same_trace(got[1], rb.lone_raw(pkg, lones[1], jobs[1]))
        assert not mb.batch_stats(1)["on_device_chain"] and got[0]["kept"] == 0
        same_info(mb.bf_stream_info(1), lones[1].bf_stream_info(-1))
        same_info(mb.bf_stream_info(3), lones[3].bf_stream_info(-1))
    finally:
        close_all(mb, lones)


# ---- 7. mapping and refusals
def test_mapping_and_refusals(pkg, ctx):
    k = 4
    jobs = mcb.scenes(pkg, ctx, CELL_OCC, "even", k)
    mb, lones = matchers(pkg, ctx, k)
    hc = pkg.Matcher(ctx, "HC", pkg.spe_cfg(), [6, 0.1, 0.1])
    try:
        perm = [2, 0, 3, 1]
        mb.set_bf_job_streams(perm)
        got = mb.process_scan_batch(jobs, trace=True)
        check_batch(ctx, mb, lones, jobs, got, stream_of=perm)
        # fewer jobs than streams
        mb.set_bf_job_streams([3, 1])
        got = mb.process_scan_batch(jobs[:2], trace=True)
        check_batch(ctx, mb, lones, jobs[:2], got, stream_of=[3, 1])
        mb.set_bf_job_streams(None)

        def state():
            infos = [mb.bf_stream_info(j) for j in range(-1, k)]
            return ([(i["base_set"], i["matches"], i["base"].tolist()) for i in infos], mb.stats(),
                    [mb.batch_stats(j) for j in range(2)])

        before = state()
        for bad, text in (([0, 1, 1, 2], "same enumerator stream"), ([0, 1, 2, 4], "out of range"), ([0, -1], "out of range"),
                          ([0, 1, 2, 3, 0], "more jobs than")):
            with pytest.raises(pkg.SlamHipError, match=text):
                mb.set_bf_job_streams(bad)
        with pytest.raises(pkg.SlamHipError, match="more jobs than"):
            mb.process_scan_batch(jobs + jobs[:1])
        mb.set_bf_job_streams([3, 2])
        with pytest.raises(pkg.SlamHipError, match="more jobs than"):  # (than the mapping names)
            mb.process_scan_batch(jobs[:3])
        mb.set_bf_job_streams(None)
        with pytest.raises(pkg.SlamHipError, match="unknown map id"):
            mb.process_scan_batch([jobs[0], dict(jobs[1], map_id=17)])
        ctx.upload_map(5, make_scene(cell_model=CELL_GMAPPING, size=120, scale=0.05, n_beams=90)["map"])
        with pytest.raises(pkg.SlamHipError):
            mb.process_scan_batch([jobs[0], dict(jobs[1], map_id=5)])
        ctx.upload_map(6, mcb.worlds_of(CELL_TBM, "even")[0]["window"])
        with pytest.raises(pkg.SlamHipError, match="share a cell model"):
            mb.process_scan_batch([jobs[0], dict(jobs[1], map_id=6)])
        for fn in (lambda: hc.set_bf_streams(2), lambda: hc.set_bf_job_streams([0]), lambda: hc.bf_stream_info(-1)):
            with pytest.raises(pkg.SlamHipError, match="brute-force"):
                fn()
        assert state() == before
        for mid in (5, 6):
            ctx.map_release(mid)
        got = mb.process_scan_batch(jobs, trace=True)  # the next valid call: the streams' sequences go on
        check_batch(ctx, mb, lones, jobs, got)
        # reset_state: the bases stay
        mb.reset_state()
        for m in lones:
            m.reset_state()
        got = mb.process_scan_batch(jobs, trace=True)
        check_batch(ctx, mb, lones, jobs, got)
        # the streams set anew: every base forgotten
        mb.set_bf_streams(k)
        assert [mb.bf_stream_info(j)["base_set"] for j in range(k)] == [False] * k
        fresh = [pkg.Matcher(ctx, "BF", pkg.spe_cfg(), R9) for _ in range(k)]
        turn = [dict(j, init_pose=j["init_pose"] + [0.01, 0.01, 0.0]) for j in jobs]
        got = mb.process_scan_batch(turn, trace=True)
        check_batch(ctx, mb, fresh, turn, got)
        # the streams removed: job after job on the matcher's own enumerator, as without these calls
        mb.set_bf_streams(0)
        one = pkg.Matcher(ctx, "BF", pkg.spe_cfg(), R9)
        got = mb.process_scan_batch(jobs[:3], trace=True)
        for j, g in enumerate(got):
            same_trace(g, mcb.lone(ctx, one, jobs[j]))
            assert not mb.batch_stats(j)["on_device_chain"]
        close_all(fresh, one)
    finally:
        close_all(mb, lones, hc)


# ---- 8. fall-backs on the job's own stream
@pytest.mark.parametrize("what", ["oope_max", "sum_sequential", "device_chain_off"])
def test_fallbacks_run_on_the_jobs_own_streams(pkg, ctx, what):
    k = 3
    jobs = mcb.scenes(pkg, ctx, CELL_OCC, "even", k)
    cfg = {"oope_max": lambda: pkg.spe_cfg(oope=pkg.OOPE_MAX, area=(-0.1, 0.1, -0.1, 0.1)),
           "sum_sequential": lambda: pkg.spe_cfg(sum_order=pkg.SUM_SEQUENTIAL), "device_chain_off": None}[what]
    mb, lones = matchers(pkg, ctx, k, cfg=cfg)
    if what == "device_chain_off":
        for m in [mb] + lones:
            m.set_device_chain(0)
    try:
        for call in range(2):
            turn = [dict(j, init_pose=j["init_pose"] + np.array([0.01, 0.02, -0.01]) * call) for j in jobs]
            got = mb.process_scan_batch(turn, trace=True)
            check_batch(ctx, mb, lones, turn, got, chains=False, lone_kernels=None)
            for j in range(k):  # latched as if by the shared launches: at call 1's pose of the stream
                info = mb.bf_stream_info(j)
                assert info["base_set"] and info["matches"] == call + 1
                np.testing.assert_array_equal(info["base"], jobs[j]["init_pose"])
        assert not mb.bf_stream_info(-1)["base_set"]
    finally:
        close_all(mb, lones)


# ---- 9. launch count
@pytest.mark.parametrize("k", [2, 16])
def test_three_launches_whatever_k(pkg, ctx, raw_worlds, k):
    jobs = mcb.scenes(pkg, ctx, CELL_OCC, "even", k)
    mb, lones = matchers(pkg, ctx, k)
    try:
        got = mb.process_scan_batch(jobs, trace=True)
        assert mb.chain_stats()["kernels_launched"] == 3
        check_batch(ctx, mb, lones, jobs, got)
    finally:
        close_all(mb, lones)
    rb.upload(ctx, raw_worlds, CELL_TBM)
    three = rb.three_jobs(pkg, raw_worlds[CELL_TBM], "cached", "viny", 257)
    pool = three + [dict(three[1], init_pose=three[1]["init_pose"] + [0.05, 0.02, -0.01]),
                    dict(three[0], init_pose=three[0]["init_pose"] + [0.02, 0.0, 0.01])]
    raw = [pool[j % len(pool)] for j in range(k)]
    mb, lones = matchers(pkg, ctx, k, r9=R9_RAW)
    try:
        got = mb.process_raw_scan_batch(raw, trace=True)
        assert mb.chain_stats()["kernels_launched"] == 4
        for j, (g, job) in enumerate(zip(got, raw)):
            same_trace(g, rb.lone_raw(pkg, lones[j], job))
            assert mb.batch_stats(j)["on_device_chain"], j
            assert lones[j].stats()["kernels_launched"] == 4, j
    finally:
        close_all(mb, lones)


# ---- 10. one placed scene
def test_four_robots_in_four_quadrants(pkg, ctx):
    """K = 4 robots around 2 x 10^3 m, one per quadrant (tests/placed_scenes.py): poses whose ulp is 2^-42 m"""
    jobs = []
    for k, st in enumerate(ps.Q_STATIONS):
        sc = ps.place(st, seed=ps.SEEDS[st])
        ctx.upload_map(k, sc["map"])
        cos_a, sin_a = pkg.beam_trig(sc["scan"].angle)
        jobs.append(dict(map_id=k, range=sc["scan"].range, cos_a=cos_a, sin_a=sin_a, weight=sc["scan"].weight,
                         factor=sc["scan"].factor, init_pose=sc["init_pose"]))
        assert np.hypot(sc["init_pose"][0], sc["init_pose"][1]) > 2.0e3
    r9 = [-0.2, 0.2, 0.1, -0.2, 0.2, 0.1, -0.04, 0.04, 0.02]  # (0.1 m cells)
    mb, lones = matchers(pkg, ctx, 4, r9=r9)
    try:
        for call in range(2):
            turn = [dict(j, init_pose=j["init_pose"] + np.array([0.03, -0.02, 0.01]) * call) for j in jobs]
            got = mb.process_scan_batch(turn, trace=True)

            def lone_fn(c, m, job):
                c.scan_upload(job["range"], job["cos_a"], job["sin_a"], job["weight"], job["factor"])
                return m.process_scan(job["map_id"], job["init_pose"], trace=True)
            check_batch(ctx, mb, lones, turn, got, r9=r9, lone_fn=lone_fn)
    finally:
        close_all(mb, lones)
        for k in (2, 3):
            ctx.map_release(k)
