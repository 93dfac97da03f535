"""GPU suite: K Monte-Carlo matches per call, every job on its own engine stream (slamhip_matcher_set_mc_streams;
csrc/mc_chain.hip with grid.y = match and a job table) -- MonteCarloScanMatcher::process_scan once per robot, every robot
owning its matcher and with it its GaussianPoseEnumerator{mt19937(seed)} (init_scan_matching.h:118-135).

The bar throughout is assert_trace_equal, bit for bit (poses, scores, accept flags, delta, probability, call count):
job k of a batch against a LONE matcher created with seeds[k] and fed the same inputs in the same order, whose own path
is pinned to the reference's goldens elsewhere.  What may not matter: the batch size, the candidates per super-step, the
route a job took (shared launches / lone path on its stream), what the other jobs of the batch are."""
import ctypes as C
import types

import numpy as np
import pyoracle as po
import pytest
import test_gpu_raw_batch as rb
from helpers import assert_trace_equal
from landscape_cases import case_map, cases_of
from synth import CELL_OCC, CELL_TBM, cast_scan, make_scene, viny_weights

import __graft_entry__ as ge

pytestmark = pytest.mark.gpu

TD, RD = 0.2, 0.1  # common/monte_carlo_scan_matching.properties
PRESET = (20, 100)
LIMITS = [(1, 5), (3, 100), PRESET, (600, 1200)]
SIZES = (300, 260)


def seeds_of(k):
    return [1000 + 7919 * j for j in range(k)]


def prm(seed, lim):
    return [seed, TD, RD, lim[0], lim[1]]


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


def crop(m, x0, x1, y0, y1, cell_model=None):
    """an oblong, off-centre window of a map: what Context.upload_map takes"""
    return types.SimpleNamespace(cell_model=m.cell_model if cell_model is None else cell_model,
                                 payload=np.ascontiguousarray(m.payload[y0:y1, x0:x1]), width=x1 - x0, height=y1 - y0,
                                 origin=(int(m.origin[0]) - x0, int(m.origin[1]) - y0), scale=m.scale, unknown=m.unknown)


_worlds = {}


def worlds_of(cell, weighting):
    """two maps of different, oblong, off-centre windows (built once per cell model)"""
    key = (cell, weighting)
    if key not in _worlds:
        out = []
        for mi, size in enumerate(SIZES):
            sc = make_scene(cell_model=cell, size=size, scale=0.05, n_beams=360, seed=5 + mi, weighting=weighting)
            sc["window"] = crop(sc["map"], 10 + 20 * mi, size - 40, 30, size - 5 - 30 * mi)
            out.append(sc)
        _worlds[key] = out
    return _worlds[key]


_jobs = {}


def scenes(pkg, ctx, cell, weighting, k, beams=(360, 200, 513), bind_as=None):
    """k jobs over the two maps: scans cast from jittered robot poses with their own noise seeds, initial poses with
    errors from zero to three times the default"""
    worlds = worlds_of(cell, weighting)
    for mi, sc in enumerate(worlds):
        w = sc["window"]
        ctx.upload_map(mi, w if bind_as is None else types.SimpleNamespace(**dict(vars(w), cell_model=bind_as)))
    key = (cell, weighting, k, beams)
    if key not in _jobs:
        rs = np.random.RandomState(100 + k)
        jobs = []
        for j in range(k):
            sc = worlds[j % len(worlds)]
            true = sc["true_pose"] + rs.randn(3) * [0.15, 0.15, 0.05]
            rng, ang = cast_scan(sc["gt"], 0.05, true, beams[j % len(beams)], seed=42 + j)
            w = np.full(rng.size, 1.0 / rng.size) if weighting == "even" else viny_weights(rng, ang)
            cos_a, sin_a = pkg.beam_trig(ang)
            err = np.array([0.07, -0.04, 0.03]) * (3.0 * j / max(k - 1, 1))
            jobs.append(dict(map_id=j % len(worlds), range=rng, cos_a=cos_a, sin_a=sin_a, weight=w, factor=None,
                             init_pose=true + err, angle=ang))
        _jobs[key] = jobs
    return _jobs[key]


def lone(ctx, m, job, trace=True):
    ctx.scan_upload(job["range"], job["cos_a"], job["sin_a"], job["weight"], np.ones(np.size(job["range"])))
    return m.process_scan(job["map_id"], job["init_pose"], trace=trace)


def same_trace(g, w):
    """assert_trace_equal, with a probability that may be NaN on both sides"""
    if np.isnan(w["prob"]):
        assert np.isnan(g["prob"])
        g, w = dict(g, prob=0.0), dict(w, prob=0.0)
    assert_trace_equal(g, w)


def matchers(pkg, ctx, k, lim, cfg=None, streams=True):
    cfg = cfg or (lambda: pkg.spe_cfg())
    seeds = seeds_of(k)
    mb = pkg.Matcher(ctx, "MC", cfg(), prm(1, lim))
    if streams:
        mb.set_mc_streams(seeds)
    return mb, [pkg.Matcher(ctx, "MC", cfg(), prm(s, lim)) for s in seeds]


def close_all(*ms):
    for m in ms:
        for x in (m if isinstance(m, list) else [m]):
            x.close()


def check_batch(ctx, mb, lones, jobs, got, stream_of=None, chains=True):
    """every job against its lone matcher; counters; the engine streams against the lone engines"""
    calls = rescored = 0
    for j, (g, job) in enumerate(zip(got, jobs)):
        s = j if stream_of is None else stream_of[j]
        want = lone(ctx, lones[s], job)
        same_trace(g, want)
        st = mb.batch_stats(j)
        assert st["scorer_calls"] == want["n_calls"] == lones[s].stats()["scorer_calls"], j
        if chains is not None:
            assert st["on_device_chain"] == (chains if isinstance(chains, bool) else chains[j]), j
        assert mb.mc_stream_info(s) == lones[s].mc_stream_info(-1), j
        calls += st["scorer_calls"]
        rescored += lones[s].stats()["steps_rescored"]
    assert mb.stats()["scorer_calls"] == calls
    return rescored


# ---- 1. batch = lone, three consecutive calls (the engines carry over)
def run_three_calls(pkg, ctx, cell, weighting, k, lim, bind_as=None):
    jobs = scenes(pkg, ctx, cell, weighting, k, bind_as=bind_as)
    mb, lones = matchers(pkg, ctx, k, lim)
    try:
        for call in range(3):
            # (stream j meets another scan, map and initial error in every call)
            turn = [dict(jobs[(j + call) % k], init_pose=jobs[(j + call) % k]["init_pose"] + 0.01 * call) for j in range(k)]
            got = mb.process_scan_batch(turn, trace=True)
            assert len(got) == k
            check_batch(ctx, mb, lones, turn, got)
            assert mb.stats()["kernels_launched"] >= 2
            assert [mb.mc_stream_info(j)["matches"] for j in range(k)] == [call + 1] * k
        # without an observer: the results of the lone matchers' next match
        got = mb.process_scan_batch(jobs)
        for j, g in enumerate(got):
            w = lone(ctx, lones[j], jobs[j], trace=False)
            assert g["prob"] == w["prob"] or (np.isnan(g["prob"]) and np.isnan(w["prob"]))
            assert np.array_equal(g["delta"], w["delta"])
            assert mb.mc_stream_info(j) == lones[j].mc_stream_info(-1)
    finally:
        close_all(mb, lones)


@pytest.mark.parametrize("lim", LIMITS, ids=lambda v: "%dx%d" % v)
@pytest.mark.parametrize("k", [2, 3, 8, 20])
@pytest.mark.parametrize("cell,weighting", [(CELL_OCC, "even"), (CELL_TBM, "viny")])
def test_batch_equals_lone_matchers_over_three_calls(pkg, ctx, cell, weighting, k, lim):
    run_three_calls(pkg, ctx, cell, weighting, k, lim)


def test_batch_equals_lone_matchers_on_credibilist_maps(pkg, ctx):
    run_three_calls(pkg, ctx, CELL_TBM, "viny", 3, PRESET, bind_as=pkg.CELL_CREDIBILIST)


# ---- 2. beam counts at the kernel's edges, in one batch
def test_beam_counts_at_the_kernels_edges_in_one_batch(pkg, ctx):
    scenes(pkg, ctx, CELL_OCC, "even", 2)  # (the maps)
    counts = [1, 63, 64, 65, 257, 513, 2049, 4096]
    sc = worlds_of(CELL_OCC, "even")[0]
    rng0, ang0 = cast_scan(sc["gt"], 0.05, sc["true_pose"], 4097, seed=9)
    assert rng0.size >= 4097 - 64  # (beams that hit nothing are dropped by the caster)

    def job_of(n, j):
        idx = np.resize(np.arange(rng0.size), n) if n > rng0.size else np.linspace(0, rng0.size - 1, n).astype(int)
        rng, ang = rng0[idx], ang0[idx]
        cos_a, sin_a = pkg.beam_trig(ang)
        return dict(map_id=0, range=rng, cos_a=cos_a, sin_a=sin_a, weight=np.full(n, 1.0 / n), factor=None,
                    init_pose=sc["true_pose"] + np.array([0.05, -0.03, 0.02]) * (1 + j % 3))

    jobs = [job_of(n, j) for j, n in enumerate(counts)]
    assert [j["range"].size for j in jobs] == counts
    mb, lones = matchers(pkg, ctx, len(counts) + 1, PRESET)
    try:
        got = mb.process_scan_batch(jobs, trace=True)
        check_batch(ctx, mb, lones, jobs, got)
        # 4097 points: more than the chain's workgroups take -- the call goes through the lone route, job by job, each
        # job on ITS stream
        jobs2 = jobs[:3] + [job_of(4097, 1)] + jobs[3:5]
        sid = [0, 1, 2, 8, 3, 4]
        mb.set_mc_job_streams(sid)
        got = mb.process_scan_batch(jobs2, trace=True)
        check_batch(ctx, mb, lones, jobs2, got, stream_of=sid, chains=False)
    finally:
        close_all(mb, lones)


# ---- 3. the speculation width must not matter
def test_candidates_per_super_step_do_not_matter(pkg, tctx):
    ctx = tctx
    L = pkg.load(testing=True)
    L.slamhip_matcher_testing_mc_batch_slots.argtypes = [C.c_void_p, C.c_int]
    k = 5
    jobs = scenes(pkg, ctx, CELL_OCC, "even", k)
    for lim in (PRESET, (600, 1200)):
        md, lones = matchers(pkg, ctx, k, lim)
        default = [md.process_scan_batch(jobs, trace=True) for _ in range(2)]
        steps = [md.batch_stats(j)["super_steps"] for j in range(k)]
        forced_steps = {}
        try:
            for s in (1, 7, 64):
                mb = pkg.Matcher(ctx, "MC", pkg.spe_cfg(), prm(1, lim))
                mb.set_mc_streams(seeds_of(k))
                assert L.slamhip_matcher_testing_mc_batch_slots(mb.h, s) == 0
                for call in range(2):
                    got = mb.process_scan_batch(jobs, trace=True)
                    for j, (g, d) in enumerate(zip(got, default[call])):
                        same_trace(g, d)
                forced_steps[s] = [mb.batch_stats(j)["super_steps"] for j in range(k)]
                assert [mb.mc_stream_info(j) for j in range(k)] == [md.mc_stream_info(j) for j in range(k)]
                mb.close()
            # (the knob is real: one candidate per super-step takes more super-steps than the rule's width)
            assert sum(forced_steps[1]) > sum(steps)
        finally:
            close_all(md, lones)


# ---- 4. chains of very different length in one batch
def test_chains_of_very_different_length(pkg, ctx):
    jobs = [dict(j) for j in scenes(pkg, ctx, CELL_OCC, "even", 6)]
    w = worlds_of(CELL_OCC, "even")[0]["window"]
    blank = types.SimpleNamespace(**dict(vars(w), payload=np.full_like(w.payload, w.unknown[0])))
    ctx.upload_map(2, blank)
    # (job 0 of scenes() has zero initial error)
    jobs[1]["map_id"] = 2  # all unknown: no candidate beats the initial pose
    jobs[2]["init_pose"] = jobs[2]["init_pose"] + 2.0 * np.array([0.07, -0.04, 0.03])
    mb, lones = matchers(pkg, ctx, 6, PRESET)
    try:
        for _ in range(2):
            got = mb.process_scan_batch(jobs, trace=True)
            rescored = check_batch(ctx, mb, lones, jobs, got)
            assert mb.chain_stats()["steps_rescored"] == rescored
        # (the initial pose is the first call and the first "update"; none of the 20 candidates after it is accepted)
        assert got[1]["accepted"][1:].sum() == 0 and got[1]["n_calls"] == PRESET[0] + 1 and not got[1]["delta"].any()
        steps = [mb.batch_stats(j)["super_steps"] for j in range(6)]
        assert min(steps) < max(steps)
    finally:
        close_all(mb, lones)


def test_one_beam_landscapes_as_jobs_of_one_batch(pkg, ctx):
    """the designed one-beam Monte-Carlo tables of tests/landscape_cases.py -- ties, plateaus where the checked mode scores
    a super-step a second time, NaN rings -- two matches per table, all in one batch, twice"""
    cases = cases_of("MC")
    jobs = []
    for mi, c in enumerate(cases):
        ctx.upload_map(mi, case_map(c, po))
        for init in c.inits:
            jobs.append(dict(map_id=mi, range=np.array([c.rng]), cos_a=np.array([1.0]), sin_a=np.array([0.0]),
                             weight=np.array([1.0]), factor=None, init_pose=np.asarray(init, dtype=np.float64)))
    k = len(jobs)
    assert k == 8 and cases[0].params[3:] == list(PRESET)
    mb = pkg.Matcher(ctx, "MC", pkg.spe_cfg(), cases[0].params)
    seeds = seeds_of(k)
    mb.set_mc_streams(seeds)
    lones = [pkg.Matcher(ctx, "MC", pkg.spe_cfg(), [s] + cases[0].params[1:]) for s in seeds]
    try:
        total = 0
        for _ in range(2):
            got = mb.process_scan_batch(jobs, trace=True)
            rescored = check_batch(ctx, mb, lones, jobs, got)
            assert mb.chain_stats()["steps_rescored"] == rescored
            total += rescored
        assert total > 0  # (the plateau re-scores)
    finally:
        close_all(mb, lones)


# ---- 5. stream mapping
def test_stream_mapping(pkg, ctx):
    k = 4
    jobs = scenes(pkg, ctx, CELL_OCC, "even", k)
    mb, lones = matchers(pkg, ctx, k, PRESET)
    hc = pkg.Matcher(ctx, "HC", pkg.spe_cfg(), [6, 0.1, 0.1])
    try:
        perm = [2, 0, 3, 1]
        mb.set_mc_job_streams(perm)
        got = mb.process_scan_batch(jobs, trace=True)
        check_batch(ctx, mb, lones, jobs, got, stream_of=perm)
        mb.set_mc_job_streams(None)
        before = [mb.mc_stream_info(j) for j in range(k)]
        stats = (mb.stats(), [mb.batch_stats(j) for j in range(k)])
        # refused before anything is launched: the mapping stays the identity, no stream moves
        for bad, text in (([0, 1, 1, 2], "same engine stream"), ([0, 1, 2, 4], "out of range"), ([0, -1], "out of range"),
                          ([0, 1, 2, 3, 0], "more jobs than")):
            with pytest.raises(pkg.SlamHipError, match=text):
                mb.set_mc_job_streams(bad)
        with pytest.raises(pkg.SlamHipError, match="more jobs than"):
            mb.process_scan_batch(jobs + jobs[:1])
        mb.set_mc_job_streams([3, 2])
        with pytest.raises(pkg.SlamHipError, match="more jobs than"):  # (than the mapping names)
            mb.process_scan_batch(jobs[:3])
        with pytest.raises(pkg.SlamHipError, match="unknown map id"):
            mb.process_scan_batch([jobs[0], dict(jobs[1], map_id=17)])
        mb.set_mc_job_streams(None)
        for fn in (lambda: hc.set_mc_streams([1, 2]), lambda: hc.set_mc_job_streams([0]), lambda: hc.mc_stream_info(-1)):
            with pytest.raises(pkg.SlamHipError, match="Monte-Carlo"):
                fn()
        assert [mb.mc_stream_info(j) for j in range(k)] == before
        assert (mb.stats(), [mb.batch_stats(j) for j in range(k)]) == stats
        got = mb.process_scan_batch(jobs, trace=True)  # the next valid call: the lone sequence goes on
        check_batch(ctx, mb, lones, jobs, got)
        # streams set but one job: the lone chain, on that job's stream
        mb.set_mc_job_streams([2])
        own = mb.mc_stream_info(-1)
        got = mb.process_scan_batch(jobs[1:2], trace=True)
        check_batch(ctx, mb, lones, jobs[1:2], got, stream_of=[2], chains=False)
        assert mb.mc_stream_info(-1) == own  # (the matcher's own engine took no part)
        # reset_state: the enumerators start over, the engines stay where they are
        mb.set_mc_job_streams(None)
        mb.reset_state()
        for m in lones:
            m.reset_state()
        got = mb.process_scan_batch(jobs, trace=True)
        check_batch(ctx, mb, lones, jobs, got)
        # lone calls on a matcher with streams use the matcher's own engine
        ml = pkg.Matcher(ctx, "MC", pkg.spe_cfg(), prm(1, PRESET))
        same_trace(lone(ctx, mb, jobs[0]), lone(ctx, ml, jobs[0]))
        assert mb.mc_stream_info(-1) == ml.mc_stream_info(-1)
        ml.close()
        # the streams removed: the single engine again
        mb.set_mc_streams([])
        mb.process_scan_batch(jobs[:2])
        assert not mb.batch_stats(0)["on_device_chain"]
    finally:
        close_all(mb, lones, hc)


# ---- 6. the raw batch
@pytest.fixture(scope="module")
def raw_worlds():
    out = {}
    for cell in (CELL_OCC, CELL_TBM):
        ws = []
        for mi, size in enumerate(rb.SIZES):
            sc = make_scene(cell_model=cell, size=size, scale=0.1, n_beams=rb.N_A, seed=20 + mi)
            sc["raw"] = {}
            for n in (rb.N_A, rb.N_B):
                rng, _, occ = cast_scan(sc["gt"], 0.1, sc["true_pose"], n, seed=7 + mi, raw=True)
                sc["raw"][n] = (rng, occ)
            ws.append(sc)
        out[cell] = ws
    return out


@pytest.mark.parametrize("cell,weighting,trig", [(CELL_OCC, "even", "raw"), (CELL_TBM, "viny", "cached"), (CELL_OCC, "ahr", "cached"),
                                                 (CELL_TBM, "even", "cached"), (CELL_OCC, "viny", "raw"), (CELL_TBM, "ahr", "raw")])
def test_raw_batch_equals_lone_raw_calls(pkg, ctx, raw_worlds, cell, weighting, trig):
    rb.upload(ctx, raw_worlds, cell)
    ws = raw_worlds[cell]
    three = rb.three_jobs(pkg, ws, trig, weighting, 257)
    empty = rb.raw_job(pkg, ws[1], 1, rb.N_B, trig, weighting, is_occ=np.zeros(rb.N_B, np.int32))
    jobs = [three[0], three[1], empty, three[2], dict(three[1], init_pose=three[1]["init_pose"] + [0.05, 0.02, -0.01])]
    k = len(jobs)
    mb, lones = matchers(pkg, ctx, k, PRESET)
    try:
        for call in range(2):
            got = mb.process_raw_scan_batch(jobs, trace=True)
            for j, (g, job) in enumerate(zip(got, jobs)):
                want = rb.lone_raw(pkg, lones[j], job)
                assert g["kept"] == want["kept"], j
                st = mb.batch_stats(j)
                if j == 2:  # nothing kept: NaN, zero delta, no observer call, the stream not advanced
                    assert want["kept"] == 0 and np.isnan(g["prob"]) and not g["delta"].any() and g["n_calls"] == 0
                    assert st == dict(scorer_calls=0, poses_evaluated=0, super_steps=0, on_device_chain=False)
                    assert mb.mc_stream_info(2) == dict(pairs_consumed=0, matches=0, failed=0, poses=0, td=TD, rd=RD,
                                                        has_saved=False)
                else:
                    same_trace(g, want)
                    assert st["on_device_chain"] and st["scorer_calls"] == want["n_calls"]
                    np.testing.assert_array_equal(rb.bits(mb.batch_scan_download(j)), rb.download(ctx),
                                                  err_msg="scan block of job %d" % j)
                assert mb.mc_stream_info(j) == lones[j].mc_stream_info(-1), j
        # one non-empty job: the lone raw call on that job's stream
        mb.set_mc_job_streams([3, 1])
        got = mb.process_raw_scan_batch([empty, jobs[1]], trace=True)
        same_trace(got[1], rb.lone_raw(pkg, lones[1], jobs[1]))
        assert not mb.batch_stats(1)["on_device_chain"] and got[0]["kept"] == 0
        assert mb.mc_stream_info(1) == lones[1].mc_stream_info(-1) and mb.mc_stream_info(3) == lones[3].mc_stream_info(-1)
    finally:
        close_all(mb, lones)


# ---- 7. fall-backs keep the stream semantics
def test_fallbacks_run_on_the_jobs_own_streams(pkg, tctx):
    ctx = tctx
    k = 4
    jobs = scenes(pkg, ctx, CELL_OCC, "even", k)
    strict = lambda: pkg.spe_cfg(sum_order=pkg.SUM_SEQUENTIAL, pose_trig=pkg.POSE_TRIG_HOST)  # noqa: E731
    mb, lones = matchers(pkg, ctx, k, PRESET, cfg=strict)
    try:
        for _ in range(2):
            got = mb.process_scan_batch(jobs, trace=True)
            check_batch(ctx, mb, lones, jobs, got, chains=False)
    finally:
        close_all(mb, lones)
    # the beam-order sum alone (device trigonometry): off the shared launches too, by the rule kept here
    seq = lambda: pkg.spe_cfg(sum_order=pkg.SUM_SEQUENTIAL)  # noqa: E731
    mb, lones = matchers(pkg, ctx, k, PRESET, cfg=seq)
    try:
        got = mb.process_scan_batch(jobs, trace=True)
        check_batch(ctx, mb, lones, jobs, got, chains=False)
    finally:
        close_all(mb, lones)
    # a trace buffer made too small (testing hook): the jobs whose trace outgrew it go the lone route
    mb, lones = matchers(pkg, ctx, k, PRESET)
    probe = matchers(pkg, ctx, k, PRESET)[0]
    L = pkg.load(testing=True)
    L.slamhip_matcher_debug_trace_cap.argtypes = [C.c_void_p, C.c_int]
    try:
        calls = [g["n_calls"] for g in probe.process_scan_batch(jobs, trace=True)]
        cap = sorted(calls)[1]  # the two shortest traces fit
        assert L.slamhip_matcher_debug_trace_cap(mb.h, cap) == 0
        got = mb.process_scan_batch(jobs, trace=True)
        on = [c <= cap for c in calls]
        assert 1 <= sum(on) < k, calls
        check_batch(ctx, mb, lones, jobs, got, chains=on)
        assert L.slamhip_matcher_debug_trace_cap(mb.h, 0) == 0
        got = mb.process_scan_batch(jobs, trace=True)
        check_batch(ctx, mb, lones, jobs, got)
    finally:
        close_all(mb, lones, probe)


# ---- 8. no streams = today
def test_without_streams_the_single_engine_sequence(pkg, ctx, raw_worlds):
    jobs = scenes(pkg, ctx, CELL_OCC, "even", 3)
    mb, ml = pkg.Matcher(ctx, "MC", pkg.spe_cfg(), prm(5, PRESET)), pkg.Matcher(ctx, "MC", pkg.spe_cfg(), prm(5, PRESET))
    try:
        got = mb.process_scan_batch(jobs, trace=True)
        for j, (g, job) in enumerate(zip(got, jobs)):  # ONE lone matcher: its engine runs on from match to match
            same_trace(g, lone(ctx, ml, job))
            assert not mb.batch_stats(j)["on_device_chain"]
        assert mb.mc_stream_info(-1) == ml.mc_stream_info(-1) and mb.mc_stream_info(-1)["matches"] == 3
        rb.upload(ctx, raw_worlds, CELL_OCC)
        raw = rb.three_jobs(pkg, raw_worlds[CELL_OCC], "raw", "even", 256)
        got = mb.process_raw_scan_batch(raw, trace=True)
        for j, (g, job) in enumerate(zip(got, raw)):
            same_trace(g, rb.lone_raw(pkg, ml, job))
            assert not mb.batch_stats(j)["on_device_chain"]
        assert mb.mc_stream_info(-1) == ml.mc_stream_info(-1)
    finally:
        close_all(mb, ml)


# ---- 9. launch count
def test_shared_launches_are_fewer_than_the_chains_super_steps(pkg, ctx):
    """K = 8 at the preset, all jobs with the same initial error: every job takes at least two super-steps and typically
    five or more, the driver runs at most a few kernels ahead -- one kernel serves a super-step of EVERY chain"""
    k = 8
    jobs = [dict(j, init_pose=j["init_pose"]) for j in scenes(pkg, ctx, CELL_OCC, "even", k)]
    err = np.array([0.07, -0.04, 0.03])
    base = scenes(pkg, ctx, CELL_OCC, "even", k)
    for j, job in enumerate(jobs):  # (scenes() scales the error with the job: put the default one everywhere)
        job["init_pose"] = base[j]["init_pose"] - err * (3.0 * j / (k - 1)) + err
    mb, lones = matchers(pkg, ctx, k, PRESET)
    try:
        for _ in range(3):
            mb.process_scan_batch(jobs)
            steps = [mb.batch_stats(j)["super_steps"] for j in range(k)]
            assert all(mb.batch_stats(j)["on_device_chain"] for j in range(k))
            print("kernels launched %d, super-steps %r" % (mb.chain_stats()["kernels_launched"], steps))
            assert mb.chain_stats()["kernels_launched"] < sum(steps)
    finally:
        close_all(mb, lones)
