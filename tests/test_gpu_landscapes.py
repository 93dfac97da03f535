"""GPU suite (-m gpu): the decisions the matchers take from scores -- the first-maximum walk of the brute-force sweep's device
arg-max (csrc/bf_device.hip: k_bf_scan, k_bf_decide), the accept rules of the hill-climbing and Monte-Carlo chains in
their three forms (co-resident launch, kernel chain, host-driven batches) and the checked default mode's closeness test
-- on the DESIGNED score landscapes of tests/landscape_cases.py: a one-beam scan scores a pose with the value of the cell
under it, so the test author wrote the score sequence every walk meets.

References: tests/golden/landscapes.npz (the compiled reference's decisions, tests/golden/make_golden_landscapes.py) and
the CPU oracle, which tests/test_oracle_landscapes.py holds to that golden and to the author's expected decision, bit for
bit.  The reference refuses the tables with NaN (its obstacle OOPE asserts on a NaN impact); those are held to the oracle
alone.  EVERY comparison is exact -- assert_trace_equal(..., exact_scores=True), in the default mode too: a one-term sum is
the same in any order, the end point of a range-0 beam is the pose's own bits, and the one range-1 case keeps its end
points 0.02 m inside their cells.  No tolerance anywhere in this file.  (Two NaN compare equal here whatever their
payload bits: the device need not make the host's NaN.)"""
import numpy as np
import pyoracle as po
import pytest
from helpers import assert_trace_equal
from landscape_cases import assert_equals_row, case_map, cases_of, golden_rows, load_golden, oracle_matches

import __graft_entry__ as ge

pytestmark = pytest.mark.gpu

STRICT = dict(sum_order=1, pose_trig=1)  # SLAMHIP_SUM_SEQUENTIAL, SLAMHIP_POSE_TRIG_HOST
BF, HC, MC = cases_of("BF"), cases_of("HC"), cases_of("MC")


def ids(cases):
    return [c.name for c in cases]


@pytest.fixture(scope="module")
def pkg():
    return ge.load_package()


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def g():
    return load_golden()


@pytest.fixture(scope="module")
def refs(oracle):
    """the oracle's traces of a case's matches, computed once per case and left unchanged"""
    memo = {}

    def get(c):
        key = c.kind + ":" + c.name
        if key not in memo:
            memo[key] = oracle_matches(c, oracle, po)
            for t in memo[key]:
                for a in (t["poses"], t["scores"], t["accepted"], t["delta"]):
                    a.setflags(write=False)
        return memo[key]
    return get


def same_prob(a, b):
    return a == b or (np.isnan(a) and np.isnan(b))


def same_trace(t, want, row=None):
    """assert_trace_equal, exact; a NaN result equals a NaN result"""
    if np.isnan(t["prob"]) and np.isnan(want["prob"]):
        t, want = dict(t, prob=0.0), dict(want, prob=0.0)
    assert_trace_equal(t, want, exact_scores=True)
    if row is not None:
        assert_equals_row(t, row)


def same_result(q, want):
    assert same_prob(q["prob"], want["prob"]) and np.array_equal(q["delta"], want["delta"])


def upload(ctx, c, map_id=0):
    ctx.upload_map(map_id, case_map(c, po))
    ctx.scan_upload([c.rng], [1.0], [0.0], [1.0])


def job_of(c, map_id, init):
    return dict(map_id=map_id, range=[c.rng], cos_a=[1.0], sin_a=[0.0], weight=[1.0], factor=[1.0], init_pose=init)


def rows_of(g, c):
    rows = golden_rows(g, c)
    return rows if rows is not None else [None] * len(c.inits)


# ---- brute force -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", BF, ids=ids(BF))
def test_brute_force_decisions(pkg, ctx, g, refs, c):
    """strict and default mode, with and without an observer, and the host-driven twin: trace, prob, delta, n_calls and
    the scorer-call count against the golden (the oracle where the reference refused).  The matches of a case run in
    order on one matcher object per mode: the base pose is latched at the first."""
    upload(ctx, c)
    ms = dict(strict=pkg.Matcher(ctx, "BF", pkg.spe_cfg(**STRICT), c.params), default=pkg.Matcher(ctx, "BF", pkg.spe_cfg(), c.params),
              host=pkg.Matcher(ctx, "BF", pkg.spe_cfg(), c.params))
    ms["host"].set_device_chain(0)
    for init, want, row in zip(c.inits, refs(c), rows_of(g, c)):
        for mode, m in ms.items():
            same_trace(m.process_scan(0, init, trace=True), want, row)
            st = m.stats()
            assert st["scorer_calls"] == want["n_calls"] == 1 + c.shape[0] * c.shape[1] * c.shape[2]
            same_result(m.process_scan(0, init), want)  # no observer: nothing replayed on the host, the device's decision
            quiet = m.stats()
            assert quiet["scorer_calls"] == want["n_calls"]
            if mode == "default":
                if c.settles == "device":  # poses, sweep, scan, decide: the device settled every comparison itself
                    assert st["kernels_launched"] == quiet["kernels_launched"] == 4
                else:  # two sums one ulp apart, from different cells: the sweep may not decide -- it reports nothing, and
                    # the host-driven batches, which launch no chain kernel, settle the comparison from beam-order sums
                    print("LANDSCAPE BF %s: default mode left the device, kernels_launched %d" % (c.name, st["kernels_launched"]))
                    assert st["kernels_launched"] == quiet["kernels_launched"] == 0
            else:
                assert st["kernels_launched"] == 0
    for m in ms.values():
        m.close()


def test_three_brute_force_matches_in_one_batch(pkg, ctx, refs):
    """process_scan_batch over three tables of one shape (one matcher: one latched base pose): each its lone match"""
    cases = [c for c in BF if c.name in ("n1025-max_at_1024", "n1025-tie_1024_1025", "n1025-staircase")]
    assert len(cases) == 3
    for k, c in enumerate(cases):
        upload(ctx, c, k)
    for cfg in (pkg.spe_cfg(), pkg.spe_cfg(**STRICT)):
        mb = pkg.Matcher(ctx, "BF", cfg, cases[0].params)
        got = mb.process_scan_batch([job_of(c, k, c.inits[0]) for k, c in enumerate(cases)], trace=True)
        for k, c in enumerate(cases):
            lone = pkg.Matcher(ctx, "BF", cfg, c.params)
            ctx.scan_upload([c.rng], [1.0], [0.0], [1.0])
            same_trace(got[k], lone.process_scan(k, c.inits[0], trace=True))
            same_trace(got[k], refs(c)[0])
            lone.close()
        mb.close()
    for k in (1, 2):
        ctx.map_release(k)


# ---- hill climbing -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", HC, ids=ids(HC))
def test_hill_climbing_decisions(pkg, ctx, g, refs, c):
    """the strict host-driven trace against the golden / the oracle; the co-resident launch (2), the kernel chain (1)
    and the host-driven batches (0) of the default mode at 256 / 512 / 1024 threads: the same decisions, poses, scores
    and number of calls"""
    upload(ctx, c)
    init, want, row = c.inits[0], refs(c)[0], rows_of(g, c)[0]
    strict = pkg.Matcher(ctx, "HC", pkg.spe_cfg(**STRICT), c.params)
    strict.set_device_chain(0)
    same_trace(strict.process_scan(0, init, trace=True), want, row)
    strict.close()
    for mode in (2, 1, 0):
        for threads in (256, 512, 1024) if mode else (0,):
            m = pkg.Matcher(ctx, "HC", pkg.spe_cfg(), c.params)
            m.set_device_chain(mode, threads)
            same_trace(m.process_scan(0, init, trace=True), want, row)
            st = m.stats()
            assert st["scorer_calls"] == want["n_calls"]
            assert (st["kernels_launched"] > 0) == (mode > 0)
            if mode == 2:
                assert m.resident_stats() == dict(matches=1, gave_up=0) and st["kernels_launched"] == 1
            same_result(m.process_scan(0, init), want)
            m.close()


@pytest.mark.parametrize("level,mode", [(1, 2), (2, 2), (2, 1), (0, 2), (0, 1)])
def test_hill_climbing_inert_tails(pkg, ctx, refs, level, mode):
    """SLAMHIP_OPT_INERT_TAIL 0 / 1 / 2 on every table: the tail calls are reported whether they were scored or not --
    the plateaus are inert from the first round, the limit-60 tables end far behind the point where the steps vanish"""
    closed = 0
    for c in HC:
        upload(ctx, c)
        ctx.set_option(pkg.OPT_INERT_TAIL, level)
        try:
            m = pkg.Matcher(ctx, "HC", pkg.spe_cfg(), c.params)
            m.set_device_chain(mode)
            same_trace(m.process_scan(0, c.inits[0], trace=True), refs(c)[0])
            st = m.stats()
            assert st["scorer_calls"] == refs(c)[0]["n_calls"]
            assert level > 0 or st["calls_closed_form"] == 0
            closed += st["calls_closed_form"]
            if mode == 2:
                assert m.resident_stats() == dict(matches=1, gave_up=0)
            m.close()
        finally:
            ctx.set_option(pkg.OPT_INERT_TAIL, 2)
    print("LANDSCAPE HC inert tail level %d mode %d: %d calls in closed form" % (level, mode, closed))
    assert (closed > 0) == (level > 0)


@pytest.mark.parametrize("limit", [6, 60])
@pytest.mark.parametrize("mode", [2, 1])
def test_all_hill_climbing_tables_in_one_batch(pkg, ctx, refs, limit, mode):
    """process_scan_batch, K = the tables of one limit (a matcher has one limit), each on its own map with its own scan:
    every match its lone match"""
    cases = [c for c in HC if c.params[0] == limit]
    assert len(cases) == 8
    for k, c in enumerate(cases):
        upload(ctx, c, k)
    mb = pkg.Matcher(ctx, "HC", pkg.spe_cfg(), cases[0].params)
    mb.set_device_chain(mode)
    got = mb.process_scan_batch([job_of(c, k, c.inits[0]) for k, c in enumerate(cases)], trace=True)
    lone = pkg.Matcher(ctx, "HC", pkg.spe_cfg(), cases[0].params)
    for k, c in enumerate(cases):
        ctx.scan_upload([c.rng], [1.0], [0.0], [1.0])
        same_trace(got[k], lone.process_scan(k, c.inits[0], trace=True))
        same_trace(got[k], refs(c)[0])
        st = mb.batch_stats(k)
        assert st["on_device_chain"] and st["scorer_calls"] == refs(c)[0]["n_calls"]
    for m in (mb, lone):
        m.close()
    for k in range(1, 8):
        ctx.map_release(k)


# ---- Monte Carlo -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", MC, ids=ids(MC))
def test_monte_carlo_decisions(pkg, ctx, g, refs, c):
    """two matches in a row on one matcher (the engine is not reseeded): the strict trace against the golden / the
    oracle, the co-resident launch, the kernel chain and the host-driven batches of the default mode the same"""
    upload(ctx, c)
    ms = {"strict": pkg.Matcher(ctx, "MC", pkg.spe_cfg(**STRICT), c.params)}
    for mode in (2, 1, 0):
        ms[mode] = pkg.Matcher(ctx, "MC", pkg.spe_cfg(), c.params)
        ms[mode].set_device_chain(mode)
    for k, (init, want, row) in enumerate(zip(c.inits, refs(c), rows_of(g, c))):
        for mode, m in ms.items():
            same_trace(m.process_scan(0, init, trace=True), want, row)
            st = m.stats()
            assert st["scorer_calls"] == want["n_calls"]
            if mode == 2:
                assert m.resident_stats() == dict(matches=k + 1, gave_up=0) and st["kernels_launched"] == 1
            elif mode == 1:
                assert st["kernels_launched"] > 0
            else:
                assert st["kernels_launched"] == 0
    for m in ms.values():
        m.close()
