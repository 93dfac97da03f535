"""GPU suite: the lone co-resident hill-climbing chain that assembles the raw scan in its prologue (csrc/hc_resident.hip,
RAW) keeps the staged scan's loads in flight across the prologue: a thread's first beam and its first further one are
asked for together (scan_assemble_issue), waited for once in front of the barrier that ends the prologue
(scan_assemble_wait) and finished there (scan_assemble_finish); narrow workgroups take their further beams two at a
time in the same shape.  A wait that came too late, or not at all, would show as a beam constant that is not the staged
scan's -- so, as in test_gpu_raw_prologue.py, option 1 (the chain's own prologue) is held against option 0 (the
assembly kernel in front of the chain) with no tolerance anywhere: the scan block's five rows, the points kept, pose
delta, probability and scorer calls as bit patterns / integers, and no chain may have given up.

Shapes: the kept-beam counts at which the two issue blocks and the finish meet -- one beam more than the workgroup has
threads, the last lane of the first wave of further beams and its neighbours, one beam more than two per thread --,
with and without an index row, for every weighting, with and without a factor.  A sequence of alternating scans of
different lengths and ranges on ONE matcher.  The constants the super-step loop reads (failed-rounds limit, instance
counts, the inert tail, the tie check, the observer's trace) at the limits where they decide: against the chain of
kernels, traces included."""
import numpy as np
import pytest

from helpers import assert_trace_equal
from synth import make_scene
from test_gpu_raw_prologue import (A_MIN, HC, INC, N_RAW, both, ctx, keep_mask, matchers, one_match, pkg,  # noqa: F401
                                   scene)

pytestmark = pytest.mark.gpu


def meeting_points(nt):
    """kept beams around the places where the first issue, the second issue and the finish meet, capped at the scan"""
    return sorted({min(k, N_RAW) for k in (nt + 1, nt + 56, nt + 63, nt + 64, nt + 65, 2 * nt + 1)} | {1, 64})


@pytest.mark.parametrize("nt,k", [(nt, k) for nt in (256, 512, 1024) for k in meeting_points(nt)])
def test_kept_beams_where_the_issue_blocks_and_the_finish_meet(pkg, ctx, matchers, scene, nt, k):  # noqa: F811
    rs = np.random.RandomState(1000 * nt + k)
    for index_row in (False, True):
        for weighting in ("even", "viny", "ahr"):
            for with_factor in (False, True):
                if index_row:  # k picked out of 1080, at random places
                    n = N_RAW
                    occ, skip, max_range = keep_mask("pick", N_RAW, k, rs, scene["raw_range"])
                else:  # all of a k-beam scan
                    n, occ, skip, max_range = k, None, 0, -1.0
                fac = 0.5 + rs.rand(n) if with_factor else None
                pose = scene["init_pose"] + rs.randn(3) * [0.03, 0.03, 0.01]
                on = both(pkg, ctx, matchers, nt, scene, n, occ, skip, max_range, fac, "raw", weighting, pose)
                assert on["kept"] == k


@pytest.mark.parametrize("nt", [256, 1024])
def test_forty_alternating_scans_on_one_matcher(pkg, ctx, matchers, scene, nt):  # noqa: F811
    """two scans of different length and different ranges take turns: a constant that was read before its load had
    landed would be the OTHER scan's (the register's, or the staging buffer's, previous content)"""
    rs = np.random.RandomState(77)
    long_scene = scene
    short_scene = dict(scene, raw_range=np.minimum(scene["raw_range"][::-1] * 0.83 + 0.21, 25.0))
    plan = []
    for i in range(40):
        sc, n = (long_scene, N_RAW) if i % 2 == 0 else (short_scene, 321)
        plan.append((sc, n, scene["init_pose"] + rs.randn(3) * [0.04, 0.04, 0.015]))
    runs = {}
    for opt in (1, 0):
        before = ctx.get_option(pkg.OPT_RAW_PROLOGUE_MATCHES)
        runs[opt] = [one_match(pkg, ctx, matchers[nt, opt], opt, sc, n, None, 0, -1.0, None, "raw", "viny", pose)
                     for sc, n, pose in plan]
        assert ctx.get_option(pkg.OPT_RAW_PROLOGUE_MATCHES) - before == (40 if opt else 0)
        assert matchers[nt, opt].resident_stats()["gave_up"] == 0
    for i, (on, off) in enumerate(zip(runs[1], runs[0])):
        assert on["kept"] == off["kept"] == plan[i][1], i
        assert np.array_equal(on["scan"], off["scan"]), i
        assert on["prob"] == off["prob"] and np.array_equal(on["delta"], off["delta"]), i
        assert on["calls"] == off["calls"], i


@pytest.fixture(scope="module")
def scene90():
    return make_scene(cell_model=0, size=200, scale=0.1, n_beams=90, seed=17)


@pytest.mark.parametrize("tie_check", [0, 1])
@pytest.mark.parametrize("limit", [1, 2, 7, 128])
def test_loop_constants_at_the_limits_where_they_decide(pkg, scene90, limit, tie_check):  # noqa: F811
    """failed-rounds limits 1, 2, 7 and 128 on 90 beams, with and without an observer, tie check off and on: the
    co-resident launch against the chain of kernels -- result, scorer calls and the observer's trace, bit for bit"""
    sc = scene90
    c = pkg.Context(0)
    ms = []
    try:
        c.upload_map(0, sc["map"])
        cos_a, sin_a = pkg.beam_trig(sc["scan"].angle)
        c.scan_upload(sc["scan"].range, cos_a, sin_a, sc["scan"].weight, sc["scan"].factor)
        for threads in (1024, 256):
            res = pkg.Matcher(c, "HC", pkg.spe_cfg(), [limit, 0.1, 0.1])
            res.set_device_chain(2, threads)
            chain = pkg.Matcher(c, "HC", pkg.spe_cfg(), [limit, 0.1, 0.1])
            chain.set_device_chain(1, threads)
            ms += [res, chain]
            for m in (res, chain):
                m.set_tie_check(tie_check)
            init = sc["init_pose"]
            for rep in range(3):
                tr, tc = res.process_scan(0, init, trace=True), chain.process_scan(0, init, trace=True)
                assert_trace_equal(tr, tc)
                assert res.stats()["scorer_calls"] == chain.stats()["scorer_calls"] == tr["n_calls"]
                qr, qc = res.process_scan(0, init), chain.process_scan(0, init)  # no observer: no trace buffer
                assert qr["prob"] == qc["prob"] == tr["prob"] and np.array_equal(qr["delta"], qc["delta"])
                assert np.array_equal(qr["delta"], tr["delta"])
                assert res.stats()["scorer_calls"] == chain.stats()["scorer_calls"] == tr["n_calls"]
                init = init + np.array([0.021, -0.013, 0.006])
            assert res.resident_stats() == dict(matches=6, gave_up=0)
    finally:
        for m in ms:
            m.close()
        c.close()
