"""GPU suite: slamhip_matcher_process_raw_scan_batch -- K raw scans in, K matches in the shared launches, the scans
assembled by ONE launch of k_scan_assemble_table (csrc/score_kernels.hip) from the call's pinned arena and the
scanners' resident tables.  No tolerance anywhere: every job must be, bit for bit, (i) a lone
slamhip_matcher_process_raw_scan on a fresh matcher and (ii) slamhip_matcher_process_scan_batch fed with the public host
filter's outputs -- pose delta, probability, points kept, scorer calls, observer trace, and the scan block in HBM.

Small scenes (maps of 90 .. 120 cells a side, raw scans of 300 / 600 beams): kept counts of 1 and on both sides of the
workgroup sizes (255 / 256 / 257, 511 / 513), a bounded map whose rim drops beams, skip_rate, a usable range, is_occ,
factors, two scanners among three jobs; even / viny / ahr weights x raw / cached beam trig x OCC / TBM maps."""
import ctypes as C

import numpy as np
import pytest
from helpers import assert_trace_equal
from synth import CELL_OCC, CELL_TBM, cast_scan, make_scene

import __graft_entry__ as ge

pytestmark = pytest.mark.gpu

_dp = C.POINTER(C.c_double)
HC = [24, 0.1, 0.1]
SIZES = (120, 100, 90)
N_A, N_B = 600, 300  # raw beams of the two scanners
A_MIN = -np.deg2rad(135.0)
WEIGHTINGS = ("even", "viny", "ahr")
K1 = (255, 256, 257, 511, 513)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def pkg():
    return ge.load_package()


def scanner(n):
    """angles as the cached provider's accumulating loop makes them (every table index exact), and its settings"""
    inc = np.deg2rad(270.0) / n
    acc, a = [], A_MIN
    while len(acc) < n:
        acc.append(a)
        a += inc
    return dict(angle=np.array(acc), a_min=A_MIN, a_max=A_MIN + inc * n + inc, a_inc=inc)


@pytest.fixture(scope="module")
def worlds():
    """per cell model three maps with different windows, and per map raw scans of both scanners cast from it"""
    out = {}
    for cell in (CELL_OCC, CELL_TBM):
        ws = []
        for mi, size in enumerate(SIZES):
            sc = make_scene(cell_model=cell, size=size, scale=0.1, n_beams=N_A, seed=20 + mi)
            sc["raw"] = {}
            for n in (N_A, N_B):
                rng, _, occ = cast_scan(sc["gt"], 0.1, sc["true_pose"], n, seed=7 + mi, raw=True)
                sc["raw"][n] = (rng, occ)
            ws.append(sc)
        out[cell] = ws
    return out


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def upload(ctx, worlds, cell):
    for mi, sc in enumerate(worlds[cell]):
        ctx.upload_map(mi, sc["map"])


def raw_job(pkg, sc, map_id, n, trig, weighting, is_occ=None, factor=None, skip_rate=0, max_range=-1.0, bounded=False,
            pose=None, rng=None):
    s = scanner(n)
    return dict(map_id=map_id, range=sc["raw"][n][0] if rng is None else rng, angle=s["angle"], is_occ=is_occ, factor=factor,
                trig_mode=pkg.TRIG_CACHED if trig == "cached" else pkg.TRIG_RAW, a_min=s["a_min"], a_max=s["a_max"],
                a_inc=s["a_inc"], skip_rate=skip_rate, max_range=max_range, bounded=bounded, weighting=weighting,
                init_pose=sc["init_pose"] if pose is None else pose, world=sc)


def three_jobs(pkg, ws, trig, weighting, k1, seed=0):
    """job 0: the smallest map, bounded, beams over its rim (the pose is 0.7 m off: the wall's far side leaves the
    window), every third beam, a usable range that drops points; job 1: is_occ partly 0 -- exactly k1 of 600 beams --,
    factors; job 2: the other scanner, one beam kept"""
    rs = np.random.RandomState(1000 + k1 + seed)
    occ1 = np.zeros(N_A, np.int32)
    occ1[rs.choice(N_A, k1, replace=False)] = 1
    occ2 = np.zeros(N_B, np.int32)
    occ2[rs.randint(N_B)] = 1
    off = ws[2]["init_pose"] + np.array([0.7, 0.0, 0.0])  # (the beams that end on the wall at x = 4 m leave the 4.5 m window)
    return [raw_job(pkg, ws[2], 2, N_A, trig, weighting, skip_rate=3, max_range=4.4, bounded=True, pose=off),
            raw_job(pkg, ws[0], 0, N_A, trig, weighting, is_occ=occ1, factor=0.5 + rs.rand(N_A)),
            raw_job(pkg, ws[1], 1, N_B, trig, weighting, is_occ=occ2)]


def lone_raw(pkg, m, job, trace=True):
    """slamhip_matcher_process_raw_scan with an observer: dict(kept, prob, delta[, trace])"""
    blk = m.make_raw_batch([job])
    scan = blk["raw_arr"][0].scan
    rec = dict(poses=[], scores=[], accepted=[])

    def on_test(_u, p, s):
        rec["poses"].append((p[0], p[1], p[2]))
        rec["scores"].append(s)
        rec["accepted"].append(0)

    def on_update(_u, p, s):
        rec["accepted"][-1] = 1

    if trace:
        m._obs = pkg.Observer(None, pkg.OBS_FN(on_test), pkg.OBS_FN(on_update), pkg.OBS_FN(0))
        assert m.L.slamhip_matcher_set_observer(m.h, C.byref(m._obs)) == 0
        m._obs_cleared = False
    else:
        assert m.L.slamhip_matcher_set_observer(m.h, None) == 0
        m._obs_cleared = True
    fn = m.L.slamhip_matcher_process_raw_scan
    fn.argtypes = [C.c_void_p, C.c_int, C.POINTER(pkg.RawScan), _dp, _dp, _dp, C.POINTER(C.c_int)]
    pose3, d3, prob, kept = (C.c_double * 3)(*[float(v) for v in job["init_pose"]]), (C.c_double * 3)(), C.c_double(), C.c_int(-1)
    rc = fn(m.h, job["map_id"], C.byref(scan), pose3, d3, C.byref(prob), C.byref(kept))
    assert rc == 0
    out = dict(kept=kept.value, prob=prob.value, delta=np.array(list(d3)))
    if trace:
        out.update(poses=np.array(rec["poses"]).reshape(-1, 3), scores=np.array(rec["scores"]),
                   accepted=np.array(rec["accepted"], dtype=np.int32), n_calls=len(rec["scores"]))
    return out


def download(ctx):
    fn = ctx.L.slamhip_scan_download
    fn.argtypes = [C.c_void_p, C.c_int, _dp, C.POINTER(C.c_int)]
    n = C.c_int(-1)
    assert fn(ctx.h, 0, None, C.byref(n)) == 0
    out = np.full((5, max(n.value, 1)), np.nan)
    assert fn(ctx.h, out.shape[1], out.ctypes.data_as(_dp), C.byref(n)) == 0
    return out[:, :n.value].view(np.uint64)


def table_uploads(ctx):
    n = C.c_longlong(-1)
    ctx.L.slamhip_scan_table_uploads.argtypes = [C.c_void_p, C.POINTER(C.c_longlong)]
    assert ctx.L.slamhip_scan_table_uploads(ctx.h, C.byref(n)) == 0
    return n.value


def filtered(pkg, job):
    """the job as slamhip_matcher_process_scan_batch takes it: the public host filter, weights and beam trig"""
    m, rng, ang = job["world"]["map"], job["range"], job["angle"]
    tab = {}
    if job["trig_mode"] == pkg.TRIG_CACHED:
        # (the provider's table: sincos of the angles its accumulating loop makes)
        acc, a = [], job["a_min"]
        while a < job["a_max"]:
            acc.append(a)
            a += job["a_inc"]
        tc, ts = pkg.beam_trig(np.array(acc))
        tab = dict(a_min=job["a_min"], a_delta=job["a_inc"], tab_sin=ts, tab_cos=tc)
    geom = dict(width=m.width, height=m.height, origin=m.origin, scale=m.scale, bounded=job["bounded"])
    kept = pkg.filter_scan(rng, ang, job["is_occ"], job["init_pose"], geom, skip_rate=job["skip_rate"],
                           max_range=job["max_range"], trig_mode=job["trig_mode"], **tab)
    cos_a, sin_a = pkg.beam_trig(ang, job["trig_mode"], job["a_min"], job["a_max"], job["a_inc"])
    w = pkg.scan_weights(job["weighting"], rng[kept], ang[kept]) if kept.size else np.zeros(0)
    return dict(map_id=job["map_id"], range=rng[kept], cos_a=cos_a[kept], sin_a=sin_a[kept], weight=w,
                factor=job["factor"][kept] if job["factor"] is not None else None, init_pose=job["init_pose"]), kept


def check_against_lone(pkg, ctx, mb, jobs, got, cfg=None, kind="HC", prm=HC, chains=True, scans=True):
    """every job of `got` against a lone raw call on a fresh matcher"""
    for c, (g, job) in enumerate(zip(got, jobs)):
        ml = pkg.Matcher(ctx, kind, cfg or pkg.spe_cfg(), prm)
        try:
            want = lone_raw(pkg, ml, job)
            assert g["kept"] == want["kept"], c
            if want["kept"] == 0:
                assert np.isnan(g["prob"]) and np.isnan(want["prob"]) and not g["delta"].any() and g["n_calls"] == 0
                assert mb.batch_stats(c) == dict(scorer_calls=0, poses_evaluated=0, super_steps=0, on_device_chain=False)
                continue
            assert_trace_equal(g, want)
            assert want["n_calls"] > 20  # (a match, not a formality)
            st = mb.batch_stats(c)
            assert st["scorer_calls"] == want["n_calls"] == ml.stats()["scorer_calls"], c
            assert st["on_device_chain"] == chains, c
            if scans and chains:
                np.testing.assert_array_equal(bits(mb.batch_scan_download(c)), download(ctx), err_msg="scan block of job %d" % c)
        finally:
            ml.close()


CASES = [(cell, w, trig) for cell in (CELL_OCC, CELL_TBM) for w in WEIGHTINGS for trig in ("raw", "cached")]


@pytest.mark.parametrize("cell,weighting,trig", CASES)
def test_equal_to_lone_calls_and_to_the_filtered_route(pkg, ctx, worlds, cell, weighting, trig):
    upload(ctx, worlds, cell)
    case = CASES.index((cell, weighting, trig))
    for k1 in (K1[case % 5], K1[(case + 2) % 5]):
        jobs = three_jobs(pkg, worlds[cell], trig, weighting, k1)
        mb = pkg.Matcher(ctx, "HC", pkg.spe_cfg(), HC)
        mf = pkg.Matcher(ctx, "HC", pkg.spe_cfg(), HC)
        try:
            got = mb.process_raw_scan_batch(jobs, trace=True)
            assert [g["kept"] for g in got][1:] == [k1, 1] and 1 < got[0]["kept"] < N_A // 3
            assert mb.stats()["kernels_launched"] >= 1
            check_against_lone(pkg, ctx, mb, jobs, got)  # (i)
            # (ii) the filtered route: the host filter's outputs through slamhip_matcher_process_scan_batch
            fj = [filtered(pkg, j) for j in jobs]
            for g, (f, kept) in zip(got, fj):
                assert g["kept"] == kept.size
            want = mf.process_scan_batch([f for f, _ in fj], trace=True)
            for c, (g, w) in enumerate(zip(got, want)):
                assert_trace_equal(g, w)
                assert mb.batch_stats(c) == mf.batch_stats(c)
            # the scan blocks are what the host route uploads: five rows per job
            for c, (f, _) in enumerate(fj):
                blk = mb.batch_scan_download(c)
                fac = f["factor"] if f["factor"] is not None else np.ones(f["range"].size)
                for row, name in enumerate(("range", "cos_a", "sin_a", "weight")):
                    np.testing.assert_array_equal(bits(blk[row]), bits(f[name]), err_msg="%s of job %d" % (name, c))
                np.testing.assert_array_equal(bits(blk[4]), bits(fac))
            # without an observer, the argument block made once: the same bits, call after call
            blk = mb.make_raw_batch(jobs)
            for _ in range(2):
                for g, a in zip(got, mb.process_raw_scan_batch(blk)):
                    assert bits(g["prob"]) == bits(a["prob"]) and np.array_equal(bits(g["delta"]), bits(a["delta"]))
                    assert g["kept"] == a["kept"]
        finally:
            mb.close()
            mf.close()


def test_empty_jobs_and_batches_of_none_and_one(pkg, ctx, worlds):
    upload(ctx, worlds, CELL_OCC)
    ws = worlds[CELL_OCC]
    jobs = three_jobs(pkg, ws, "raw", "viny", 257)
    empty = raw_job(pkg, ws[1], 1, N_B, "raw", "viny", is_occ=np.zeros(N_B, np.int32))
    mb = pkg.Matcher(ctx, "HC", pkg.spe_cfg(), HC)
    try:
        ref = mb.process_raw_scan_batch(jobs, trace=True)
        got = mb.process_raw_scan_batch([jobs[0], empty, jobs[1]], trace=True)
        assert got[1]["kept"] == 0 and np.isnan(got[1]["prob"]) and not got[1]["delta"].any() and got[1]["n_calls"] == 0
        for g, r in ((got[0], ref[0]), (got[2], ref[1])):  # the others unchanged
            assert_trace_equal(g, r)
        check_against_lone(pkg, ctx, mb, [jobs[0], empty, jobs[1]], got)
        assert mb.batch_scan_download(1).shape == (5, 0)
        # all three empty: nothing launched
        got = mb.process_raw_scan_batch([empty, empty, empty], trace=True)
        assert all(g["kept"] == 0 and np.isnan(g["prob"]) and not g["delta"].any() and g["n_calls"] == 0 for g in got)
        assert mb.stats()["kernels_launched"] == 0 and mb.stats()["scorer_calls"] == 0
        # K = 0 and K = 1
        assert mb.process_raw_scan_batch([]) == []
        for job in (jobs[1], empty):
            got = mb.process_raw_scan_batch([job], trace=True)
            check_against_lone(pkg, ctx, mb, [job], got, chains=False)
    finally:
        mb.close()


FALLBACKS = [("MC", dict(), [7, 0.2, 0.1, 20, 100]),
             ("BF", dict(), [-0.1, 0.1, 0.05, -0.1, 0.1, 0.05, -0.04, 0.04, 0.02]),
             ("HC", dict(oope="OOPE_MAX", area=(-0.1, 0.1, -0.1, 0.1)), HC),
             ("HC", dict(sum_order="SUM_SEQUENTIAL"), HC)]


@pytest.mark.parametrize("kind,cfg_kw,prm", FALLBACKS)
def test_fallbacks_equal_the_sequence_of_lone_calls(pkg, ctx, worlds, kind, cfg_kw, prm):
    upload(ctx, worlds, CELL_OCC)
    ws = worlds[CELL_OCC]
    jobs = three_jobs(pkg, ws, "cached", "viny", 256)
    cfg = lambda: pkg.spe_cfg(**{k: getattr(pkg, v) if isinstance(v, str) else v for k, v in cfg_kw.items()})  # noqa: E731
    mb, ml = pkg.Matcher(ctx, kind, cfg(), prm), pkg.Matcher(ctx, kind, cfg(), prm)
    try:
        got = mb.process_raw_scan_batch(jobs, trace=True)
        for c, (g, job) in enumerate(zip(got, jobs)):  # ONE lone matcher: a Monte-Carlo engine runs on from match to match
            want = lone_raw(pkg, ml, job)
            assert g["kept"] == want["kept"]
            assert_trace_equal(g, want)
            st = mb.batch_stats(c)
            assert st["scorer_calls"] == want["n_calls"] and not st["on_device_chain"]
        # the next lone match of both: the engine's position after the batch is that after the lone calls
        a, b = lone_raw(pkg, mb, jobs[1]), lone_raw(pkg, ml, jobs[1])
        assert_trace_equal(a, b)
    finally:
        mb.close()
        ml.close()


def test_a_job_with_4097_kept_beams_sends_the_batch_through_the_lone_calls(pkg, ctx, worlds):
    upload(ctx, worlds, CELL_OCC)
    ws = worlds[CELL_OCC]
    small = three_jobs(pkg, ws, "raw", "even", 255)
    n = 4097
    s = scanner(n)
    rng = np.interp(np.linspace(0, N_A - 1, n), np.arange(N_A), np.minimum(ws[0]["raw"][N_A][0], 12.0))
    big = dict(small[1], range=rng, angle=s["angle"], is_occ=None, factor=None, a_min=s["a_min"], a_max=s["a_max"], a_inc=s["a_inc"])
    jobs = [small[1], big, small[2]]
    mb = pkg.Matcher(ctx, "HC", pkg.spe_cfg(), HC)
    try:
        got = mb.process_raw_scan_batch(jobs, trace=True)
        assert [g["kept"] for g in got] == [255, n, 1]
        check_against_lone(pkg, ctx, mb, jobs, got, chains=False)
    finally:
        mb.close()


def test_the_callers_scans_are_left_alone(pkg, ctx, worlds):
    upload(ctx, worlds, CELL_OCC)
    ws = worlds[CELL_OCC]
    jobs = three_jobs(pkg, ws, "raw", "viny", 513)
    f, _ = filtered(pkg, jobs[1])
    ctx.scan_store(5, f["range"], f["cos_a"], f["sin_a"], f["weight"], f["factor"])
    ctx.scan_select(5)
    own = pkg.Matcher(ctx, "HC", pkg.spe_cfg(), HC)
    mb = pkg.Matcher(ctx, "HC", pkg.spe_cfg(), HC)
    ms = pkg.Matcher(ctx, "HC", pkg.spe_cfg(sum_order=pkg.SUM_SEQUENTIAL), HC)
    try:
        before, slot = own.process_scan(0, jobs[1]["init_pose"], trace=True), download(ctx)
        got = mb.process_raw_scan_batch(jobs)  # the shared launches: the selection is not touched
        assert mb.batch_stats(0)["on_device_chain"]
        np.testing.assert_array_equal(download(ctx), slot)
        assert_trace_equal(own.process_scan(0, jobs[1]["init_pose"], trace=True), before)
        seq = ms.process_raw_scan_batch(jobs)  # lone calls inside: the selection is put back
        assert not ms.batch_stats(0)["on_device_chain"] and [g["kept"] for g in seq] == [g["kept"] for g in got]
        np.testing.assert_array_equal(download(ctx), slot)
        assert_trace_equal(own.process_scan(0, jobs[1]["init_pose"], trace=True), before)
        # ... and the stored scan itself is what it was: a batch job that names the slot matches it as before
        via_slot = own.process_scan_batch([dict(map_id=0, scan_slot=5, init_pose=jobs[1]["init_pose"])] * 2, trace=True)
        assert_trace_equal(via_slot[0], before)
    finally:
        for m in (own, mb, ms):
            m.close()


def test_tables_go_up_once_per_scanner(pkg, worlds):
    c = pkg.Context(0)
    mb = pkg.Matcher(c, "HC", pkg.spe_cfg(), HC)
    try:
        upload(c, worlds, CELL_OCC)
        ws = worlds[CELL_OCC]
        jobs = three_jobs(pkg, ws, "cached", "viny", 256)
        got = mb.process_raw_scan_batch(jobs, trace=True)
        assert table_uploads(c) == 2  # two scanners among three jobs
        # new ranges from the same scanners, back to back: no upload, both calls right
        rs = np.random.RandomState(3)
        jobs2 = [dict(j, range=j["range"] * (1.0 + 0.002 * rs.randn(j["range"].size))) for j in three_jobs(pkg, ws, "cached", "viny", 511)]
        got2 = mb.process_raw_scan_batch(jobs2, trace=True)
        got3 = mb.process_raw_scan_batch(jobs, trace=True)
        assert table_uploads(c) == 2
        # a changed scanner: one more
        moved = dict(jobs[2], angle=jobs[2]["angle"].copy())
        moved["angle"][17] = np.nextafter(moved["angle"][17], 10.0)
        got4 = mb.process_raw_scan_batch([jobs[0], jobs[1], moved], trace=True)
        assert table_uploads(c) == 3
        before = table_uploads(c)
        check_against_lone(pkg, c, mb, [jobs[0], jobs[1], moved], got4)  # (the lone calls upload the context's own table)
        for g, r in zip(got3, got):
            assert_trace_equal(g, r)
        mb.process_raw_scan_batch(jobs2)
        check_against_lone(pkg, c, mb, jobs2, got2)
        assert table_uploads(c) > before
    finally:
        mb.close()
        c.close()


def test_errors_launch_nothing(pkg, worlds):
    c = pkg.Context(0)
    mb = pkg.Matcher(c, "HC", pkg.spe_cfg(), HC)
    pyr = m3 = None
    try:
        upload(c, worlds, CELL_OCC)
        c.upload_map(7, worlds[CELL_TBM][0]["map"])
        ws = worlds[CELL_OCC]
        jobs = three_jobs(pkg, ws, "cached", "even", 257)
        good = mb.process_raw_scan_batch(jobs)
        state = (mb.stats(), [mb.batch_stats(k) for k in range(3)], table_uploads(c))

        def refused(block_or_jobs, text):
            with pytest.raises(pkg.SlamHipError, match=text):
                mb.process_raw_scan_batch(block_or_jobs)
            assert (mb.stats(), [mb.batch_stats(k) for k in range(3)], table_uploads(c)) == state

        refused([jobs[0], dict(jobs[1], map_id=5), jobs[2]], "unknown map id")
        refused([jobs[0], dict(jobs[1], map_id=7), jobs[2]], "share a cell model")
        refused([jobs[0], dict(jobs[1], trig_mode=7), jobs[2]], "trig mode")
        refused([jobs[0], dict(jobs[1], a_max=jobs[1]["a_min"] + 100 * jobs[1]["a_inc"]), jobs[2]], "outside the trig table")
        refused([jobs[0], dict(jobs[1], a_inc=0.0), jobs[2]], "bad arguments")
        for field, value in (("n", 0), ("n", -3), ("range", None), ("angle", None), ("weighting", 5)):
            blk = mb.make_raw_batch(jobs)
            setattr(blk["raw_arr"][2].scan, field, value)
            refused(blk, "bad scan|weighting")
        # ... and the matcher goes on as before
        for g, a in zip(good, mb.process_raw_scan_batch(jobs)):
            assert bits(g["prob"]) == bits(a["prob"]) and np.array_equal(bits(g["delta"]), bits(a["delta"]))
        # a multi-resolution matcher is refused, as by process_scan_batch
        pyr = pkg.Pyramid(c, 0, pkg.OIE_DISCREPANCY, 10)
        m3 = pkg.Matcher(c, "BF_M3RSM", pkg.spe_cfg(oope=pkg.OOPE_MAX), [pyr, 0.2, 0.2, 0.05, 0.02, 0.1])
        with pytest.raises(pkg.SlamHipError, match="not batched"):
            m3.process_raw_scan_batch(jobs)
    finally:
        for o in (m3, pyr, mb):
            if o is not None:
                o.close()
        c.close()


def test_two_contexts_on_one_device(pkg, worlds):
    a, b = pkg.Context(0), pkg.Context(0)
    ma, mb = pkg.Matcher(a, "HC", pkg.spe_cfg(), HC), pkg.Matcher(b, "HC", pkg.spe_cfg(), HC)
    try:
        upload(a, worlds, CELL_OCC)
        upload(b, worlds, CELL_TBM)
        ja = three_jobs(pkg, worlds[CELL_OCC], "raw", "ahr", 511)
        jb = three_jobs(pkg, worlds[CELL_TBM], "cached", "viny", 257, seed=1)
        ga, gb = [], []
        for _ in range(2):  # alternating
            ga.append(ma.process_raw_scan_batch(ja, trace=True))
            gb.append(mb.process_raw_scan_batch(jb, trace=True))
        assert table_uploads(a) == 2 and table_uploads(b) == 2
        for first, again in ((ga[0], ga[1]), (gb[0], gb[1])):
            for g, r in zip(first, again):
                assert_trace_equal(g, r)
        check_against_lone(pkg, a, ma, ja, ga[1])
        check_against_lone(pkg, b, mb, jb, gb[1])
    finally:
        ma.close()
        mb.close()
        a.close()
        b.close()
