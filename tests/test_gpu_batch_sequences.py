"""GPU suite: batch calls BACK TO BACK on one context, their shape changing from call to call -- the production loop of
slamhip_matcher_process_scan_batch / _process_raw_scan_batch / slamhip_map_append_scan_batch.

hc_batch_run and mc_batch_run (csrc/matchers.cpp) queue the next burst of step kernels and its marker before they wait for
the previous marker, so every call returns with launches still queued; the tests of test_gpu_batch.py / test_gpu_mc_batch.py
compute their expectations with lone matches on the SAME context after every call, which drains the stream.  Here a
sequence of calls runs to its end on context A with NOTHING else issued on A between two calls (no lone match, no download,
no synchronize; the counters read per call -- batch_stats, mc_stream_info, stats -- are plain host fields:
slamhip_matcher_batch_stats, _mc_stream_info, _stats, _timing, _chain_stats, _tail_stats touch no stream).  Only then the
expectations are computed: the same inputs in the same order through lone matchers on a SECOND context B with the same
maps -- Monte-Carlo: lone matcher k seeded seeds[k] and fed stream k's jobs in call order -- and compared:

  observer trace (poses, scores, accept flags), result, scorer calls, on_device_chain, engine-stream position: bit for bit;
  one OCC sequence per matcher form additionally against the oracle's strict loop: identical accept trace, scores to
  rtol 1e-12 (the default mode's contract, DESIGN.md section 5, as test_batch_against_the_oracle has it).

What a matcher carries from call to call and a sequence therefore crosses: the chains' capacity (control, result and staging
blocks reallocated when K outgrows it), the observer's trace slices (laid out again when the capacity grows; their length
per chain is fixed when the matcher is created, so "longer matches arriving" is a second matcher with larger limits on the
same context), the smoothed chain length that sizes the first burst, the epochs in HBM, the done count, and the context's
one marker flag and sequence number that all matchers share.

Shapes: two oblong, off-centre windows of 200 x 160 and 192 x 156 cells at 0.05 m, beam counts 1 / 63 / 64 / 65 / 257 / 360,
K from 1 to 20, at most 40 calls per sequence."""
import ctypes as C
import types

import numpy as np
import pyoracle as po
import pytest
import test_gpu_mc_batch as mcb
import test_gpu_raw_batch as rb
from helpers import assert_trace_equal
from mapupdate_oblong_cases import AUX_STRIDE, MODELS, STRIDE
from synth import CELL_OCC, Scan, cast_scan, make_scene

import __graft_entry__ as ge

pytestmark = pytest.mark.gpu

FORMS = ("hc_chain", "hc_resident", "mc")  # kernel chains (set_device_chain(1)), co-resident launch (2), MC with streams
HC_LIMITS = ([1, 0.1, 0.1], [6, 0.1, 0.1], [60, 0.1, 0.1])
MC_LIMITS = ((3, 2), (20, 100), (64, 512))
BEAMS = (1, 63, 64, 65, 257, 360)
ERR = np.array([0.07, -0.04, 0.03])
BLANK = 2  # map id of the all-unknown map, beside the two windows' 0 and 1


@pytest.fixture(scope="module")
def pkg():
    return ge.load_package()


@pytest.fixture(scope="module")
def two(pkg):
    """contexts A (the sequences) and B (the lone route)"""
    a, b = pkg.Context(0), pkg.Context(0)
    yield a, b
    a.close()
    b.close()


@pytest.fixture(scope="module")
def two_testing(pkg):
    """the same of libslamhip_testing.so -- the build with the test hooks compiled in"""
    a, b = pkg.Context(0, testing=True), pkg.Context(0, testing=True)
    yield a, b
    a.close()
    b.close()


# ---- worlds, windows, jobs (built once)
_worlds = {}


def worlds_of(cell):
    """two scenes with oblong, off-centre windows cropped out of their maps (as test_gpu_mc_batch.worlds_of does: walls
    beyond the window's rim score as unknown cells), a smaller third window of scene 1 and an all-unknown copy of window 0"""
    if cell not in _worlds:
        out = []
        for mi in range(2):
            sc = make_scene(cell_model=cell, size=240, scale=0.05, n_beams=360, seed=5 + mi)
            x0, y0 = 10 + 20 * mi, 30 + 10 * mi
            sc["window"] = mcb.crop(sc["map"], x0, x0 + 200 - 8 * mi, y0, y0 + 160 - 4 * mi)
            out.append(sc)
        w = out[0]["window"]
        out[0]["blank"] = types.SimpleNamespace(**dict(vars(w), payload=np.full_like(w.payload, 0.0) + w.unknown[:w.payload.shape[2]]))
        out[1]["third"] = mcb.crop(out[1]["map"], 40, 40 + 150, 50, 50 + 120)
        for sc in out:
            w = sc["window"]
            assert w.width != w.height and w.origin[0] != w.origin[1] and (w.width, w.height) != (240, 240)
        _worlds[cell] = out
    return _worlds[cell]


_pool = {}


def pool_job(pkg, cell, i, err=None, n=None):
    """job i of an endless pool: window i % 2, beam count BEAMS[i % 6] (exactly: a full scan thinned), the robot's pose
    jittered, an initial error of (i % 4) times the default one (or `err` times)"""
    n = BEAMS[i % len(BEAMS)] if n is None else n
    key = (cell, i, n)
    if key not in _pool:
        sc = worlds_of(cell)[i % 2]
        true = sc["true_pose"] + np.random.RandomState(300 + i).randn(3) * [0.15, 0.15, 0.05]
        rng0, ang0 = cast_scan(sc["gt"], 0.05, true, 360, seed=42 + i)
        assert rng0.size >= n
        idx = np.linspace(0, rng0.size - 1, n).astype(int)
        rng, ang = np.ascontiguousarray(rng0[idx]), np.ascontiguousarray(ang0[idx])
        cos_a, sin_a = pkg.beam_trig(ang)
        _pool[key] = dict(map_id=i % 2, range=rng, cos_a=cos_a, sin_a=sin_a, weight=np.full(n, 1.0 / n), factor=None,
                          angle=ang, true=true)
    j = _pool[key]
    return dict(j, init_pose=j["true"] + ERR * float(i % 4 if err is None else err))


def raw_pool_job(pkg, cell, i, n=None, empty=False):
    """raw job i: every beam of a scanner of BEAMS[1 + i % 5] beams as the scanner hands it over (is_occ marks the hits),
    the host filter and the even weights left to the call"""
    n = BEAMS[1 + i % 5] if n is None else n
    key = (cell, "raw", i, n)
    if key not in _pool:
        sc = worlds_of(cell)[i % 2]
        true = sc["true_pose"] + np.random.RandomState(700 + i).randn(3) * [0.15, 0.15, 0.05]
        rng, ang, occ = cast_scan(sc["gt"], 0.05, true, n, seed=90 + i, raw=True)
        _pool[key] = dict(map_id=i % 2, range=rng, angle=ang, is_occ=occ, weighting="even", true=true)
    j = _pool[key]
    out = dict(j, init_pose=j["true"] + ERR * float(i % 4))
    if empty:
        out["is_occ"] = np.zeros(n, np.int32)
    return out


# ---- the two routes
def upload(m_id, m, release=False):
    return dict(op="upload", id=m_id, m=m, release=release)


def call(m, jobs, trace=True, raw=False, sid=None, cap=0, raises=None):
    return dict(op="call", m=m, jobs=jobs, trace=trace, raw=raw, sid=sid, cap=cap, raises=raises)


class Rig:
    """Batch matchers on context A, their lone counterparts on context B, and the two passes over a list of steps."""

    def __init__(self, pkg, two, cell=CELL_OCC, testing=False):
        self.pkg, (self.a, self.b), self.cell, self.testing = pkg, two, cell, testing
        self.ms = {}
        self.maps = {}  # map id -> what is bound there on B (the oracle's map)
        ws = worlds_of(cell)
        for ctx in two:
            for mi in range(2):
                ctx.upload_map(mi, ws[mi]["window"])
            ctx.upload_map(BLANK, ws[0]["blank"])
        self.first_maps = {0: ws[0]["window"], 1: ws[1]["window"], BLANK: ws[0]["blank"]}
        if testing:
            self.hook = pkg.load(testing=True).slamhip_matcher_debug_trace_cap
            self.hook.argtypes = [C.c_void_p, C.c_int]

    def matcher(self, name, form, lim, k=1):
        """lim: index into HC_LIMITS / MC_LIMITS; k: engine streams of a Monte-Carlo matcher"""
        pkg = self.pkg
        if form == "mc":
            seeds = mcb.seeds_of(k)
            mb = pkg.Matcher(self.a, "MC", pkg.spe_cfg(), mcb.prm(1, MC_LIMITS[lim]))
            mb.set_mc_streams(seeds)
            lones = [pkg.Matcher(self.b, "MC", pkg.spe_cfg(), mcb.prm(s, MC_LIMITS[lim])) for s in seeds]
            self.ms[name] = dict(mc=True, mb=mb, lones=lones, prm=[mcb.prm(s, MC_LIMITS[lim]) for s in seeds])
        else:
            mb = pkg.Matcher(self.a, "HC", pkg.spe_cfg(), HC_LIMITS[lim])
            mb.set_device_chain(1 if form == "hc_chain" else 2)
            ml = pkg.Matcher(self.b, "HC", pkg.spe_cfg(), HC_LIMITS[lim])
            ml.set_device_chain(1)
            self.ms[name] = dict(mc=False, mb=mb, lones=[ml], prm=HC_LIMITS[lim])
        return self.ms[name]

    def close(self):
        for m in self.ms.values():
            mcb.close_all(m["mb"], m["lones"])

    # -- context A: the calls, nothing between them
    def run_a(self, steps):
        recs = []
        for s in steps:
            if s["op"] == "upload":
                if s["release"]:
                    self.a.map_release(s["id"])
                self.a.upload_map(s["id"], s["m"])
                recs.append(None)
                continue
            m = self.ms[s["m"]]
            mb, n = m["mb"], len(s["jobs"])
            sid = list(range(n)) if s["sid"] is None else s["sid"]
            if m["mc"]:
                mb.set_mc_job_streams(s["sid"])
            if self.testing:
                assert self.hook(mb.h, s["cap"]) == 0
            fn = mb.process_raw_scan_batch if s["raw"] else mb.process_scan_batch
            if s["raises"]:
                before = ([mb.batch_stats(j) for j in range(n)], mb.stats()["scorer_calls"],
                          [mb.mc_stream_info(k) for k in range(len(m["lones"]))] if m["mc"] else None)
                with pytest.raises(self.pkg.SlamHipError, match=s["raises"]):
                    fn(s["jobs"], trace=s["trace"])
                after = ([mb.batch_stats(j) for j in range(n)], mb.stats()["scorer_calls"],
                         [mb.mc_stream_info(k) for k in range(len(m["lones"]))] if m["mc"] else None)
                assert after == before  # refused before a stream or the last-batch state is touched
                recs.append(None)
                continue
            got = fn(s["jobs"], trace=s["trace"])
            assert len(got) == n
            st = mb.stats()
            recs.append(dict(got=got, stats=[mb.batch_stats(j) for j in range(n)], total=st["scorer_calls"],
                             launched=st["kernels_launched"],
                             streams=[mb.mc_stream_info(k) for k in sid] if m["mc"] else None))
        return recs

    # -- context B: the lone route, in the same order
    def lone(self, ml, job, trace, raw):
        if raw:
            return rb.lone_raw(self.pkg, ml, job, trace=trace)
        if job.get("scan_slot") is not None:
            self.b.scan_select(job["scan_slot"])
            return ml.process_scan(job["map_id"], job["init_pose"], trace=trace)
        return mcb.lone(self.b, ml, job, trace=trace)

    def run_b(self, steps, recs=None, oracle=None):
        """the steps through the lone matchers; with `recs`: every call of run_a compared.  Returns the lone results."""
        wants = []
        self.maps = dict(self.first_maps)
        enums = {}
        for at, s in enumerate(steps):
            if s["op"] == "upload":
                if s["release"]:
                    self.b.map_release(s["id"])
                self.b.upload_map(s["id"], s["m"])
                self.maps[s["id"]] = s["m"]
                wants.append(None)
                continue
            if s["raises"]:
                wants.append(None)
                continue
            m = self.ms[s["m"]]
            n = len(s["jobs"])
            sid = list(range(n)) if s["sid"] is None else s["sid"]
            rec = recs[at] if recs is not None else None
            want_all, calls = [], 0
            for j, job in enumerate(s["jobs"]):
                ml = m["lones"][sid[j] if m["mc"] else 0]
                want = self.lone(ml, job, s["trace"], s["raw"])
                want["scorer_calls"] = ml.stats()["scorer_calls"]
                want_all.append(want)
                if rec is None:
                    continue
                where = "call %d (%s), job %d" % (at, s["m"], j)
                g, st = rec["got"][j], rec["stats"][j]
                if s["raw"]:
                    assert g["kept"] == want["kept"], where
                if s["raw"] and want["kept"] == 0:  # nothing kept: NaN, zero delta, no observer call, no stream advanced
                    assert np.isnan(g["prob"]) and not g["delta"].any() and g.get("n_calls", 0) == 0, where
                    assert st == dict(scorer_calls=0, poses_evaluated=0, super_steps=0, on_device_chain=False), where
                else:
                    if s["trace"]:
                        mcb.same_trace(g, want)
                        assert want["n_calls"] == want["scorer_calls"], where
                    else:
                        assert g["prob"] == want["prob"] or (np.isnan(g["prob"]) and np.isnan(want["prob"])), where
                        np.testing.assert_array_equal(g["delta"], want["delta"], err_msg=where)
                    assert st["scorer_calls"] == want["scorer_calls"], where
                    # on the shared launches, unless the call is one job (the lone route) or the hook's cap is in the way
                    if s["raw"]:  # (the jobs that keep something are the chains' jobs)
                        on = sum(1 for q in s["jobs"] if np.any(q["is_occ"])) > 1
                    else:
                        on = n > 1 and (not s["cap"] or want["n_calls"] <= s["cap"])
                    assert st["on_device_chain"] == on, where
                    calls += st["scorer_calls"]
                if m["mc"]:
                    assert rec["streams"][j] == ml.mc_stream_info(-1), where
                if oracle is not None and s["trace"] and not s["raw"]:
                    key = (s["m"], sid[j])
                    if m["mc"] and key not in enums:
                        enums[key] = oracle.enumerator(po.SM_MC, m["prm"][sid[j]])
                    e = enums[key] if m["mc"] else oracle.enumerator(po.SM_HC, m["prm"])
                    r = oracle.process_scan(e, self.maps[job["map_id"]], Scan(job["range"], job["angle"], job["weight"]),
                                            po.make_cfg(), job["init_pose"])
                    assert_trace_equal(g, r, exact_scores=False, rtol=1e-12)
            if rec is not None:
                assert rec["total"] == calls, "call %d" % at
            wants.append(want_all)
        return wants

    def run(self, steps, oracle=None):
        recs = self.run_a(steps)
        return recs, self.run_b(steps, recs, oracle)


def jobs_of(pkg, cell, call_no, k, err=None, map_id=None):
    """the K jobs of a call: stream j meets another scan, window and beam count in every call"""
    out = []
    for j in range(k):
        job = pool_job(pkg, cell, 7 * call_no + j, err=err)
        out.append(job if map_id is None else dict(job, map_id=map_id))
    return out


# ---- 1. same K, the chains' lengths swinging
@pytest.mark.parametrize("form", FORMS)
def test_same_k_lengths_swinging(pkg, two, oracle, form):
    """K = 4, 40 calls on ONE matcher at the longest limits: 10 calls of long chains (three times the default initial
    error), 10 of the shortest there are (no error, an all-unknown map: no candidate beats the initial pose), 10 long, 10
    mixed.  After short calls the first burst is far too long -- dozens of launches run past the chains' ends and return on
    done_epoch, under the next call's staging; after long calls the wait loop goes many rounds.  OCC: every traced job
    also against the oracle's strict loop."""
    rig = Rig(pkg, two)
    try:
        rig.matcher("m", form, 2, k=4)
        steps = []
        for c in range(40):
            phase = c // 10
            if phase in (0, 2):
                jobs = jobs_of(pkg, CELL_OCC, c, 4, err=3.0 - 0.1 * (c % 10))
            elif phase == 1:
                jobs = jobs_of(pkg, CELL_OCC, c, 4, err=0.0, map_id=BLANK)
            else:
                jobs = [dict(job, map_id=BLANK if (c + j) % 3 == 0 else job["map_id"])
                        for j, job in enumerate(jobs_of(pkg, CELL_OCC, c, 4))]
            steps.append(call("m", jobs))
        recs, _ = rig.run(steps, oracle)
        # the lengths really swing: the longest chain's super-steps, call by call
        steps_of = [max(st["super_steps"] for st in r["stats"]) for r in recs]
        print("super-steps of the longest chain per call %r\nkernels launched per call %r" % (steps_of, [r["launched"] for r in recs]))
        assert min(steps_of[0:10] + steps_of[20:30]) > max(steps_of[10:20]), steps_of
        if form != "hc_resident":
            # the premise: the driver has the next burst (two kernels or more) queued when the marker that ends the call
            # arrives, so every call returns with launches the chains no longer need
            assert all(r["launched"] >= s + 2 for r, s in zip(recs, steps_of))
    finally:
        rig.close()


# ---- 2. K shrinking and returning
@pytest.mark.parametrize("form", FORMS)
def test_k_shrinking_and_returning(pkg, two, form):
    """20 -> 4 -> 1 -> 4 -> 20 -> 3: the done count and the result slots a larger call left are >= the next call's n;
    K = 1 is the lone route inside the batch call.  Monte-Carlo: the second K = 4 call on streams 7, 2, 19, 0."""
    rig = Rig(pkg, two)
    try:
        rig.matcher("m", form, 1, k=20)
        steps = []
        for rnd in range(2):
            for c, k in enumerate((20, 4, 1, 4, 20, 3)):
                sid = [7, 2, 19, 0] if (form == "mc" and c == 3) else None
                steps.append(call("m", jobs_of(pkg, CELL_OCC, 6 * rnd + c, k), trace=not (rnd == 1 and c in (1, 4)), sid=sid))
        rig.run(steps)
    finally:
        rig.close()


# ---- 3. K growing across the capacity
@pytest.mark.parametrize("form", FORMS)
def test_k_growing_across_the_capacity(pkg, two, form):
    """8 -> 9 -> 17 -> 8 (-> 20 -> 2): the chains' control, result and staging blocks -- and the trace slices -- are
    reallocated (capacity 8 -> 16 -> 32) while the call before has launches queued"""
    rig = Rig(pkg, two)
    try:
        rig.matcher("m", form, 1, k=20)
        steps = [call("m", jobs_of(pkg, CELL_OCC, c, k)) for c, k in enumerate((8, 9, 17, 8, 20, 2))]
        rig.run(steps)
    finally:
        rig.close()


# ---- 4. observer on / off / on, matchers with longer matches arriving
@pytest.mark.parametrize("form", FORMS)
def test_observer_on_off_on_and_longer_matches(pkg, two, form):
    """A matcher at the middle limits: no observer for the first calls (K = 9: the blocks exist, the trace slices do not),
    then on (the slices are made), off, on at K = 17 (capacity grows: laid out again).  Then a second matcher at the longest
    limits on the same context -- Monte Carlo (64, 512) after (20, 100), hill climbing 60 after 6: its slices are longer --
    alternating with the first, the observer going on and off on both."""
    rig = Rig(pkg, two)
    try:
        rig.matcher("p", form, 1, k=17)
        rig.matcher("q", form, 2, k=9)
        plan = [("p", 9, False), ("p", 9, False), ("p", 9, True), ("p", 4, False), ("p", 17, True), ("q", 9, True),
                ("p", 9, True), ("q", 4, False), ("q", 9, True), ("p", 17, False), ("q", 3, True), ("p", 3, True)]
        steps = [call(m, jobs_of(pkg, CELL_OCC, c, k, err=2.0 if m == "q" else None), trace=t) for c, (m, k, t) in enumerate(plan)]
        rig.run(steps)
    finally:
        rig.close()


# ---- 5. two matchers alternating on one context
@pytest.mark.parametrize("mode", ["hc_chain", "hc_resident"])
def test_two_matchers_alternating(pkg, two, mode):
    """MC batch, HC batch, MC batch, ... at K = 4 and K = 8: each has its own batch state, they share the context's one
    marker flag and sequence number (and the marker of one's queued burst lands under the other's wait)"""
    rig = Rig(pkg, two)
    try:
        rig.matcher("mc", "mc", 1, k=8)
        rig.matcher("hc", mode, 1)
        steps = []
        for c in range(12):
            steps.append(call("mc" if c % 2 == 0 else "hc", jobs_of(pkg, CELL_OCC, c, 4 if (c // 2) % 2 == 0 else 8), trace=c % 5 != 4))
        rig.run(steps)
    finally:
        rig.close()


# ---- 6. packed and raw entry alternating; the caller's scan
@pytest.mark.parametrize("form", FORMS)
def test_packed_and_raw_entry_alternating(pkg, two, form):
    """process_scan_batch and process_raw_scan_batch on one matcher, jobs naming stored scan slots among them, calls of one
    job (the lone route: its scan becomes the context's current one), a raw job that keeps nothing.  The caller's own
    selection -- stored scan 20 with its angles -- is what it was when the sequence ends: the scan block bit for bit, and
    a SLAMHIP_POSE_TRIG_RAW_EXACT scoring call (which needs the angles) gives the bits it gave before the first call."""
    rig = Rig(pkg, two)
    a = two[0]
    try:
        rig.matcher("m", form, 1, k=4)
        stored = [pool_job(pkg, CELL_OCC, 50 + q) for q in range(4)]
        for ctx in two:
            for q, j in enumerate(stored):
                ctx.scan_store(10 + q, j["range"], j["cos_a"], j["sin_a"], j["weight"])
        slot = [dict(map_id=j["map_id"], scan_slot=10 + q, init_pose=j["init_pose"]) for q, j in enumerate(stored)]
        own = pool_job(pkg, CELL_OCC, 60, n=257)
        a.scan_store(20, own["range"], own["cos_a"], own["sin_a"], own["weight"])
        a.scan_store_angles(20, own["angle"])
        a.scan_select(20)
        cfg = pkg.spe_cfg(pose_trig=pkg.POSE_TRIG_RAW_EXACT)
        poses = own["true"] + np.random.RandomState(7).randn(8, 3) * [0.1, 0.1, 0.05]
        scores, block = a.score_poses(0, cfg, poses), rb.download(a)
        assert block.shape == (5, 257)
        pj = lambda i: pool_job(pkg, CELL_OCC, i)  # noqa: E731
        rj = lambda i, **kw: raw_pool_job(pkg, CELL_OCC, i, **kw)  # noqa: E731
        steps = [call("m", [slot[0], pj(1), slot[2], pj(3)]),
                 call("m", [rj(0), rj(1), rj(2), rj(3)], raw=True),
                 call("m", [slot[1]]),
                 call("m", [rj(4), rj(5, empty=True), rj(6)], raw=True),
                 call("m", [pj(5)]),
                 call("m", [rj(7)], raw=True),
                 call("m", [pj(6), slot[3], slot[0], pj(9)], trace=False),
                 call("m", [rj(8), rj(9), rj(10, empty=True), rj(11)], raw=True),
                 call("m", [slot[2], slot[1]])]
        recs = rig.run_a(steps)
        np.testing.assert_array_equal(rb.download(a), block)  # (the ScanKeeper's promise)
        assert np.array_equal(a.score_poses(0, cfg, poses), scores)
        rig.run_b(steps, recs)
    finally:
        rig.close()


# ---- 7. a refused call in the middle
@pytest.mark.parametrize("form", FORMS)
def test_a_refused_call_in_the_middle(pkg, two, form):
    """a call with an unknown map id between good ones: it raises, advances no stream, changes no counter, and the calls
    after it equal the lone route (which never saw it).  At the shortest limits: hill climbing 1, Monte Carlo (3, 2)."""
    rig = Rig(pkg, two)
    try:
        rig.matcher("m", form, 0, k=8)
        bad = jobs_of(pkg, CELL_OCC, 9, 4)
        bad[2] = dict(bad[2], map_id=17)
        steps = [call("m", jobs_of(pkg, CELL_OCC, 0, 4)), call("m", jobs_of(pkg, CELL_OCC, 1, 8)),
                 call("m", bad, raises="unknown map id"), call("m", jobs_of(pkg, CELL_OCC, 2, 8)),
                 call("m", bad, raises="unknown map id", trace=False), call("m", jobs_of(pkg, CELL_OCC, 3, 4))]
        rig.run(steps)
    finally:
        rig.close()


# ---- 8. a fall-back in the middle
@pytest.mark.parametrize("form", FORMS)
def test_a_fallback_in_the_middle(pkg, two_testing, form):
    """the slamhip_matcher_debug_trace_cap hook sends the jobs of ONE call whose traces outgrow the cap to the lone route
    (inside the batch call, on their own streams); the hook is lifted for the next call: every job is on the chains again
    and the streams go on where the lone matchers do"""
    rig = Rig(pkg, two_testing, testing=True)
    try:
        rig.matcher("m", form, 1, k=4)
        rig.matcher("probe", form, 1, k=4)
        steps = [call("m", jobs_of(pkg, CELL_OCC, c, 4)) for c in range(5)]
        # the cap: between the trace lengths of call 2 (the lone route's, from matchers that are used for nothing else)
        lengths = sorted(w["n_calls"] for w in rig.run_b([dict(s, m="probe") for s in steps[:3]])[2])
        assert lengths[0] < lengths[-1], lengths
        gap = max(range(3), key=lambda q: lengths[q + 1] - lengths[q])
        assert lengths[gap + 1] - lengths[gap] >= 2, lengths
        steps[2]["cap"] = (lengths[gap] + lengths[gap + 1]) // 2
        recs, _ = rig.run(steps)
        on = [st["on_device_chain"] for st in recs[2]["stats"]]
        assert 1 <= sum(on) < 4, (lengths, on)
        for c in (0, 1, 3, 4):
            assert all(st["on_device_chain"] for st in recs[c]["stats"]), c
    finally:
        rig.close()


# ---- 9. maps changing under queued launches
@pytest.mark.parametrize("form", FORMS)
def test_maps_changing_under_queued_launches(pkg, two, form):
    """between two calls: upload_map of a window of another size to a map id the call before used (the block in HBM is
    replaced while that call's run-ahead launches are queued); later map_release + a new bind of that id; an all-unknown
    map under id 0"""
    rig = Rig(pkg, two)
    ws = worlds_of(CELL_OCC)
    try:
        rig.matcher("m", form, 1, k=8)
        steps = [call("m", jobs_of(pkg, CELL_OCC, 0, 8)),
                 upload(1, ws[1]["third"]),
                 call("m", jobs_of(pkg, CELL_OCC, 1, 8)),
                 call("m", jobs_of(pkg, CELL_OCC, 2, 4)),
                 upload(1, ws[1]["window"], release=True),
                 call("m", jobs_of(pkg, CELL_OCC, 3, 8)),
                 upload(0, ws[0]["blank"]),
                 call("m", jobs_of(pkg, CELL_OCC, 4, 8), trace=False),
                 upload(0, ws[0]["window"], release=True),
                 upload(1, ws[1]["third"], release=True),
                 call("m", jobs_of(pkg, CELL_OCC, 5, 8))]
        assert (ws[1]["third"].width, ws[1]["third"].height) != (ws[1]["window"].width, ws[1]["window"].height)
        rig.run(steps)
    finally:
        rig.close()


# ---- 10. a fleet loop
_fleet = {}


FLEET_RANGE = 3.0  # the updates' max_range: 60 cells


def fleet_world(cell, mi):
    """a closed 110 x 110 world (walls 2.45 m from its centre) set into an oblong, off-centre window of unknown cells.
    The robots stay within 0.5 m of the world's centre, 77 cells and more from every rim, and the updates take beams of up
    to FLEET_RANGE -- the walls, not the corners: a well-matched pose sends no beam over a rim.  A match of few beams on a
    map that earlier rounds have smeared may wander further (seen: 0.3 rad, and Monte-Carlo walks of most of a metre), so
    the fleet's maps grow (slamhip_map_set_auto_grow) where a fixed window would fail the job -- on both contexts alike."""
    key = (cell, mi)
    if key not in _fleet:
        sc = make_scene(cell_model=cell, size=110, scale=0.05, n_beams=360, seed=11 + mi)
        m = sc["map"]
        left, bottom, w, h = (50, 22, 200, 160) if mi == 0 else (34, 25, 194, 158)
        pay = np.empty((h, w, m.payload.shape[2]))
        pay[:] = m.unknown[:m.payload.shape[2]]
        pay[bottom:bottom + 110, left:left + 110] = m.payload
        sc["window"] = types.SimpleNamespace(cell_model=m.cell_model, payload=pay, width=w, height=h,
                                             origin=(m.origin[0] + left, m.origin[1] + bottom), scale=m.scale, unknown=m.unknown)
        _fleet[key] = sc
    return _fleet[key]


def fleet_job(pkg, cell, k, rnd):
    key = (cell, "job", k, rnd)
    if key not in _fleet:
        sc = fleet_world(cell, k % 2)
        rs = np.random.RandomState(1000 + 31 * k)
        true = sc["true_pose"] + rs.randn(3) * [0.08, 0.08, 0.04] + rnd * np.array([0.01, -0.005, 0.004])
        n = BEAMS[1 + (k + rnd) % 5]
        rng, ang, occ = cast_scan(sc["gt"], 0.05, true, n, seed=500 + 13 * k + rnd, raw=True)
        assert occ.all()  # (a closed world: every beam hits)
        cos_a, sin_a = pkg.beam_trig(ang)
        _fleet[key] = dict(map_id=k, range=rng, angle=ang, is_occ=occ, weighting="even", cos_a=cos_a, sin_a=sin_a,
                           init_pose=true + ERR * (0.5 + 0.25 * ((k + rnd) % 3)))
    return _fleet[key]


@pytest.mark.parametrize("k,name", [(4, "mean"), (9, "tbm")])
@pytest.mark.parametrize("form", FORMS)
def test_a_fleet_loop(pkg, two, form, k, name):
    """12 rounds of [raw-scan match batch, map_append_scan_batch of the same K scans at the matched poses], robot j on its
    own map j: the matches of round r + 1 run on what round r's updates left, the updates queue behind the matches' run-ahead
    launches.  On B: lone raw matches and lone map_append_scan in job order.  Every round's matches as above; at the end
    every map downloaded from both contexts: equal, cell for cell (payload and the mean rule's counters)."""
    a, b = two
    cell, rule = MODELS[name]
    rig = Rig(pkg, two, cell=cell)
    ids = [10 + j for j in range(k)]
    try:
        for ctx in two:
            for j in range(k):
                ctx.upload_map(ids[j], fleet_world(cell, j % 2)["window"])
                ctx.map_set_auto_grow(ids[j], True)
        rig.matcher("m", form, 1, k=k)
        rounds = [[dict(fleet_job(pkg, cell, j, r), map_id=ids[j]) for j in range(k)] for r in range(12)]

        def updates(jobs, res):
            return [dict(map_id=j["map_id"], pose=j["init_pose"] + g["delta"], range=j["range"], cos_a=j["cos_a"], sin_a=j["sin_a"],
                         is_occ=j["is_occ"]) for j, g in zip(jobs, res)]

        # A: nothing but the two batch calls, round after round
        recs, cells_a = [], []
        for jobs in rounds:
            recs += rig.run_a([call("m", jobs, raw=True)])
            nu, status = a.map_append_scan_batch(rule, updates(jobs, recs[-1]["got"]), max_range=FLEET_RANGE)
            assert not status.any()
            cells_a.append(nu)
        # B: the lone route
        for r, jobs in enumerate(rounds):
            want = rig.run_b([call("m", jobs, raw=True)], recs[r:r + 1])[0]
            for q, u in enumerate(updates(jobs, want)):
                nu = b.map_append_scan(u["map_id"], rule, u["pose"], u["range"], u["cos_a"], u["sin_a"], u["is_occ"],
                                       max_range=FLEET_RANGE)
                assert nu == cells_a[r][q] and nu > 0, (r, q)
        assert all(st["on_device_chain"] for rec in recs for st in rec["stats"])
        first = fleet_world(cell, 0)["window"].payload
        for j, mid in enumerate(ids):
            ia, ib = a.map_info(mid), b.map_info(mid)
            assert ia == ib
            w, h = ia["width"], ia["height"]
            pa = a.map_download_window(mid, 0, 0, w, h, STRIDE[cell])
            np.testing.assert_array_equal(pa, b.map_download_window(mid, 0, 0, w, h, STRIDE[cell]), err_msg="map %d" % mid)
            if j == 0:
                assert not np.array_equal(pa, first)  # (the updates wrote)
            if rule in AUX_STRIDE:
                np.testing.assert_array_equal(a.map_download_aux(mid, 0, 0, w, h, AUX_STRIDE[rule]),
                                              b.map_download_aux(mid, 0, 0, w, h, AUX_STRIDE[rule]), err_msg="counters of map %d" % mid)
        print("windows grown (times per map): %r" % [a.map_info(mid)["times_grown"] for mid in ids])
    finally:
        rig.close()
        for ctx in two:
            for mid in ids:
                try:
                    ctx.map_release(mid)
                except pkg.SlamHipError:
                    pass
