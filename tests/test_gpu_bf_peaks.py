"""GPU suite (-m gpu): the peaks of a brute-force sweep's score landscape, picked on the device (slamhip_matcher_bf_peaks
and its batch form; csrc/bf_peaks.hip behind the scoring launch).  Every comparison is exact: lattice indices and score
bits with assert_array_equal, poses bit for bit against the enumerator's additions.  The expected peaks come from the
rule as it reads, a window loop in numpy (numpy_peaks, tests/test_bf_peaks_host.py), over
  * the DESIGNED score tables of tests/landscape_cases.py (a one-beam scan of range 0 scores a pose with the value of the
    cell under it: the author wrote the volume; range 0 makes every theta layer equal),
  * the scores a twin matcher's observer sees in process_scan from the same base, and slamhip_score_poses.
The in-plane kernel (k_bf_peaks_plane) works on tiles of 32 x 8 outputs for radii up to 8 and of 16 x 8 outputs above;
test_windows_across_tile_seams was written for these two tile shapes."""
import numpy as np
import placed_scenes as ps
import pyoracle as po
import pytest
import test_gpu_mc_batch as mcb
from landscape_cases import NAN, Q, background, bf_case, bf_offsets, bf_params, bf_poses, bits, case_map
from synth import CELL_OCC, CELL_TBM, make_scene
from test_bf_peaks_host import numpy_peaks

import __graft_entry__ as ge

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (9, 7, 1), (33, 31, 1), (64, 32, 1), (683, 3, 1), (9, 7, 5)]
R9 = [-0.2, 0.2, 0.01, -0.12, 0.12, 0.01, -0.04, 0.04, 0.02]  # about 41 x 25 x 5


@pytest.fixture(scope="module")
def pkg():
    return ge.load_package()


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def designed(ctx, name, shape, cand):
    """the case of a designed slab (bf_case asserts the MARGIN rule for its end points), uploaded; its volume"""
    c = bf_case(name, shape, 0.6, cand)
    ctx.upload_map(0, case_map(c, po))
    ctx.scan_upload([0.0], [1.0], [0.0], [1.0])
    return c, np.tile(np.asarray(cand, dtype=np.float64), shape[2])


def check(m, c, volume, radius=(1, 1, 1), min_ratio=0.0, min_score=0.0, max_peaks=16):
    got = m.bf_peaks(0, c.inits[0], radius, min_ratio, min_score, max_peaks)
    want_i, want_s = numpy_peaks(volume, c.shape, radius, min_ratio, min_score)
    assert got["shape"] == c.shape
    assert got["n_found"] == len(want_i)
    k = min(max_peaks, len(want_i))
    np.testing.assert_array_equal(got["index"], want_i[:k])
    np.testing.assert_array_equal(bits(got["scores"]), bits(want_s[:k]))
    np.testing.assert_array_equal(bits(got["poses"]), bits(bf_poses(c.shape, c.inits[0])[want_i[:k]].reshape(-1, 3)))
    if radius[2] >= 1:  # (equal layers: a layer's point loses to its copy one layer down)
        assert np.all(got["index"] < c.shape[0] * c.shape[1])
    return got


# ---- 1. designed landscapes
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_designed_landscapes(pkg, ctx, shape):
    nx, ny, _ = shape
    n = nx * ny
    at = lambda ix, iy: min(ix, nx - 1) + nx * min(iy, ny - 1)  # noqa: E731
    m = pkg.Matcher(ctx, "BF", pkg.spe_cfg(), bf_params(shape))
    try:
        # two equal maxima farther apart than the window: both, the lower index first
        s = background(n, 5)
        s[at(0, 0)] = s[at(nx - 1, ny - 1)] = 0.9
        c, v = designed(ctx, "two_far", shape, s)
        got = check(m, c, v, radius=(1, 1, 1))
        if nx > 2 or ny > 2:
            assert got["index"][:2].tolist() == [0, n - 1] and got["scores"][:2].tolist() == [0.9, 0.9]
        # ... the same two inside one window: the lower index only
        s = background(n, 5)
        s[at(nx // 2, ny // 2)] = s[at(nx // 2 + 1, ny // 2 + 1)] = 0.9
        c, v = designed(ctx, "two_near", shape, s)
        got = check(m, c, v, radius=(1, 1, 1))
        assert got["index"][0] == at(nx // 2, ny // 2) and (got["scores"] == 0.9).sum() == 1
        check(m, c, v, radius=(3, 2, 1))
        # a plateau: its first point alone; a plateau above a background
        c, v = designed(ctx, "plateau", shape, np.full(n, 0.75))
        got = check(m, c, v, radius=(1, 1, 1))
        assert got["n_found"] == 1 and got["index"].tolist() == [0]
        s = background(n, 7)
        s.reshape(ny, nx)[ny // 3:ny // 3 + 4, nx // 3:nx // 3 + 5] = 0.8
        c, v = designed(ctx, "plateau_block", shape, s)
        check(m, c, v, radius=(2, 2, 0))
        # NaN beside the maximum, and a maximum walled in by NaN
        s = background(n, 9)
        for dx, dy in ((-1, 0), (1, 0), (0, -1), (0, 1), (1, 1)):
            s[at(max(nx // 2 + dx, 0), max(ny // 2 + dy, 0))] = NAN
        s[at(nx // 2, ny // 2)] = 0.9
        c, v = designed(ctx, "nan_beside", shape, s)
        got = check(m, c, v, radius=(1, 1, 1))
        assert got["index"][0] == at(nx // 2, ny // 2)
        check(m, c, v, radius=(0, 0, 0), max_peaks=5)
        # peaks on a corner, an edge and a face of the volume, and inside
        s = background(n, 11)
        s[at(0, 0)], s[at(nx // 2, 0)], s[at(nx - 1, ny // 2)], s[at(nx // 2, ny // 2)] = 0.9, 0.9 - Q, 0.9 - 2 * Q, 0.9 - 3 * Q
        s[at(nx - 1, ny - 1)] = 0.9 - 4 * Q
        c, v = designed(ctx, "faces", shape, s)
        check(m, c, v, radius=(1, 1, 1))
        check(m, c, v, radius=(3, 2, 1))
        check(m, c, v, radius=(32, 32, 32))  # (wider than every axis: the lattice maximum alone)
        # floors at exact equality: 0.75 = 0.75 x 1.0 stays, one quantum below goes; min_score likewise
        s = background(n, 13) * 0.5 + 0.25  # (multiples of 2^-21 in [0.5, 0.625))
        s[at(0, 0)], s[at(nx - 1, 0)], s[at(0, ny - 1)], s[at(nx - 1, ny - 1)] = 1.0, 0.75, 0.75 - Q, 0.875
        c, v = designed(ctx, "floors", shape, s)
        far = (min(3, max(nx // 3, 0)), min(2, max(ny // 3, 0)), 1)
        got = check(m, c, v, radius=far, min_ratio=0.75)
        if nx >= 9 and ny >= 7:
            assert sorted(got["scores"].tolist()) == [0.75, 0.875, 1.0]
        check(m, c, v, radius=far, min_score=0.75)
        check(m, c, v, radius=far, min_ratio=1.0)
        check(m, c, v, radius=far, min_ratio=0.5, min_score=0.875)
        # max_peaks below n_found (the N best poses), and count only
        got = check(m, c, v, radius=(0, 0, 1), max_peaks=3)
        assert got["n_found"] == n and len(got["index"]) == min(3, n)
        got = check(m, c, v, radius=(1, 1, 1), max_peaks=0)
        assert got["index"].size == 0 and got["n_found"] >= 1
        # nothing but NaN
        c, v = designed(ctx, "all_nan", shape, np.full(n, NAN))
        assert check(m, c, v)["n_found"] == 0
    finally:
        m.close()


# ---- 2. windows across the seams of the in-plane kernel's tiles
@pytest.mark.parametrize("radius", [(2, 2, 1), (8, 8, 0), (9, 3, 1), (3, 9, 1), (32, 32, 1)], ids=str)
def test_windows_across_tile_seams(pkg, ctx, radius):
    """Tiles of 32 x 8 outputs (radii up to 8) and 16 x 8 (above): on a 70 x 20 x 3 volume both have seams inside the
    volume in x and in y, and every window of radius >= 1 next to one crosses it; the theta pass crosses layers.  Equal
    maxima sit on either side of the seams x = 32 | 16 and y = 8, once inside one window and once farther apart, over a
    background of three values and NaN that ties everywhere."""
    shape = (70, 20, 3)
    nx, ny, _ = shape
    rs = np.random.RandomState(radius[0] * 37 + radius[1])
    s = rs.choice([0.625, 0.75, 0.875, NAN], size=nx * ny, p=[0.4, 0.3, 0.2, 0.1])
    g = s.reshape(ny, nx)
    tx = 32 if max(radius[0], radius[1]) <= 8 else 16
    g[3, tx - 1] = g[3, tx + 1] = 0.9                      # across the x seam, two cells apart
    g[7, 50] = g[9, 50] = 0.9                              # across the y seam
    g[15, tx - 1] = g[15, tx + radius[0] + 1] = 0.9        # across the x seam, farther apart than the window (or clipped)
    m = pkg.Matcher(ctx, "BF", pkg.spe_cfg(), bf_params(shape))
    try:
        c, v = designed(ctx, "seams", shape, s)
        got = check(m, c, v, radius=radius, max_peaks=64)
        if radius[0] >= 2 and radius[1] >= 2:
            assert 3 * nx + tx - 1 in got["index"] and 3 * nx + tx + 1 not in got["index"]
            assert 7 * nx + 50 in got["index"] and 9 * nx + 50 not in got["index"]
        check(m, c, v, radius=radius, min_ratio=0.875 / 0.9, max_peaks=8192)
        check(m, c, v, radius=(radius[0], radius[1], 0), max_peaks=64)
    finally:
        m.close()


# ---- 3. real scores: the volume behind the peaks is the sweep's
def lattice(r9, centre):
    xs, ys, ts = bf_offsets(*r9[0:3], True), bf_offsets(*r9[3:6], True), bf_offsets(*r9[6:9], False)
    return (len(xs), len(ys), len(ts)), np.array([(centre[0] + x, centre[1] + y, centre[2] + t) for t in ts for y in ys for x in xs])


def upload_scene(pkg, ctx, sc, map_id=0):
    ctx.upload_map(map_id, sc["map"])
    cos_a, sin_a = pkg.beam_trig(sc["scan"].angle)
    ctx.scan_upload(sc["scan"].range, cos_a, sin_a, sc["scan"].weight, sc["scan"].factor)


CONFIGS = {"occ_point": (CELL_OCC, "even", {}), "occ_max": (CELL_OCC, "even", dict(oope=1, area=(-0.1, 0.1, -0.1, 0.1))),
           "tbm_viny": (CELL_TBM, "viny", {})}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_peaks_of_the_sweeps_own_scores(pkg, ctx, name):
    cell, weighting, kw = CONFIGS[name]
    sc = make_scene(cell_model=cell, size=400, scale=0.1, n_beams=360, seed=3, weighting=weighting)
    upload_scene(pkg, ctx, sc)
    cfg = lambda: pkg.spe_cfg(**kw)  # noqa: E731
    m, twin = pkg.Matcher(ctx, "BF", cfg(), R9), pkg.Matcher(ctx, "BF", cfg(), R9)
    try:
        centre = sc["init_pose"]
        shape, poses = lattice(R9, centre)
        # (the peaks are those of the canonical sums: the twin's tie check is off, so that its trace carries them whatever
        # comparisons its walk meets)
        twin.set_tie_check(False)
        t = twin.process_scan(0, centre, trace=True)
        assert t["n_calls"] == 1 + len(poses)
        np.testing.assert_array_equal(bits(t["poses"][1:]), bits(poses))
        volume = t["scores"][1:]
        np.testing.assert_array_equal(bits(volume), bits(ctx.score_poses(0, cfg(), poses)))
        for radius, ratio, floor, mp in [((1, 1, 1), 0.0, 0.0, 64), ((3, 3, 1), 0.97, 0.0, 16), ((2, 2, 2), 0.0, float(np.median(volume)), 4),
                                         ((0, 0, 0), 0.0, 0.0, 8)]:
            got = m.bf_peaks(0, centre, radius, ratio, floor, mp)
            want_i, want_s = numpy_peaks(volume, shape, radius, ratio, floor)
            assert got["shape"] == shape and got["n_found"] == len(want_i)
            k = min(mp, len(want_i))
            np.testing.assert_array_equal(got["index"], want_i[:k])
            np.testing.assert_array_equal(bits(got["scores"]), bits(want_s[:k]))
            np.testing.assert_array_equal(bits(got["poses"]), bits(poses[want_i[:k]].reshape(-1, 3)))
        assert not m.bf_peaks_stats()["on_shared_launch"]
    finally:
        mcb.close_all(m, twin)


# ---- 4. the matcher's own state
STAT_KEYS = ("scorer_calls", "poses_evaluated", "launches", "kernels_launched", "steps_rescored", "calls_closed_form")


def test_the_matchers_state_is_not_touched(pkg, ctx):
    sc = make_scene(cell_model=CELL_OCC, size=400, scale=0.1, n_beams=360, seed=3)
    upload_scene(pkg, ctx, sc)
    r9 = [-0.1, 0.1, 0.05, -0.1, 0.1, 0.05, -0.02, 0.02, 0.02]
    m, twin = pkg.Matcher(ctx, "BF", pkg.spe_cfg(), r9), pkg.Matcher(ctx, "BF", pkg.spe_cfg(), r9)
    try:
        scan = ctx.scan_download()

        def same_state():
            a, b = m.bf_stream_info(-1), twin.bf_stream_info(-1)
            assert a["base_set"] == b["base_set"] and a["matches"] == b["matches"]
            np.testing.assert_array_equal(a["base"], b["base"])
            sa, sb = m.stats(), twin.stats()
            assert [sa[k] for k in STAT_KEYS] == [sb[k] for k in STAT_KEYS]
            np.testing.assert_array_equal(ctx.scan_download(), scan)

        other = sc["init_pose"] + [0.3, -0.2, 0.1]
        m.bf_peaks(0, other, (1, 1, 1))
        same_state()
        assert not m.bf_stream_info(-1)["base_set"]
        for init in (sc["init_pose"], sc["init_pose"] + [0.02, 0.01, -0.01]):
            mcb.same_trace(m.process_scan(0, init, trace=True), twin.process_scan(0, init, trace=True))
            same_state()
            m.bf_peaks(0, other, (1, 1, 0), max_peaks=0)
            m.bf_peaks_batch([dict(map_id=0, range=[1.0], cos_a=[1.0], sin_a=[0.0], weight=[1.0], init_pose=other)] * 2)
            same_state()
    finally:
        mcb.close_all(m, twin)


# ---- 5. K jobs in one call
def batch_jobs(pkg, ctx):
    """four jobs over two maps with their own scans and centres; job 2's scan weighs nothing (tot_w 0: a NaN volume)"""
    jobs = [dict(j) for j in mcb.scenes(pkg, ctx, CELL_OCC, "even", 4)]
    jobs[2]["weight"] = np.zeros_like(jobs[2]["weight"])
    sent = []
    for k, j in enumerate(jobs):
        ctx.scan_store(60 + k, j["range"], j["cos_a"], j["sin_a"], j["weight"])
        sent.append(dict(map_id=j["map_id"], scan_slot=60 + k, init_pose=j["init_pose"]) if k % 2 else
                    dict(map_id=j["map_id"], range=j["range"], cos_a=j["cos_a"], sin_a=j["sin_a"], weight=j["weight"],
                         init_pose=j["init_pose"]))
    return jobs, sent


@pytest.mark.parametrize("name", ["occ_point", "occ_max"])
def test_batch_jobs_equal_lone_calls(pkg, ctx, name):
    _, _, kw = CONFIGS[name]
    jobs, sent = batch_jobs(pkg, ctx)
    r9 = [-0.2, 0.2, 0.05, -0.2, 0.2, 0.05, -0.06, 0.06, 0.02]
    m, lone = pkg.Matcher(ctx, "BF", pkg.spe_cfg(**kw), r9), pkg.Matcher(ctx, "BF", pkg.spe_cfg(**kw), r9)
    try:
        for radius, ratio, mp in [((1, 1, 1), 0.0, 16), ((2, 2, 0), 0.9, 3)]:
            got = m.bf_peaks_batch(sent, radius, ratio, 0.0, mp)
            st = m.bf_peaks_stats()
            assert st["on_shared_launch"] == (name == "occ_point")
            for k, (g, j) in enumerate(zip(got, jobs)):
                ctx.scan_select(60 + k)
                w = lone.bf_peaks(j["map_id"], j["init_pose"], radius, ratio, 0.0, mp)
                assert g["n_found"] == w["n_found"], k
                np.testing.assert_array_equal(g["index"], w["index"])
                np.testing.assert_array_equal(bits(g["scores"]), bits(w["scores"]))
                np.testing.assert_array_equal(bits(g["poses"]), bits(w["poses"]))
                assert (w["n_found"] == 0) == (k == 2), k
        if name == "occ_point":  # the launches of the shared route do not depend on K
            m.bf_peaks_batch(sent[:1], (1, 1, 1))
            one = m.bf_peaks_stats()
            assert one["on_shared_launch"] and one["launches"] == st["launches"] == 4
    finally:
        mcb.close_all(m, lone)


def test_launch_count_does_not_depend_on_the_shape(pkg, ctx):
    counts = []
    for shape in ((9, 7, 1), (64, 32, 5)):
        n = shape[0] * shape[1]
        c, v = designed(ctx, "count", shape, background(n, 17))
        m = pkg.Matcher(ctx, "BF", pkg.spe_cfg(), c.params)
        try:
            for radius in ((1, 1, 1), (32, 32, 2)):
                check(m, c, v, radius=radius)
                counts.append(m.bf_peaks_stats()["launches"])
        finally:
            m.close()
    assert counts == [5, 5, 5, 5]  # poses, scores, plane, theta + compaction, ordering


# ---- 6. refusals: nothing launched
def test_refusals_launch_nothing(pkg, ctx):
    shape = (9, 7, 1)
    c, v = designed(ctx, "refusals", shape, background(63, 19))
    m = pkg.Matcher(ctx, "BF", pkg.spe_cfg(), c.params)
    hc = pkg.Matcher(ctx, "HC", pkg.spe_cfg(), [6, 0.1, 0.1])
    wide = pkg.Matcher(ctx, "BF", pkg.spe_cfg(), bf_params((201, 201, 1)))
    unsupported = [pkg.Matcher(ctx, "BF", pkg.spe_cfg(**kw), c.params)
                   for kw in (dict(sum_order=pkg.SUM_SEQUENTIAL), dict(pose_trig=pkg.POSE_TRIG_HOST),
                              dict(pose_trig=pkg.POSE_TRIG_RAW_EXACT), dict(oope=pkg.OOPE_GMAPPING))]
    job = dict(map_id=0, range=[0.0], cos_a=[1.0], sin_a=[0.0], weight=[1.0], init_pose=c.inits[0])
    try:
        check(m, c, v)
        before = m.bf_peaks_stats()
        bad = [dict(radius=(-1, 0, 0)), dict(radius=(0, 0, 33)), dict(max_peaks=-1), dict(max_peaks=8193), dict(min_ratio=-0.5),
               dict(min_ratio=1.25), dict(min_ratio=NAN), dict(min_score=NAN)]
        for kw in bad:
            with pytest.raises(pkg.SlamHipError, match="slamhip error -1:"):
                m.bf_peaks(0, c.inits[0], **kw)
            with pytest.raises(pkg.SlamHipError, match="slamhip error -1:"):
                m.bf_peaks_batch([job, job], **kw)
        assert m.bf_peaks_stats() == before
        for call in (lambda x: x.bf_peaks(0, c.inits[0]), lambda x: x.bf_peaks_batch([job, job])):
            with pytest.raises(pkg.SlamHipError, match="slamhip error -1:"):  # not a brute-force matcher
                call(hc)
            for u in unsupported:
                with pytest.raises(pkg.SlamHipError, match="slamhip error -5:"):
                    call(u)
                assert u.bf_peaks_stats()["launches"] == 0
        for call in (lambda x: x.bf_peaks(0, c.inits[0], (0, 0, 0)), lambda x: x.bf_peaks_batch([job, job], (0, 0, 0))):
            with pytest.raises(pkg.SlamHipError, match="slamhip error -1:.*8192"):  # B = 40401 under radius 0
                call(wide)
        assert wide.bf_peaks_stats()["launches"] == 0
        with pytest.raises(pkg.SlamHipError, match="slamhip error -1:"):  # an unknown map
            m.bf_peaks(37, c.inits[0])
        assert m.bf_peaks_stats() == before
        check(m, c, v)  # ... and the matcher still answers
    finally:
        mcb.close_all(m, hc, wide, *unsupported)


def test_sweeps_too_large_are_refused(pkg, ctx):
    """A sweep above 2^26 poses is UNSUPPORTED, a batch whose K x (1 + nx ny nt) exceeds 2^24 INVALID: both before any
    scratch is asked for (the matcher's offsets alone are made: 2 x 8193 doubles)."""
    c, _ = designed(ctx, "large", (9, 7, 1), background(63, 23))
    huge = pkg.Matcher(ctx, "BF", pkg.spe_cfg(), bf_params((8193, 8193, 1)))  # 8193^2 = 2^26 + 16385
    wide = pkg.Matcher(ctx, "BF", pkg.spe_cfg(), bf_params((201, 201, 1)))
    job = dict(map_id=0, range=[0.0], cos_a=[1.0], sin_a=[0.0], weight=[1.0], init_pose=c.inits[0])
    try:
        for call in (lambda x: x.bf_peaks(0, c.inits[0], (32, 32, 0)), lambda x: x.bf_peaks_batch([job], (32, 32, 0))):
            with pytest.raises(pkg.SlamHipError, match="slamhip error -5:.*2\\^26"):
                call(huge)
        assert huge.bf_peaks_stats() == dict(launches=0, survivors_bound=0, on_shared_launch=False)
        k = 416  # 416 x 40402 = 2^24 + 30016; 415 x 40402 lies below
        assert k * 40402 > 1 << 24 > (k - 1) * 40402
        with pytest.raises(pkg.SlamHipError, match="slamhip error -1:.*2\\^24"):
            wide.bf_peaks_batch([job] * k, (3, 3, 0))
        assert wide.bf_peaks_stats() == dict(launches=0, survivors_bound=0, on_shared_launch=False)
    finally:
        mcb.close_all(huge, wide)


def test_null_arguments_are_refused(pkg, ctx):
    """Through the C-ABI itself (the Python wrappers always pass buffers): null centre, radius, n_written, n_found, jobs,
    and null peaks_out with max_peaks > 0 are SLAMHIP_ERR_INVALID, nothing launched; null peaks_out with max_peaks = 0 and a
    null shape_out go through."""
    import ctypes as C
    c, v = designed(ctx, "nulls", (9, 7, 1), background(63, 29))
    m = pkg.Matcher(ctx, "BF", pkg.spe_cfg(), c.params)
    try:
        check(m, c, v)
        before = m.bf_peaks_stats()
        L = ctx.L
        c3, rad = (C.c_double * 3)(*c.inits[0]), (C.c_int * 3)(1, 1, 1)
        buf, nw, nf, shape = (pkg.BfPeak * 4)(), C.c_int(), C.c_longlong(), (C.c_int * 3)()
        lone = dict(centre=c3, radius=rad, peaks_out=buf, n_written=C.byref(nw), n_found=C.byref(nf), shape_out=shape)

        def call_lone(max_peaks=4, **kw):
            a = dict(lone, **kw)
            return L.slamhip_matcher_bf_peaks(m.h, 0, a["centre"], a["radius"], 0.0, 0.0, max_peaks, a["peaks_out"], a["n_written"],
                                              a["n_found"], a["shape_out"])

        assert L.slamhip_matcher_bf_peaks(None, 0, c3, rad, 0.0, 0.0, 4, buf, C.byref(nw), C.byref(nf), shape) == -1
        for name in ("centre", "radius", "peaks_out", "n_written", "n_found"):
            assert call_lone(**{name: None}) == -1, name
        assert m.bf_peaks_stats() == before
        assert call_lone(max_peaks=0, peaks_out=None, shape_out=None) == 0 and nw.value == 0 and nf.value >= 1
        blk = m.make_batch([dict(map_id=0, range=[0.0], cos_a=[1.0], sin_a=[0.0], weight=[1.0], init_pose=c.inits[0])] * 2)
        bbuf, bnw, bnf = (pkg.BfPeak * 8)(), (C.c_int * 2)(), (C.c_longlong * 2)()
        batch = dict(jobs=blk["arr"], radius=rad, peaks_out=bbuf, n_written=bnw, n_found=bnf)

        def call_batch(max_peaks=4, **kw):
            a = dict(batch, **kw)
            return L.slamhip_matcher_bf_peaks_batch(m.h, 2, a["jobs"], a["radius"], 0.0, 0.0, max_peaks, a["peaks_out"],
                                                    a["n_written"], a["n_found"])

        before = m.bf_peaks_stats()
        assert L.slamhip_matcher_bf_peaks_batch(None, 2, blk["arr"], rad, 0.0, 0.0, 4, bbuf, bnw, bnf) == -1
        assert L.slamhip_matcher_bf_peaks_batch(m.h, -1, blk["arr"], rad, 0.0, 0.0, 4, bbuf, bnw, bnf) == -1
        for name in ("jobs", "radius", "peaks_out", "n_written", "n_found"):
            assert call_batch(**{name: None}) == -1, name
        assert m.bf_peaks_stats() == before
        assert call_batch() == 0 and call_batch(max_peaks=0, peaks_out=None) == 0 and list(bnw) == [0, 0]
        assert L.slamhip_matcher_bf_peaks_stats(None, None, None, None) == -1
        assert L.slamhip_matcher_bf_peaks_stats(m.h, None, None, None) == 0
    finally:
        m.close()


# ---- 7. far from the origin
def test_far_from_the_origin(pkg, ctx):
    sc = ps.place("Q3", size=240, scale=0.1, n_beams=360)  # 10007 and 20011 cells out
    upload_scene(pkg, ctx, sc)
    r9 = [-0.2, 0.2, 0.05, -0.15, 0.15, 0.05, -0.04, 0.04, 0.02]
    m = pkg.Matcher(ctx, "BF", pkg.spe_cfg(), r9)
    try:
        centre = sc["init_pose"]
        shape, poses = lattice(r9, centre)
        volume = ctx.score_poses(0, pkg.spe_cfg(), poses)
        for radius in ((1, 1, 1), (2, 1, 0)):
            got = m.bf_peaks(0, centre, radius, 0.5, 0.0, 32)
            want_i, want_s = numpy_peaks(volume, shape, radius, 0.5, 0.0)
            assert got["shape"] == shape and got["n_found"] == len(want_i) >= 1
            np.testing.assert_array_equal(got["index"], want_i[:32])
            np.testing.assert_array_equal(bits(got["scores"]), bits(want_s[:32]))
            np.testing.assert_array_equal(bits(got["poses"]), bits(poses[want_i[:32]].reshape(-1, 3)))
    finally:
        m.close()
