"""GPU suite: slamhip_map_append_scan_batch -- K scans into K resident maps through shared launches of the gather
kernels (k_mu_lines_batch / k_mu_cells_batch, csrc/map_update_gather.h).

The contract: after the call every map holds bit for bit what the same jobs leave behind when they go through the lone
entry point one after another in job order.  So the expected value of nearly everything here is a second set of
identically bound maps updated by Context.map_append_scan / map_append_scan_raw; the first test holds the batch to the
compiled reference's golden (tests/golden/map_update_oblong.npz) at the bars of test_gpu_mapupdate_oblong.py.
Every window has width != height, origin_x != origin_y and a width that is no multiple of 16.

The golden's three steps differ in blur and max_range, which are adder settings: a round that holds step k on one map
and step k - 1 on another needs them per job (slamhip_map_update_job::cfg; the Python wrapper fills it for a job that
names blur / max_range / base)."""
import numpy as np
import pytest
from mapupdate_oblong_cases import (AUX_STRIDE, MODELS, RUN_IDS, RUNS, STRIDE, UNKNOWN, fresh_map, geometry, golden,
                                    oracle_step, step_args, tag)

import __graft_entry__ as ge

pytestmark = pytest.mark.gpu

SCALE = 0.1
AUX = AUX_STRIDE
RIM_W, RIM_H, RIM_ORIGIN = 77, 45, (9, 31)
ERR_STATE = -4
GATED = 50.0  # a range beyond every max_range used here
ANG_A = np.deg2rad(np.linspace(-177.0, 177.0, 360))  # scanner A: 360 beams, nearly a full turn
ANG_B = np.deg2rad(np.linspace(-135.0, 135.0, 181))  # scanner B: 181 beams, 1.5 degrees apart: 0, 45 and 90 degrees among them


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
    return v


@pytest.fixture(autouse=True)
def _defaults(pkg, ctx):
    yield
    ctx.set_option(pkg.OPT_K6_PATH, 0)
    ctx.map_set_deferred(False)


def bind_fresh(pkg, ctx, map_id, cell_model, w, h, origin, grow=False):
    try:
        ctx.map_release(map_id)
    except pkg.SlamHipError:
        pass  # (nothing bound under this id)
    assert w != h and origin[0] != origin[1] and w % 16
    ctx.map_bind(map_id, cell_model, w, h, origin, SCALE, UNKNOWN[cell_model])
    if grow:
        ctx.map_set_auto_grow(map_id, True)


def adder(est):
    return dict(estimator=1, shift_amount=0.01 * SCALE) if est else {}


def lone(ctx, rule, job, map_id, **kw):
    """the job through the lone entry point, on map map_id"""
    kw = dict(kw)
    for key in ("blur", "max_range", "base"):
        if key in job:
            kw[key] = job[key]
    if job.get("angle") is not None:
        return ctx.map_append_scan_raw(map_id, rule, job["pose"], job["range"], job["angle"], job.get("is_occ"),
                                       quality=job.get("quality", 1.0), beam_quality=job.get("beam_quality"), **kw)
    return ctx.map_append_scan(map_id, rule, job["pose"], job["range"], job["cos_a"], job["sin_a"], job.get("is_occ"),
                               quality=job.get("quality", 1.0), beam_quality=job.get("beam_quality"), **kw)


def same_maps(ctx, a, b, cell_model, rule, msg=""):
    """payload, counters and geometry of maps a and b: equal"""
    ia, ib = ctx.map_info(a), ctx.map_info(b)
    assert ia == ib, msg
    w, h = ia["width"], ia["height"]
    np.testing.assert_array_equal(ctx.map_download_window(a, 0, 0, w, h, STRIDE[cell_model]),
                                  ctx.map_download_window(b, 0, 0, w, h, STRIDE[cell_model]), err_msg=msg)
    if rule in AUX:
        np.testing.assert_array_equal(ctx.map_download_aux(a, 0, 0, w, h, AUX[rule]),
                                      ctx.map_download_aux(b, 0, 0, w, h, AUX[rule]), err_msg=msg)


def job_on(pkg, map_id, pose, ang, rng, seed, **more):
    c, s = pkg.beam_trig(ang)
    occ = (np.random.RandomState(seed).rand(ang.size) < 0.8).astype(np.int32)
    return dict(map_id=map_id, pose=np.asarray(pose, dtype=np.float64), range=np.asarray(rng, dtype=np.float64), cos_a=c, sin_a=s,
                is_occ=occ, **more)


def inside_scan(seed, ang=ANG_B, lo=0.4, hi=2.0):
    return np.random.RandomState(seed).uniform(lo, hi, ang.size)


RIM_MID = (2.93, -0.87)  # metres: the middle of the 77 x 45 window with origin (9, 31)


# ---- 1. the reference's golden, two maps per call ----------------------------------------------------------------------
def _golden_through_the_batch(pkg, ctx, oracle, name, est, raw):
    g = golden()
    cell_model, rule = MODELS[name]
    st = STRIDE[cell_model]
    n_steps = int(g["n_steps"])
    ids = {"full": 2, "crop": 3}
    boxes, oracles = {}, {}
    for window, mid in ids.items():
        w, h, origin = geometry(g, name, window)
        try:
            ctx.map_release(mid)
        except pkg.SlamHipError:
            pass
        assert w != h and origin[0] != origin[1] and w % 16
        ctx.map_bind(mid, cell_model, w, h, origin, float(g["scale"]), g[name + "_unknown"][:st])
        boxes[window] = [int(v) for v in g["crop"]] if window == "full" else (0, 0, w, h)
        oracles[window] = fresh_map(g, name, window)

    def job(window, k):
        kw, ex = step_args(g, name, est, k)
        j = dict(map_id=ids[window], pose=g["step%d_pose" % k], range=g["step%d_range" % k], is_occ=g["step%d_occ" % k],
                 quality=kw["quality"], blur=kw["blur"], max_range=kw["max_range"], base=kw["base"])
        if raw:
            j["angle"] = g["step%d_angle" % k]
        else:
            j["cos_a"], j["sin_a"] = pkg.beam_trig(g["step%d_angle" % k])
        return j

    shift = dict(estimator=1, shift_amount=float(g["shift_amount"])) if est else {}
    shared_calls = 0
    for call in range(n_steps + 1):  # the crop map runs one step behind the full map
        todo = ([("full", call)] if call < n_steps else []) + ([("crop", call - 1)] if call >= 1 else [])
        nu, status = ctx.map_append_scan_batch(rule, [job(w_, k) for w_, k in todo], **shift)
        assert not status.any()
        stats = ctx.map_update_batch_stats()
        if len(todo) == 2:
            assert (stats["rounds"], stats["jobs_shared"], stats["jobs_lone"], stats["launches"]) == (1, 2, 0, 3), stats
            shared_calls += 1
        else:
            assert (stats["rounds"], stats["jobs_shared"], stats["jobs_lone"]) == (0, 0, 1), stats
        for i, (window, k) in enumerate(todo):
            m, aux, _ = oracles[window]
            assert nu[i] == oracle_step(oracle, g, name, est, k, m, aux, rule) > 1000
            x0, y0, x1, y1 = boxes[window]
            got = ctx.map_download_window(ids[window], x0, y0, x1 - x0, y1 - y0, st)
            want = g[tag(name, est, k) + "payload"]
            msg = "%s %s step %d" % (name, window, k)
            if raw:
                np.testing.assert_array_equal(got, want, err_msg=msg)
            elif est:
                np.testing.assert_allclose(got, want, rtol=1e-11, atol=1e-13, err_msg=msg)
            elif name == "gmapping":
                np.testing.assert_array_equal(got[..., 0], want[..., 0], err_msg=msg)
                np.testing.assert_allclose(got[..., 1:], want[..., 1:], rtol=1e-13, atol=1e-15, err_msg=msg)  # obstacle means
            else:
                np.testing.assert_array_equal(got, want, err_msg=msg)
            if rule in AUX:
                np.testing.assert_array_equal(ctx.map_download_aux(ids[window], x0, y0, x1 - x0, y1 - y0, AUX[rule]),
                                              g[tag(name, est, k) + "aux"], err_msg=msg)
    assert shared_calls == n_steps - 1 >= 2
    # nothing outside the crop box of the full window
    w, h, _ = geometry(g, name, "full")
    x0, y0, x1, y1 = boxes["full"]
    whole = ctx.map_download_window(2, 0, 0, w, h, st)
    outside = np.ones((h, w), bool)
    outside[y0:y1, x0:x1] = False
    assert (whole[outside] == g[name + "_unknown"][:st]).all()
    for mid in ids.values():
        ctx.map_release(mid)


@pytest.mark.parametrize("name,est", RUNS, ids=RUN_IDS)
def test_batch_of_two_maps_vs_reference_golden_raw_provider_bit_for_bit(pkg, ctx, oracle, variant, name, est):
    """`angle` jobs (the reference's own cos / sin(theta + a)): assert_array_equal against the golden throughout."""
    _golden_through_the_batch(pkg, ctx, oracle, name, est, raw=True)


@pytest.mark.parametrize("name,est", RUNS, ids=RUN_IDS)
def test_batch_of_two_maps_vs_reference_golden_cached_provider(pkg, ctx, oracle, name, est):
    """cos_a / sin_a jobs at test_gpu_mapupdate_oblong.py's bars: const estimator bit for bit but GMapping's obstacle
    means (1e-13), area estimator 1e-11, counters and update counts exact."""
    _golden_through_the_batch(pkg, ctx, oracle, name, est, raw=False)


# ---- 2. batch = lone, bit for bit --------------------------------------------------------------------------------------
def _centre(cell):
    return (cell + 0.5) * SCALE


def five_jobs(pkg, ids, batch_no):
    """Five jobs on the five maps of five_maps(): 37, 90, 181, 1 and 360 ray-traced beams (the others lie beyond
    max_range) of scanners A, B, B, B, A; poses in all four quadrants; job 2 from a cell centre with all of B's beams,
    among them 0, 90 and 45 degrees (axis-parallel beams and a diagonal through grid vertices: irregular beams, and the
    cells around the robot are visited by several of them)."""
    rs = np.random.RandomState(100 + batch_no)
    d = 0.013 * batch_no  # the poses move a little from batch to batch (job 2 stays on its cell centre)

    def gated(ang, n_in, lo, hi):
        rng = np.full(ang.size, GATED)
        keep = rs.permutation(ang.size)[:n_in]
        rng[keep] = rs.uniform(lo, hi, n_in)
        return rng
    jobs = []
    # 77 x 45 at (9, 31): x > 0, y < 0
    jobs.append(job_on(pkg, ids[0], [3.4 + d, -1.2 - d, 0.7], ANG_A, gated(ANG_A, 37, 0.3, 1.0), 1 + batch_no, quality=0.9))
    # 60 x 40 at (-13, 42): x > 0, y < 0 (the window holds nothing else)
    jobs.append(job_on(pkg, ids[1], [4.2 - d, -2.2 + d, 2.0], ANG_B, gated(ANG_B, 90, 0.3, 1.0), 2 + batch_no, quality=0.8))
    # 203 x 131 at (101, 65): x < 0, y > 0, exactly on the centre of cell (-11, 5), heading 0
    rng = rs.uniform(1.0, 4.0, ANG_B.size)
    rng[90], rng[150] = 2.5 + batch_no * SCALE, 1.7  # 0 and 90 degrees: along the row and the column of the robot's cell
    rng[120] = (14 + batch_no) * SCALE * np.sqrt(2.0)  # 45 degrees: through the vertices
    rng[60] = 9 * SCALE * np.sqrt(2.0)  # -45 degrees
    jobs.append(job_on(pkg, ids[2], [_centre(-11), _centre(5), 0.0], ANG_B, rng, 3 + batch_no, quality=1.0))
    # 47 x 1 at (10, 0): one cell high; x > 0, y > 0; the one beam in range runs along +x
    rng = np.full(ANG_B.size, GATED)
    rng[90] = 2.2 + batch_no * SCALE
    jobs.append(job_on(pkg, ids[3], [_centre(5), 0.05, 0.0], ANG_B, rng, 4 + batch_no, quality=0.7))
    # grows from 21 x 13 at (3, 10): x < 0, y < 0, all of A's beams
    jobs.append(job_on(pkg, ids[4], [-0.33 - 7 * d, -0.41 - 9 * d, -2.5], ANG_A, rs.uniform(1.0, 3.0 + batch_no, ANG_A.size),
                       5 + batch_no, quality=0.85))
    return jobs


def five_maps(pkg, ctx, cell_model, first_id):
    ids = list(range(first_id, first_id + 5))
    bind_fresh(pkg, ctx, ids[0], cell_model, RIM_W, RIM_H, RIM_ORIGIN)
    bind_fresh(pkg, ctx, ids[1], cell_model, 60, 40, (-13, 42))
    bind_fresh(pkg, ctx, ids[2], cell_model, 203, 131, (101, 65))
    bind_fresh(pkg, ctx, ids[3], cell_model, 47, 1, (10, 0))
    bind_fresh(pkg, ctx, ids[4], cell_model, 21, 13, (3, 10), grow=True)
    return ids


@pytest.mark.parametrize("name,est", RUNS, ids=RUN_IDS)
def test_five_maps_in_one_call_equal_the_lone_calls_bit_for_bit(pkg, name, est):
    cell_model, rule = MODELS[name]
    ctx = pkg.Context(0)  # (its own context: the count of direction tables starts from zero)
    try:
        batch_ids, lone_ids = five_maps(pkg, ctx, cell_model, 10), five_maps(pkg, ctx, cell_model, 20)
        kw = dict(blur=0.3, max_range=6.0, **adder(est))
        cfg = pkg.spe_cfg(oope=pkg.OOPE_GMAPPING) if name == "gmapping" else pkg.spe_cfg()
        cs, sn = pkg.beam_trig(ANG_B[::2])
        ctx.scan_upload(inside_scan(77, ANG_B[::2], 0.5, 3.0), cs, sn, np.ones(cs.size))
        rs = np.random.RandomState(9)
        uploads = None
        for batch_no in range(3):
            jobs = five_jobs(pkg, batch_ids, batch_no)
            counts = [int(np.count_nonzero(j["range"] < 6.0)) for j in jobs]
            assert counts == [37, 90, 181, 1, 360]
            nu, status = ctx.map_append_scan_batch(rule, jobs, **kw)
            stats = ctx.map_update_batch_stats()
            assert not status.any()
            assert (stats["rounds"], stats["jobs_shared"], stats["jobs_lone"], stats["launches"]) == (1, 5, 0, 3), stats
            assert stats["tables"] == 2  # two scanners
            if batch_no == 0:
                assert stats["table_uploads"] == 2
                uploads = stats["table_uploads"]
            assert stats["table_uploads"] == uploads  # a later call with the same scanners uploads none
            for k, j in enumerate(jobs):
                msg = "batch %d job %d" % (batch_no, k)
                assert nu[k] == lone(ctx, rule, j, lone_ids[k], **kw) > 0, msg
                same_maps(ctx, batch_ids[k], lone_ids[k], cell_model, rule, msg)
                # the scorer in its default mode reads the TBM probability plane / the GMapping neighbourhood masks
                # the updates keep: 16 poses around the job's
                poses = j["pose"] + rs.randn(16, 3) * [0.15, 0.15, 0.1]
                if name == "gmapping":
                    ctx.gm_cache_reset()
                a = ctx.score_poses(batch_ids[k], cfg, poses)
                if name == "gmapping":
                    ctx.gm_cache_reset()
                b = ctx.score_poses(lone_ids[k], cfg, poses)
                np.testing.assert_array_equal(a, b, err_msg=msg)
        grown = ctx.map_info(batch_ids[4])
        assert grown["times_grown"] >= 1 and grown["width"] > 21 and grown["height"] > 13
        one_high = ctx.map_download_window(batch_ids[3], 0, 0, 47, 1, STRIDE[cell_model])
        assert np.count_nonzero((one_high != UNKNOWN[cell_model]).any(axis=2)) >= 22
    finally:
        ctx.close()


# ---- 3 .. 7 on 77 x 45 windows ------------------------------------------------------------------------------------------
def rim_maps(pkg, ctx, cell_model, ids):
    for mid in ids:
        bind_fresh(pkg, ctx, mid, cell_model, RIM_W, RIM_H, RIM_ORIGIN)


def plain_job(pkg, map_id, seed, **more):
    rs = np.random.RandomState(seed)
    pose = [RIM_MID[0] + rs.uniform(-0.3, 0.3), RIM_MID[1] + rs.uniform(-0.2, 0.2), rs.uniform(-3.0, 3.0)]
    return job_on(pkg, map_id, pose, ANG_B, inside_scan(seed + 1000), seed, quality=0.9, **more)


THREE = ["mean", "tbm", "gmapping"]


@pytest.mark.parametrize("est", [0, 1], ids=["const", "area"])
@pytest.mark.parametrize("name", THREE)
def test_two_jobs_on_one_map_keep_job_order(pkg, ctx, name, est):
    """K = 3, jobs 0 and 2 on one map: two rounds, and the map holds what three lone calls in order leave."""
    cell_model, rule = MODELS[name]
    rim_maps(pkg, ctx, cell_model, [10, 11, 20, 21])
    kw = dict(blur=0.3, **adder(est))
    jobs = [plain_job(pkg, 10, 1), plain_job(pkg, 11, 2), plain_job(pkg, 10, 3)]
    jobs[2]["pose"] = jobs[0]["pose"] + [0.04, -0.03, 0.2]  # (the second scan of the map overlaps the first)
    nu, status = ctx.map_append_scan_batch(rule, jobs, **kw)
    stats = ctx.map_update_batch_stats()
    assert (stats["rounds"], stats["jobs_shared"], stats["jobs_lone"], stats["launches"]) == (2, 3, 0, 6), stats
    assert not status.any()
    for k, j in enumerate(jobs):
        assert nu[k] == lone(ctx, rule, j, j["map_id"] + 10, **kw) > 0
    same_maps(ctx, 10, 20, cell_model, rule)
    same_maps(ctx, 11, 21, cell_model, rule)


@pytest.mark.parametrize("name", THREE)
def test_jobs_the_launches_do_not_cover_go_through_the_lone_call(pkg, ctx, name):
    cell_model, rule = MODELS[name]
    kw = dict(blur=0.3)
    # a. beam directions that descend: that job alone
    rim_maps(pkg, ctx, cell_model, [10, 11, 12, 20, 21, 22])
    jobs = [plain_job(pkg, 10, 1), plain_job(pkg, 11, 2), plain_job(pkg, 12, 3)]
    for key in ("range", "cos_a", "sin_a", "is_occ"):
        jobs[1][key] = jobs[1][key][::-1].copy()
    nu, status = ctx.map_append_scan_batch(rule, jobs, **kw)
    stats = ctx.map_update_batch_stats()
    assert (stats["rounds"], stats["jobs_shared"], stats["jobs_lone"]) == (1, 2, 1), stats
    for k, j in enumerate(jobs):
        assert nu[k] == lone(ctx, rule, j, 20 + k, **kw) > 0
        same_maps(ctx, 10 + k, 20 + k, cell_model, rule, "descending, job %d" % k)
    # b. the record pipelines: the whole batch
    for path in (1, 2):
        ctx.set_option(pkg.OPT_K6_PATH, path)
        jobs = [plain_job(pkg, 10 + k, 10 * path + k) for k in range(3)]
        nu, status = ctx.map_append_scan_batch(rule, jobs, **kw)
        stats = ctx.map_update_batch_stats()
        assert (stats["rounds"], stats["jobs_shared"], stats["jobs_lone"], stats["launches"]) == (0, 0, 3, 0), stats
        for k, j in enumerate(jobs):
            assert nu[k] == lone(ctx, rule, j, 20 + k, **kw) > 0
            same_maps(ctx, 10 + k, 20 + k, cell_model, rule, "path %d, job %d" % (path, k))
    ctx.set_option(pkg.OPT_K6_PATH, 0)
    # c. a batch of one
    j = plain_job(pkg, 10, 77)
    nu, status = ctx.map_append_scan_batch(rule, [j], **kw)
    stats = ctx.map_update_batch_stats()
    assert (stats["rounds"], stats["jobs_shared"], stats["jobs_lone"]) == (0, 0, 1), stats
    assert nu[0] == lone(ctx, rule, j, 20, **kw) > 0
    same_maps(ctx, 10, 20, cell_model, rule, "one job")
    # ... and none
    nu, status = ctx.map_append_scan_batch(rule, [], **kw)
    assert nu.size == 0 and status.size == 0


@pytest.mark.parametrize("name", THREE)
def test_empty_jobs_take_no_part(pkg, ctx, name):
    """n = 0 and a scan whose beams all lie beyond max_range: 0 updates, maps untouched, the neighbours complete."""
    cell_model, rule = MODELS[name]
    rim_maps(pkg, ctx, cell_model, [10, 11, 12, 13, 20, 23])
    kw = dict(blur=0.3, max_range=6.0)
    jobs = [plain_job(pkg, 10, 1), plain_job(pkg, 11, 2), plain_job(pkg, 12, 3), plain_job(pkg, 13, 4)]
    for key in ("range", "cos_a", "sin_a", "is_occ"):
        jobs[1][key] = jobs[1][key][:0].copy()
    jobs[2]["range"] = np.full(ANG_B.size, GATED)
    nu, status = ctx.map_append_scan_batch(rule, jobs, **kw)
    stats = ctx.map_update_batch_stats()
    assert (stats["rounds"], stats["jobs_shared"], stats["jobs_lone"]) == (1, 2, 0), stats
    assert nu[1] == 0 and nu[2] == 0 and not status.any()
    for mid in (11, 12):
        assert (ctx.map_download_window(mid, 0, 0, RIM_W, RIM_H, STRIDE[cell_model]) == UNKNOWN[cell_model]).all()
    assert nu[0] == lone(ctx, rule, jobs[0], 20, **kw) > 0 and nu[3] == lone(ctx, rule, jobs[3], 23, **kw) > 0
    same_maps(ctx, 10, 20, cell_model, rule)
    same_maps(ctx, 13, 23, cell_model, rule)


def rim_placements():
    """test_gpu_mapupdate_oblong.py case c: internal robot cells two cells inside each rim and each corner"""
    lo, hx, hy, mx, my = 2, RIM_W - 3, RIM_H - 3, RIM_W // 2, RIM_H // 2
    return {"left": (lo, my), "right": (hx, my), "bottom": (mx, lo), "top": (mx, hy),
            "bottom-left": (lo, lo), "bottom-right": (hx, lo), "top-left": (lo, hy), "top-right": (hx, hy)}


@pytest.mark.parametrize("name", THREE)
def test_a_beam_that_leaves_a_fixed_window_fails_its_job_alone(pkg, ctx, name):
    cell_model, rule = MODELS[name]
    kw = dict(blur=0.3)
    rs = np.random.RandomState(41)
    ang = np.deg2rad(np.linspace(-180.0, 180.0, 64, endpoint=False))
    for where, (rx, ry) in rim_placements().items():
        rim_maps(pkg, ctx, cell_model, [10, 11, 12, 20, 21, 22])
        pose = np.array([(rx - RIM_ORIGIN[0] + 0.37) * SCALE, (ry - RIM_ORIGIN[1] + 0.61) * SCALE, 0.3])
        rng = rs.uniform(0.3, 3.0, ang.size)
        ex = np.floor((pose[0] + rng * np.cos(ang + pose[2])) / SCALE) + RIM_ORIGIN[0]
        ey = np.floor((pose[1] + rng * np.sin(ang + pose[2])) / SCALE) + RIM_ORIGIN[1]
        n_in = np.count_nonzero((ex >= 0) & (ex < RIM_W) & (ey >= 0) & (ey < RIM_H))
        assert 8 <= n_in <= ang.size - 8, where  # some beams stay inside, some cross
        jobs = [plain_job(pkg, 10, 1), job_on(pkg, 11, pose, ang, rng, 5, quality=0.9), plain_job(pkg, 12, 3)]
        with pytest.raises(pkg.SlamHipError, match=r"slamhip error -4: .*a beam leaves the bound map window") as info:
            ctx.map_append_scan_batch(rule, jobs, **kw)
        assert list(info.value.status) == [0, ERR_STATE, 0], where
        stats = ctx.map_update_batch_stats()
        assert (stats["rounds"], stats["jobs_shared"], stats["jobs_lone"]) == (1, 3, 0), stats
        assert info.value.n_updates[0] == lone(ctx, rule, jobs[0], 20, **kw) > 0
        with pytest.raises(pkg.SlamHipError, match=r"slamhip error -4: .*a beam leaves the bound map window"):
            lone(ctx, rule, jobs[1], 21, **kw)
        assert info.value.n_updates[2] == lone(ctx, rule, jobs[2], 22, **kw) > 0
        for k in range(3):
            same_maps(ctx, 10 + k, 20 + k, cell_model, rule, "%s, job %d" % (where, k))
    # the rule against the cell model of the LAST job's map: found before anything is launched
    other = "tbm" if name != "tbm" else "mean"
    bind_fresh(pkg, ctx, 13, MODELS[other][0], RIM_W, RIM_H, RIM_ORIGIN)
    before = [ctx.map_download_window(mid, 0, 0, RIM_W, RIM_H, STRIDE[cell_model]) for mid in (10, 11)]
    jobs = [plain_job(pkg, 10, 7), plain_job(pkg, 11, 8), plain_job(pkg, 13, 9)]
    with pytest.raises(pkg.SlamHipError, match="does not fit the map's payload model"):
        ctx.map_append_scan_batch(rule, jobs, **kw)
    for mid, was in zip((10, 11), before):
        np.testing.assert_array_equal(ctx.map_download_window(mid, 0, 0, RIM_W, RIM_H, STRIDE[cell_model]), was)
    assert (ctx.map_download_window(13, 0, 0, RIM_W, RIM_H, STRIDE[MODELS[other][0]]) == UNKNOWN[MODELS[other][0]]).all()


@pytest.mark.parametrize("name", THREE)
def test_a_batch_runs_behind_queued_lone_updates_and_leaves_them_queued(pkg, ctx, name):
    cell_model, rule = MODELS[name]
    rim_maps(pkg, ctx, cell_model, [10, 11, 20, 21])
    kw = dict(blur=0.3)
    first, second = plain_job(pkg, 10, 1), plain_job(pkg, 10, 2)
    jobs = [plain_job(pkg, 10, 3), plain_job(pkg, 11, 4)]
    # the expected maps and counts: awaited lone calls in order
    want = [lone(ctx, rule, first, 20, **kw), lone(ctx, rule, second, 20, **kw),
            lone(ctx, rule, jobs[0], 20, **kw), lone(ctx, rule, jobs[1], 21, **kw)]
    ctx.map_set_deferred(True)
    assert lone(ctx, rule, first, 10, **kw) == -1 and lone(ctx, rule, second, 10, **kw) == -1
    nu, status = ctx.map_append_scan_batch(rule, jobs, **kw)
    stats = ctx.map_update_batch_stats()
    assert (stats["rounds"], stats["jobs_shared"], stats["jobs_lone"]) == (1, 2, 0), stats
    assert list(nu) == want[2:] and not status.any()
    assert ctx.map_drain() == want[0] + want[1]  # the two queued updates alone
    ctx.map_set_deferred(False)
    same_maps(ctx, 10, 20, cell_model, rule)
    same_maps(ctx, 11, 21, cell_model, rule)
