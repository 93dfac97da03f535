"""GPU suite (-m gpu): slamhip_score_poses_batch -- the pose sets of K jobs, each over its own map and scan, in one
scoring launch (csrc/score_batch.hip; the planning: csrc/score_batch_plan.h).

References and bars:
  * the compiled reference's goldens (tests/golden/scene_*.npz, tests/golden/window_oope.npz): beam-order sum + host
    pose trig (or SLAMHIP_POSE_TRIG_RAW_EXACT behind the raw provider) bit-equal; default mode 1e-12 relative, the bar
    of tests/test_gpu_parity.py;
  * everywhere else the lone call -- scan_select of the job's slot, score_poses of its map and poses -- bit for bit:
    a job's scores depend neither on the route, nor on the other jobs, nor on the poses a workgroup takes."""
import types

import numpy as np
import pytest
import placed_scenes
from helpers import SCENES, filtered_scan, load, map_from
from synth import CELL_GMAPPING, CELL_OCC, CELL_TBM, make_scene, viny_weights
from window_oope_cases import OOPES, SCAN_SIZES, TRIGS, golden_map, golden_scan, load_golden

import __graft_entry__ as ge

pytestmark = pytest.mark.gpu

STRICT = dict(sum_order=1, pose_trig=1)  # SLAMHIP_SUM_SEQUENTIAL, SLAMHIP_POSE_TRIG_HOST
DEFAULT_RTOL = 1e-12
CELL_CREDIBILIST = 3
OBLONG = (-0.12, 0.05, -0.03, 0.21)  # (bot, top, left, right): off-centre, wider than high


@pytest.fixture(scope="module")
def pkg():
    return ge.load_package()


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_bits_equal(got, want, msg=""):
    """bit for bit, NaN payloads included"""
    assert len(got) == len(want), msg
    for k, (g, w) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(bits(g), bits(w), err_msg="%s job %d" % (msg, k))


def scan_arrays(pkg, scan):
    """(range, cos, sin, weight, factor) of a ScanData / synth.Scan as the tests upload it: the table's entries behind a
    cached provider, libm's behind the raw one"""
    if getattr(scan, "trig_mode", 0) == 1:
        idx = np.round((scan.angle - scan.a_min) / scan.a_delta).astype(np.int64)
        cos_a, sin_a = scan.tab_cos[idx], scan.tab_sin[idx]
    else:
        cos_a, sin_a = pkg.beam_trig(scan.angle)
    return scan.range, cos_a, sin_a, scan.weight, scan.factor


def lone_scores(ctx, cfg, jobs, current=None):
    """every job through the lone call: scan_select of its slot (slot -1: `current`, uploaded anew) + score_poses; the
    current scan is `current` again afterwards"""
    out = []
    for map_id, slot, poses in jobs:
        poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
        if len(poses) == 0:
            out.append(np.zeros(0))
            continue
        if slot < 0:
            ctx.scan_upload(*current)
        else:
            ctx.scan_select(slot)
        out.append(ctx.score_poses(map_id, cfg, poses))
    if current is not None:
        ctx.scan_upload(*current)
    return out


def random_map(pkg, kind, w, h, origin, scale, seed):
    """a window of w x h cells whose every cell differs: occupancies, or (u, e, o, c) beliefs"""
    rs = np.random.RandomState(seed)
    if kind == CELL_OCC:
        return types.SimpleNamespace(cell_model=CELL_OCC, payload=rs.rand(h, w, 1), width=w, height=h, origin=origin, scale=scale,
                                     unknown=np.array([0.5, 0, 0, 0]))
    m = rs.rand(h, w, 4) + 0.05
    m[..., 3] *= 0.2
    m /= m.sum(axis=2, keepdims=True)
    return types.SimpleNamespace(cell_model=kind, payload=m, width=w, height=h, origin=origin, scale=scale,
                                 unknown=np.array([1.0, 0, 0, 0]))


def random_scan(pkg, n, reach, weighting, seed):
    rs = np.random.RandomState(seed)
    rng, ang = rs.uniform(0.05, reach, n), np.sort(rs.uniform(-2.3, 2.3, n))
    w = np.full(n, 1.0 / n) if weighting == "even" else viny_weights(rng, ang)
    f = np.where(rs.rand(n) < 0.2, rs.rand(n), 1.0)
    return (rng,) + tuple(pkg.beam_trig(ang)) + (w, f)


def poses_in(m, n, seed, margin=0.6):
    """n poses over the window and a margin around it: some beams end outside"""
    rs = np.random.RandomState(seed)
    x0, y0 = -m.origin[0] * m.scale, -m.origin[1] * m.scale
    x = rs.uniform(x0 - margin, x0 + m.width * m.scale + margin, n)
    y = rs.uniform(y0 - margin, y0 + m.height * m.scale + margin, n)
    return np.stack([x, y, rs.uniform(-4.0, 7.0, n)], axis=1)


# three windows of different size, scale and off-centre origin
WINDOWS = ((120, 90, (40, 30), 0.1), (47, 61, (10, 50), 0.07), (77, 33, (70, 5), 0.05))


def three_jobs(pkg, ctx, kind, weighting, seed, beams=(65, 300, 130), counts=(9, 14, 5), with_scenes=False):
    """maps 0..2 and slots 0, 2 filled, the second job's scan the CURRENT one: (jobs, current); with_scenes: (jobs,
    current, maps, scans)"""
    maps = [random_map(pkg, kind, w, h, org, sc, seed + k) for k, (w, h, org, sc) in enumerate(WINDOWS)]
    scans = [random_scan(pkg, n, 0.4 * m.width * m.scale, weighting, seed + 10 + k) for k, (n, m) in enumerate(zip(beams, maps))]
    for k, m in enumerate(maps):
        ctx.upload_map(k, m)
    ctx.scan_store(0, *scans[0])
    ctx.scan_store(2, *scans[2])
    ctx.scan_upload(*scans[1])
    jobs = [(k, (0, -1, 2)[k], poses_in(maps[k], counts[k], seed + 20 + k)) for k in range(3)]
    return (jobs, scans[1], maps, scans) if with_scenes else (jobs, scans[1])


def outside_fraction(m, scan, poses):
    """the share of (pose, beam) end points outside the window, in host arithmetic"""
    rng, cos_a, sin_a = scan[:3]
    c, s = np.cos(poses[:, 2:3]), np.sin(poses[:, 2:3])
    x = poses[:, 0:1] + rng[None, :] * (c * cos_a[None, :] - s * sin_a[None, :])
    y = poses[:, 1:2] + rng[None, :] * (s * cos_a[None, :] + c * sin_a[None, :])
    ix, iy = np.floor(x / m.scale) + m.origin[0], np.floor(y / m.scale) + m.origin[1]
    return float(((ix < 0) | (ix >= m.width) | (iy < 0) | (iy >= m.height)).mean())


# ---- 1. against the compiled reference -----------------------------------------------------------------------------------
@pytest.mark.parametrize("group", [("mean_raw", "mean_cached", "affine_raw"), ("tbm_raw", "tbm_cached")], ids=["occ", "tbm"])
def test_the_reference_scenes_as_jobs_of_one_call(pkg, ctx, group):
    assert set(group) <= set(SCENES)
    gold = [load("scene_%s.npz" % s) for s in group]
    jobs = []
    for k, g in enumerate(gold):
        ctx.upload_map(k, map_from(g))
        ctx.scan_store(k, *scan_arrays(pkg, filtered_scan(g)))
        jobs.append((k, k, g["poses"]))
    strict = ctx.score_poses_batch(pkg.spe_cfg(**STRICT), jobs)
    assert ctx.score_poses_batch_stats() == dict(jobs_shared=len(group), jobs_lone=0, launches=2)
    dflt = ctx.score_poses_batch(pkg.spe_cfg(), jobs)
    assert ctx.score_poses_batch_stats() == dict(jobs_shared=len(group), jobs_lone=0, launches=1)
    for k, g in enumerate(gold):
        print(group[k], ": strict max |diff| %g, default max rel %g"
              % (np.max(np.abs(strict[k] - g["scores"])), np.max(np.abs(dflt[k] / g["scores"] - 1))))
        np.testing.assert_array_equal(strict[k], g["scores"], err_msg=group[k])  # bit-exact with the reference
        np.testing.assert_allclose(dflt[k], g["scores"], rtol=DEFAULT_RTOL, atol=0, err_msg=group[k])


def test_the_window_goldens_as_three_jobs_of_one_call(pkg, ctx):
    g = load_golden()
    ctx.upload_map(0, golden_map(g, "occ10"))
    poses = g["scan_poses"]
    areas = g["occ10_areas"][g["scan_area_idx"]]
    jobs = [(0, k, poses) for k in range(len(SCAN_SIZES))]
    for tname, trig in TRIGS:
        for k, n in enumerate(SCAN_SIZES):
            scan = golden_scan(g, n, trig)
            ctx.scan_store(k, *scan_arrays(pkg, scan))
            ctx.scan_store_angles(k, scan.angle)
        exact = dict(sum_order=pkg.SUM_SEQUENTIAL, pose_trig=pkg.POSE_TRIG_HOST if tname == "cached" else pkg.POSE_TRIG_RAW_EXACT)
        for ai, area in enumerate(areas):
            for oi, (oname, kind) in enumerate(OOPES):
                got = ctx.score_poses_batch(pkg.spe_cfg(oope=kind, area=area, **exact), jobs)
                st = ctx.score_poses_batch_stats()
                assert st == (dict(jobs_shared=3, jobs_lone=0, launches=2) if tname == "cached" else dict(jobs_shared=0, jobs_lone=3, launches=0))
                dflt = ctx.score_poses_batch(pkg.spe_cfg(oope=kind, area=area), jobs)
                assert ctx.score_poses_batch_stats() == dict(jobs_shared=3, jobs_lone=0, launches=1)
                for k, n in enumerate(SCAN_SIZES):
                    want = g["scan%d_occ10_%s" % (n, tname)][ai, oi]
                    msg = "%s %d beams area %d %s" % (tname, n, ai, oname)
                    np.testing.assert_array_equal(got[k], want, err_msg=msg)
                    np.testing.assert_allclose(dflt[k], want, rtol=DEFAULT_RTOL, atol=0, err_msg=msg)


# ---- 2. against the lone call, bit for bit ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,plane", [(CELL_OCC, 1), (CELL_TBM, 1), (CELL_TBM, 0), (CELL_CREDIBILIST, 1)],
                         ids=["occ", "tbm_plane", "tbm_cells", "credibilist"])
@pytest.mark.parametrize("weighting", ["even", "viny"])
def test_every_mode_equals_the_lone_calls(pkg, ctx, kind, plane, weighting):
    ctx.set_option(pkg.OPT_TBM_PLANE, plane)
    try:
        jobs, current, maps, scans = three_jobs(pkg, ctx, kind, weighting, seed=100 + 7 * kind + plane, with_scenes=True)
        for k in range(3):  # some beams of every job end outside its window, most inside
            assert 0.02 < outside_fraction(maps[k], scans[k], jobs[k][2]) < 0.8, k
        oies = (pkg.OIE_DISCREPANCY, pkg.OIE_OCCUPANCY) if kind == CELL_OCC else (pkg.OIE_DISCREPANCY,)
        n_checked = 0
        for oie in oies:
            for oope in (pkg.OOPE_OBSTACLE, pkg.OOPE_MAX, pkg.OOPE_MEAN, pkg.OOPE_OVERLAP):
                for sum_order in (pkg.SUM_TREE256, pkg.SUM_SEQUENTIAL):
                    for trig in (pkg.POSE_TRIG_DEVICE, pkg.POSE_TRIG_HOST):
                        cfg = pkg.spe_cfg(oope=oope, oie=oie, area=OBLONG, sum_order=sum_order, pose_trig=trig)
                        want = lone_scores(ctx, cfg, jobs, current)
                        before = ctx.scan_download()
                        got = ctx.score_poses_batch(cfg, jobs)
                        msg = "oie %d oope %d sum %d trig %d" % (oie, oope, sum_order, trig)
                        assert_bits_equal(got, want, msg)
                        assert ctx.score_poses_batch_stats() == dict(jobs_shared=3, jobs_lone=0, launches=1 + sum_order), msg
                        np.testing.assert_array_equal(bits(ctx.scan_download()), bits(before), err_msg=msg)
                        assert all(len(np.unique(w)) > len(w) // 2 for w in want), msg  # (scores differ from pose to pose)
                        n_checked += 1
        assert n_checked == 16 * len(oies)
    finally:
        ctx.set_option(pkg.OPT_TBM_PLANE, 1)


# ---- 3. ragged pose counts, every poses-per-workgroup value ----------------------------------------------------------------
@pytest.mark.parametrize("counts", [(1, 3, 1019), (1, 3, 1020), (2, 5, 2041), (5, 8178, 9)], ids=["1023", "1024", "2048", "8192"])
def test_ragged_pose_counts_with_an_empty_job_in_the_middle(pkg, ctx, counts):
    total = sum(counts)
    assert pkg_poses_per_block(total) == {1023: 1, 1024: 2, 2048: 4, 8192: 8}[total]
    maps = [random_map(pkg, CELL_OCC, w, h, org, sc, 300 + k) for k, (w, h, org, sc) in enumerate(WINDOWS)]
    for k, m in enumerate(maps):
        ctx.upload_map(k, m)
        ctx.scan_store(k, *random_scan(pkg, 65, 0.4 * m.width * m.scale, "viny", 310 + k))
    a, b, c = counts
    jobs = [(0, 0, poses_in(maps[0], a, 320)), (1, 1, poses_in(maps[1], b, 321)), (2, 2, np.zeros((0, 3))),
            (2, 2, poses_in(maps[2], c, 322))]
    for oope in (pkg.OOPE_OBSTACLE, pkg.OOPE_MAX):
        for mode in (dict(), STRICT):
            cfg = pkg.spe_cfg(oope=oope, area=OBLONG, **mode)
            got = ctx.score_poses_batch(cfg, jobs)
            assert [len(x) for x in got] == [a, b, 0, c]
            assert ctx.score_poses_batch_stats() == dict(jobs_shared=3, jobs_lone=0, launches=2 if mode else 1)
            assert_bits_equal(got, lone_scores(ctx, cfg, jobs), "oope %d %r" % (oope, mode))


def pkg_poses_per_block(n):
    """pick_poses_per_block (csrc/kernel_pick.h): tests/test_score_batch_plan_host.py holds this restatement to its text"""
    return 8 if n >= 8192 else (4 if n >= 2048 else (2 if n >= 1024 else 1))


# ---- 4. beam counts at the scorer's edges in one call ----------------------------------------------------------------------
@pytest.mark.parametrize("beams", [(1, 256, 257, 1280, 1281), (1, 256, 257, 1280)], ids=["generic", "kb5"])
def test_beam_counts_at_the_edges_of_the_beam_constant_forms(pkg, ctx, beams):
    m = random_map(pkg, CELL_TBM, *WINDOWS[0], seed=400)
    ctx.upload_map(0, m)
    for k, n in enumerate(beams):
        ctx.scan_store(k, *random_scan(pkg, n, 4.0, "viny", 410 + k))
    jobs = [(0, k, poses_in(m, 5 + k, 420 + k)) for k in range(len(beams))]
    for cfg in (pkg.spe_cfg(), pkg.spe_cfg(**STRICT), pkg.spe_cfg(oope=pkg.OOPE_MAX, area=OBLONG),
                pkg.spe_cfg(oope=pkg.OOPE_OVERLAP, area=OBLONG, **STRICT)):
        got = ctx.score_poses_batch(cfg, jobs)
        assert ctx.score_poses_batch_stats()["jobs_shared"] == len(beams)
        assert_bits_equal(got, lone_scores(ctx, cfg, jobs), "oope %d sum %d" % (cfg.oope, cfg.sum_order))


def test_a_scan_whose_weights_add_up_to_zero_scores_nan_in_its_job_alone(pkg, ctx):
    m = random_map(pkg, CELL_OCC, *WINDOWS[1], seed=430)
    ctx.upload_map(0, m)
    good = random_scan(pkg, 70, 1.5, "even", 431)
    ctx.scan_store(0, *good)
    ctx.scan_store(1, good[0], good[1], good[2], np.zeros(70), good[4])
    jobs = [(0, 0, poses_in(m, 4, 432)), (0, 1, poses_in(m, 6, 433)), (0, 0, poses_in(m, 3, 434))]
    for cfg in (pkg.spe_cfg(), pkg.spe_cfg(**STRICT), pkg.spe_cfg(oope=pkg.OOPE_MEAN, area=OBLONG)):
        got = ctx.score_poses_batch(cfg, jobs)
        assert np.all(np.isnan(got[1])) and not np.any(np.isnan(got[0])) and not np.any(np.isnan(got[2]))
        assert_bits_equal(got, lone_scores(ctx, cfg, jobs))


# ---- 5. one job far from the world origin ----------------------------------------------------------------------------------
def test_a_job_1100_cells_from_the_origin_beside_two_near_it(pkg, ctx, oracle):
    import pyoracle as po
    scenes = [placed_scenes.place("N1", size=100, scale=0.1, n_beams=200), placed_scenes.place("O", size=100, scale=0.1, n_beams=150),
              placed_scenes.place("O", cell_model=CELL_OCC, size=90, scale=0.05, n_beams=90, seed=5)]
    assert np.hypot(*scenes[0]["shift"][:2]) / 0.1 > 1100
    jobs = []
    for k, sc in enumerate(scenes):
        ctx.upload_map(k, sc["map"])
        ctx.scan_store(k, *scan_arrays(pkg, sc["scan"]))
        jobs.append((k, k, placed_scenes.candidates(sc, 12 + k, seed=500 + k)))
    for cfg in (pkg.spe_cfg(), pkg.spe_cfg(**STRICT), pkg.spe_cfg(oope=pkg.OOPE_OVERLAP, area=OBLONG)):
        assert_bits_equal(ctx.score_poses_batch(cfg, jobs), lone_scores(ctx, cfg, jobs), "oope %d sum %d" % (cfg.oope, cfg.sum_order))
    # ... and against the CPU oracle's canonical order (host pose trig: the oracle's own arithmetic)
    got = ctx.score_poses_batch(pkg.spe_cfg(pose_trig=pkg.POSE_TRIG_HOST), jobs)
    for k, sc in enumerate(scenes):
        want = oracle.score_poses(sc["map"], sc["scan"], po.make_cfg(sum_order=po.SUM_TREE256), jobs[k][2])
        np.testing.assert_array_equal(got[k], want, err_msg="scene %d" % k)
        assert len(np.unique(want)) > 8


# ---- 6. launch count -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [2, 16])
def test_one_scoring_launch_whatever_the_job_count(pkg, ctx, K):
    m = random_map(pkg, CELL_OCC, *WINDOWS[2], seed=600)
    ctx.upload_map(0, m)
    for k in range(K):
        ctx.scan_store(k, *random_scan(pkg, 40 + 3 * k, 1.0, "even", 610 + k))
    jobs = [(0, k, poses_in(m, 1 + (k % 5), 620 + k)) for k in range(K)]
    for oope in (pkg.OOPE_OBSTACLE, pkg.OOPE_MEAN):
        for sum_order, launches in ((pkg.SUM_TREE256, 1), (pkg.SUM_SEQUENTIAL, 2)):
            cfg = pkg.spe_cfg(oope=oope, area=OBLONG, sum_order=sum_order)
            got = ctx.score_poses_batch(cfg, jobs)
            assert ctx.score_poses_batch_stats() == dict(jobs_shared=K, jobs_lone=0, launches=launches)
            assert_bits_equal(got, lone_scores(ctx, cfg, jobs))


# ---- 7. the routes the shared launches do not cover --------------------------------------------------------------------------
def test_the_gmapping_estimator_runs_the_lone_calls_in_job_order(pkg, ctx):
    sc = make_scene(cell_model=CELL_GMAPPING, size=100, scale=0.1, n_beams=180, seed=7)
    ctx.upload_map(0, sc["map"])
    arrays = scan_arrays(pkg, sc["scan"])
    ctx.scan_store(0, *arrays)
    ctx.scan_store(1, arrays[0] * 0.97, *arrays[1:])
    rs = np.random.RandomState(70)
    # (the first pose of a job repeated: equal end cells at a job's seam are what the run cache carries over)
    first = sc["init_pose"] + rs.randn(3) * [0.05, 0.05, 0.02]
    jobs = [(0, 0, np.vstack([first, sc["init_pose"] + rs.randn(6, 3) * [0.1, 0.1, 0.05], first])),
            (0, 1, np.vstack([first, sc["init_pose"] + rs.randn(4, 3) * [0.1, 0.1, 0.05]])),
            (0, 0, np.vstack([first, first]))]
    ctx.scan_upload(*random_scan(pkg, 33, 2.0, "even", 71))
    before = ctx.scan_download()
    for mode in (dict(), dict(sum_order=pkg.SUM_SEQUENTIAL)):
        cfg = pkg.spe_cfg(oope=pkg.OOPE_GMAPPING, **mode)
        ctx.gm_cache_reset()
        got = ctx.score_poses_batch(cfg, jobs)
        cache = ctx.gm_cache_get()
        assert ctx.score_poses_batch_stats() == dict(jobs_shared=0, jobs_lone=3, launches=0)
        np.testing.assert_array_equal(bits(ctx.scan_download()), bits(before))  # the current scan is back
        ctx.gm_cache_reset()
        want = lone_scores(ctx, cfg, jobs)
        assert_bits_equal(got, want, repr(mode))
        assert ctx.gm_cache_get() == cache
        ctx.scan_upload(before[0], before[1], before[2], before[3], before[4])
        assert np.ptp(np.concatenate(want)) > 0


def test_raw_exact_pose_trig_runs_the_lone_calls_and_keeps_the_current_scans_angles(pkg, ctx):
    jobs, current = three_jobs(pkg, ctx, CELL_OCC, "viny", seed=700)
    rs = np.random.RandomState(701)
    angles = [np.sort(rs.uniform(-2.3, 2.3, n)) for n in (65, 300, 130)]
    ctx.scan_store_angles(0, angles[0])
    ctx.scan_store_angles(2, angles[2])
    ctx.scan_set_angles(angles[1])
    for oope in (pkg.OOPE_OBSTACLE, pkg.OOPE_MAX):
        cfg = pkg.spe_cfg(oope=oope, area=OBLONG, pose_trig=pkg.POSE_TRIG_RAW_EXACT, sum_order=pkg.SUM_SEQUENTIAL)
        before = ctx.scan_download()
        mine_before = ctx.score_poses(1, cfg, jobs[1][2])  # (the current scan under its own angles)
        got = ctx.score_poses_batch(cfg, jobs)
        assert ctx.score_poses_batch_stats() == dict(jobs_shared=0, jobs_lone=3, launches=0)
        np.testing.assert_array_equal(bits(ctx.scan_download()), bits(before))
        np.testing.assert_array_equal(bits(ctx.score_poses(1, cfg, jobs[1][2])), bits(mine_before))  # ... angles included
        np.testing.assert_array_equal(bits(got[1]), bits(mine_before))
        for k, slot in ((0, 0), (2, 2)):
            ctx.scan_select(slot)
            np.testing.assert_array_equal(bits(got[k]), bits(ctx.score_poses(k, cfg, jobs[k][2])))
        ctx.scan_upload(*current)
        ctx.scan_set_angles(angles[1])


def test_a_single_job_with_poses_takes_the_lone_route(pkg, ctx):
    jobs, current = three_jobs(pkg, ctx, CELL_TBM, "even", seed=720)
    alone = [(0, 0, np.zeros((0, 3))), jobs[1], (2, 2, np.zeros((0, 3)))]
    for cfg in (pkg.spe_cfg(), pkg.spe_cfg(oope=pkg.OOPE_MEAN, area=OBLONG, **STRICT)):
        got = ctx.score_poses_batch(cfg, alone)
        assert ctx.score_poses_batch_stats() == dict(jobs_shared=0, jobs_lone=1, launches=0)
        assert_bits_equal(got, lone_scores(ctx, cfg, alone, current))
    assert ctx.score_poses_batch(pkg.spe_cfg(), []) == []
    assert ctx.score_poses_batch_stats() == dict(jobs_shared=0, jobs_lone=0, launches=0)
    got = ctx.score_poses_batch(pkg.spe_cfg(), [(0, 0, np.zeros((0, 3))), (99, 4000, np.zeros((0, 3)))])  # (not looked at)
    assert [len(x) for x in got] == [0, 0]


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_output_the_stats_and_the_current_scan_alone(pkg, ctx):
    jobs, current = three_jobs(pkg, ctx, CELL_OCC, "even", seed=800)
    ctx.upload_map(3, random_map(pkg, CELL_TBM, *WINDOWS[1], seed=801))
    ctx.scan_store(2002, *random_scan(pkg, 9, 1.0, "even", 802))
    ctx.set_option(pkg.OPT_TBM_PLANE, 0)  # (through its plane a belief map scores as occupancies: another refusal's subject)
    try:
        cfg = pkg.spe_cfg()
        ctx.score_poses_batch(cfg, jobs)
        stats, scan = ctx.score_poses_batch_stats(), ctx.scan_download()
        assert stats == dict(jobs_shared=3, jobs_lone=0, launches=1)
        p = jobs[0][2]
        bad = {
            "unknown map": [jobs[0], (57, 0, p), jobs[2]],
            "empty slot beyond the stored ones": [jobs[0], (1, 3000, p), jobs[2]],
            "empty slot between stored ones": [jobs[0], (1, 2001, p), jobs[2]],
            "slot out of range": [jobs[0], (1, 4096, p), jobs[2]],
            "mixed cell models": [jobs[0], (3, 0, p), jobs[2]],
            "null poses": [jobs[0], jobs[1], (2, 2, 4)],
            "negative count": [jobs[0], (1, 0, -1)],
        }
        for name, js in bad.items():
            out = np.full(64, np.nan)
            with pytest.raises(pkg.SlamHipError):
                ctx.score_poses_batch(cfg, js, out=out)
            assert np.all(np.isnan(out)), name
            assert ctx.score_poses_batch_stats() == stats, name
            np.testing.assert_array_equal(bits(ctx.scan_download()), bits(scan), err_msg=name)
        # what the lone call refuses for the configuration is refused here: a window too large, OccupancyOIE over beliefs
        for js, c in ((jobs, pkg.spe_cfg(oope=pkg.OOPE_MAX, area=(-9.0, 9.0, -9.0, 9.0))),
                      ([(3, 0, p), (3, 2, p)], pkg.spe_cfg(oie=pkg.OIE_OCCUPANCY))):
            out = np.full(64, np.nan)
            with pytest.raises(pkg.SlamHipError):
                ctx.score_poses_batch(c, js, out=out)
            assert np.all(np.isnan(out)) and ctx.score_poses_batch_stats() == stats
        # ... and the call still works afterwards
        assert_bits_equal(ctx.score_poses_batch(cfg, jobs), lone_scores(ctx, cfg, jobs, current))
    finally:
        ctx.set_option(pkg.OPT_TBM_PLANE, 1)


def test_no_current_scan_is_a_state_error(pkg):
    c = pkg.Context(0)
    try:
        m = random_map(pkg, CELL_OCC, *WINDOWS[2], seed=810)
        c.upload_map(0, m)
        c.scan_store(0, *random_scan(pkg, 20, 1.0, "even", 811))
        out = np.full(8, np.nan)
        with pytest.raises(pkg.SlamHipError, match="no scan uploaded"):
            c.score_poses_batch(pkg.spe_cfg(), [(0, 0, poses_in(m, 2, 812)), (0, -1, poses_in(m, 2, 813))], out=out)
        assert np.all(np.isnan(out))
    finally:
        c.close()


# ---- 9. calls back to back whose shape grows, then shrinks -----------------------------------------------------------------
def test_back_to_back_calls_that_grow_and_shrink(pkg, ctx):
    maps = [random_map(pkg, CELL_OCC, w, h, org, sc, 900 + k) for k, (w, h, org, sc) in enumerate(WINDOWS)]
    for k, m in enumerate(maps):
        ctx.upload_map(k, m)
    for k in range(12):
        ctx.scan_store(k, *random_scan(pkg, 30 + 50 * k, 2.0, "viny" if k % 2 else "even", 910 + k))
    shapes = [[3, 2], [40, 0, 700, 9, 1, 2300, 17, 5, 64, 3, 8, 1], [1, 0, 2], [5000, 6000], [2, 2]]
    for cfg in (pkg.spe_cfg(pose_trig=pkg.POSE_TRIG_HOST), pkg.spe_cfg(oope=pkg.OOPE_MAX, area=OBLONG, sum_order=pkg.SUM_SEQUENTIAL)):
        calls = [[(k % 3, k, poses_in(maps[k % 3], n, 920 + 13 * c + k)) for k, n in enumerate(counts)] for c, counts in enumerate(shapes)]
        got = [ctx.score_poses_batch(cfg, jobs) for jobs in calls]  # back to back: nothing else touches the context
        for c, jobs in enumerate(calls):
            assert_bits_equal(got[c], lone_scores(ctx, cfg, jobs), "call %d" % c)
