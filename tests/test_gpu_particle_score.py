"""GPU suite: pose sets scored over the particles' own maps (slamhip_gmapping_particle_score_poses: the kernels
k_score_gmapping_jobs and k_gm_carry_jobs of csrc/gm_score_batch.hip over the copy-on-write tile pool).

Every comparison but one is exact and made against the route the call replaces, job by job: the particle's map
DOWNLOADED over a window that covers the pool's extent with a margin, uploaded again as a dense SLAMHIP_CELL_GMAPPING map,
gm_cache_reset, scan_select of the job's scan, score_poses.  The one other comparison is against the CPU oracle's GMapping
scorer at the dense GMapping test's tolerance, 1e-11 relative (tests/test_gpu_parity.py).  Scenes and the conditions that
keep the comparisons from passing vacuously -- at least 20 % of the (pose, beam) values above 0 and 20 % equal to 0, a
best full cell across a tile seam, an end point outside the extent; asserted over the downloaded maps --:
tests/particle_score_scenes.py.

The implementation switches kernel forms at ONE place: up to 160 poses in a call every pose gets a workgroup of 1024
threads, above that one of 256 (kGmBatchWideBelow, csrc/gm_score_batch.h); every scene is scored by a call on either
side of it.  The kernels are instantiated on ceil(longest scan of the call / 256): the scans of 1, 90, 256 and 257
points put jobs of one block of beams into calls instantiated for two."""
import ctypes as C

import numpy as np
import particle_score_scenes as S
import pyoracle as po
import pytest
from helpers import load

import __graft_entry__ as ge

pytestmark = pytest.mark.gpu

N = 4
DENSE_ID = 10  # dense map ids 10 .. 10 + N - 1: the particles' downloaded maps
SLOT_CUR = 3   # the slot that holds a copy of the current scan (the dense route selects it for jobs that name -1)


@pytest.fixture(scope="module")
def pkg():
    return ge.load_package()


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def a_filter(pkg, ctx, m, n=N):
    ctx.upload_map(4, m)
    pf = pkg.GmappingFilter(ctx, pkg.gmapping_params(), n, np.arange(700, 700 + n, dtype=np.uint32))
    pf.enable_particle_maps(4, extent_tiles=2, pool_tiles=48)
    return pf


def store(pkg, ctx, slot, sc):
    c, s = pkg.beam_trig(sc.angle)
    ctx.scan_store(slot, sc.range, c, s, sc.weight, sc.factor)


def make_current(pkg, ctx, sc):
    c, s = pkg.beam_trig(sc.angle)
    ctx.scan_upload(sc.range, c, s, sc.weight, sc.factor)


def store_all(pkg, ctx, scans):
    """slots 0 .. 3 = the scans of 1, 90, 256, 257 points; the last one is the current scan as well"""
    for k, sc in enumerate(scans):
        store(pkg, ctx, k, sc)
    make_current(pkg, ctx, scans[SLOT_CUR])


class DenseRoute:
    """the route the call replaces: every particle's map downloaded over [-half, half)^2 and uploaded as a dense map"""

    def __init__(self, ctx, pf, half, particles=range(N)):
        self.ctx, self.half, self.maps = ctx, half, {}
        for i in particles:
            self.maps[i] = S.window_map(pf.particle_map(i, -half, -half, 2 * half, 2 * half)[0], -half, -half)
            ctx.upload_map(DENSE_ID + i, self.maps[i])

    def score(self, cfg, job):
        poses = np.asarray(job["poses"], dtype=np.float64).reshape(-1, 3)
        if poses.shape[0] == 0:
            return np.zeros(0)
        slot = job.get("scan_slot", -1)
        self.ctx.gm_cache_reset()
        self.ctx.scan_select(SLOT_CUR if slot < 0 else slot)
        return self.ctx.score_poses(DENSE_ID + job["particle"], cfg, poses)

    def release(self):
        for i in self.maps:
            self.ctx.map_release(DENSE_ID + i)


def both_routes(pkg, ctx, pf, dense, cfg, jobs, current, msg=""):
    """the jobs through the replaced route, then -- the current scan put back -- through the call; compared job by job"""
    want = [dense.score(cfg, j) for j in jobs]
    make_current(pkg, ctx, current)
    got = pf.score_particle_poses(jobs, cfg)
    assert len(got) == len(jobs)
    for k in range(len(jobs)):
        np.testing.assert_array_equal(got[k], want[k], err_msg="%s job %d" % (msg, k))
    return got


def views_of(dense, scans, jobs, th, extent):
    return [S.window_view(dense.maps[j["particle"]], scans[SLOT_CUR if j.get("scan_slot", -1) < 0 else j["scan_slot"]], j["poses"], th,
                          extent) for j in jobs if len(j["poses"])]


CONFIGS = [  # (gm_window, threshold, pose_trig): masks | masks | nine cells | one cell | 5 x 5 cells
    (1, S.TH_FILTER, 0), (1, S.TH_FILTER, 1), (1, S.TH_OTHER, 0), (0, S.TH_FILTER, 1), (2, S.TH_OTHER, 0)]


def cfg_of(pkg, window, th, trig):
    return pkg.spe_cfg(oope=pkg.OOPE_GMAPPING, gm_th=th, gm_window=window, pose_trig=trig)


def ragged_jobs(scans, big):
    """0, 1, 5 and 17 poses, particle 2 named twice, slots 0 .. 2 and the current scan; an empty job whose particle and
    slot do not exist; big: a job of 150 poses on top, which takes the call past 160 poses"""
    ps = S.random_poses(40)
    jobs = [dict(particle=99, scan_slot=4000, poses=np.zeros((0, 3))),
            dict(particle=2, scan_slot=1, poses=ps[0:1]),
            dict(particle=1, scan_slot=2, poses=ps[1:6]),
            dict(particle=2, scan_slot=-1, poses=ps[6:23]),
            dict(particle=3, scan_slot=0, poses=np.vstack([ps[23:26], S.seam_poses(scans[0], 6)]))]
    if big:
        jobs.append(dict(particle=0, scan_slot=2, poses=np.vstack([S.random_poses(138, S.SEED_POSES + 7), S.seam_poses(scans[2], 12)])))
        jobs.append(dict(particle=1, scan_slot=1, poses=ps[26:40]))
    return jobs


# ---- 1. the common ancestor ------------------------------------------------------------------------------------------
def test_ragged_jobs_over_the_common_ancestor_equal_the_replaced_route(pkg, ctx, oracle):
    m, scans = S.gm_map(), S.scans()
    pf = a_filter(pkg, ctx, m)
    store_all(pkg, ctx, scans)
    half = S.TILE + 16
    dense = DenseRoute(ctx, pf, half)
    np.testing.assert_array_equal(dense.maps[2].payload[16:-16, 16:-16], m.payload)  # the ancestor, and unknown around it
    extent = (-S.TILE, -S.TILE, S.TILE, S.TILE)
    small, large = ragged_jobs(scans, False), ragged_jobs(scans, True)
    assert sum(len(j["poses"]) for j in small) <= 160 < sum(len(j["poses"]) for j in large)
    for th in (S.TH_FILTER, S.TH_OTHER):
        S.check_conditions(views_of(dense, scans, large, th, extent), "ancestor, threshold %g" % th)
    for window, th, trig in CONFIGS:
        cfg = cfg_of(pkg, window, th, trig)
        a = both_routes(pkg, ctx, pf, dense, cfg, small, scans[SLOT_CUR], "window %d th %g trig %d, small" % (window, th, trig))
        st = pf.particle_score_stats()
        assert (st["jobs_scored"], st["poses_scored"], st["launches"]) == (4, 32, 2)
        b = both_routes(pkg, ctx, pf, dense, cfg, large, scans[SLOT_CUR], "window %d th %g trig %d, large" % (window, th, trig))
        # a job's scores do not depend on the other jobs of its call, nor on the kernel form
        for k in range(len(small)):
            np.testing.assert_array_equal(a[k], b[k])
        assert np.count_nonzero(np.concatenate(b)) > 10
    # the two thresholds see different full cells
    assert not np.array_equal(np.concatenate(pf.score_particle_poses(large, cfg_of(pkg, 1, S.TH_FILTER, 0))),
                              np.concatenate(pf.score_particle_poses(large, cfg_of(pkg, 1, S.TH_OTHER, 0))))
    # a scan whose weights add up to 0: NaN, as the replaced route says
    zero = S.a_scan(scans[1].range, scans[1].angle, np.zeros(90), scans[1].factor)
    store(pkg, ctx, 5, zero)
    jz = [dict(particle=1, scan_slot=5, poses=S.random_poses(3)), dict(particle=1, scan_slot=1, poses=S.random_poses(3))]
    gz = both_routes(pkg, ctx, pf, dense, cfg_of(pkg, 1, S.TH_FILTER, 0), jz, scans[SLOT_CUR], "zero weights")
    assert np.all(np.isnan(gz[0])) and not np.any(np.isnan(gz[1]))
    # the CPU oracle's GMapping scorer, one estimator object per job (sequential sum, libm: 1e-11 relative)
    got = pf.score_particle_poses(large, cfg_of(pkg, 1, S.TH_FILTER, 1))
    for k, j in enumerate(large):
        if len(j["poses"]) == 0:
            continue
        sc = scans[SLOT_CUR if j["scan_slot"] < 0 else j["scan_slot"]]
        want = oracle.score_poses(dense.maps[j["particle"]], sc, po.make_cfg(oope=po.OOPE_GMAPPING, gm_th=S.TH_FILTER, gm_window=1),
                             j["poses"], po.Oracle.new_gm_cache())
        np.testing.assert_allclose(got[k], want, rtol=1e-11, atol=1e-300, err_msg="oracle, job %d" % k)
    dense.release()
    pf.close()
    ctx.map_release(4)


# ---- 2. diverged and grown maps ----------------------------------------------------------------------------------------
FAN = np.linspace(-0.5, 0.5, 90)  # the scan that makes the maps of particles 1 and 3 grow: a wall 4 m away, beyond the low-x rim
GROW_FROM = [[-5.013, -1.027, np.pi], [-5.113, 0.933, np.pi - 0.2]]


def grown_jobs(scans):
    """(at most 160 poses, more than 160, the poses that look at the new wall): poses whose end points lie beyond the
    extent (old and grown), poses whose first end point lies within 2 cells of a tile seam, poses anywhere"""
    beyond = np.array([[6.3, 0.1, 0.0], [-12.7, -1.0, np.pi], [0.3, 6.35, 1.6], [-7.6, -1.0, 3.0], [-7.7, 0.9, 2.9],
                       [-8.9, -1.0, 0.1], [-9.05, 0.4, -0.4]])
    ps = S.random_poses(60, S.SEED_POSES + 11)
    ps[:, 0] = ps[:, 0] * 1.15 - 0.9  # (over a part of the grown extent as well)
    # poses whose first beam ends on the wall particle 1 has appended beyond the old extent
    wall = np.column_stack([GROW_FROM[0][0] + 4.0 * np.cos(np.pi + FAN[::10]), GROW_FROM[0][1] + 4.0 * np.sin(np.pi + FAN[::10])])
    look = S.poses_ending_at(scans[1], wall)
    jobs = [dict(particle=1, scan_slot=1, poses=np.vstack([beyond, look, S.seam_poses(scans[1], 10)])),
            dict(particle=3, scan_slot=2, poses=np.vstack([beyond[3:], ps[:9]])),
            dict(particle=0, scan_slot=3, poses=np.vstack([S.seam_poses(scans[3], 8), ps[9:20]])),
            dict(particle=2, scan_slot=0, poses=S.seam_poses(scans[0], 16, S.SEED_POSES + 3)),
            dict(particle=1, scan_slot=3, poses=ps[20:40])]
    more = jobs + [dict(particle=3, scan_slot=1, poses=np.vstack([ps, beyond])), dict(particle=0, scan_slot=1, poses=ps[:50])]
    return jobs, more, look


def test_diverged_and_grown_maps_equal_their_downloads(pkg, ctx):
    m, scans = S.gm_map(), S.scans()
    pf = a_filter(pkg, ctx, m)
    store_all(pkg, ctx, scans)
    before = pf.particle_map_stats()
    pf.particle_maps_append([0, 1], [[0.513, 0.277, 0.3], [-0.721, -0.433, -1.1]], np.full(90, 2.0),
                            np.linspace(-np.pi, np.pi, 90, endpoint=False))
    after = pf.particle_map_stats()
    assert after["cow_copies"] > before["cow_copies"] and after["tiles_shared"] > 0
    # growth on the low-x side: the extent gains a tile column there and the pool's origin moves
    pf.particle_maps_append([1, 3], GROW_FROM, np.full(90, 4.0), FAN)
    jobs, more, look = grown_jobs(scans)
    assert sum(len(j["poses"]) for j in jobs) <= 160 < sum(len(j["poses"]) for j in more)
    cfg = cfg_of(pkg, 1, S.TH_FILTER, 0)
    # (stream order: scored directly behind the append, before anything waits for it)
    direct = pf.score_particle_poses(jobs, cfg)
    assert pf.particle_map_stats()["tiles_in_use"] > after["tiles_in_use"]
    big = 3 * S.TILE
    dense = DenseRoute(ctx, pf, big)
    assert np.any(dense.maps[1].payload[:, :big - S.TILE, 0] != -1.0)  # cells written beyond the old extent
    assert np.count_nonzero(dense.maps[0].payload != dense.maps[1].payload) > 0
    extent = (-2 * S.TILE, -S.TILE, S.TILE, S.TILE)
    for th in (S.TH_FILTER, S.TH_OTHER):
        S.check_conditions(views_of(dense, scans, more, th, extent), "grown maps, threshold %g" % th)
    for k, j in enumerate(jobs):
        np.testing.assert_array_equal(direct[k], dense.score(cfg, j), err_msg="directly behind the append, job %d" % k)
    for window, th, trig in CONFIGS:
        c = cfg_of(pkg, window, th, trig)
        both_routes(pkg, ctx, pf, dense, c, jobs, scans[SLOT_CUR], "window %d th %g trig %d, small" % (window, th, trig))
        both_routes(pkg, ctx, pf, dense, c, more, scans[SLOT_CUR], "window %d th %g trig %d, large" % (window, th, trig))
    # the appended walls are seen: the same poses score differently over particle 1's map and particle 2's
    two = pf.score_particle_poses([dict(particle=1, scan_slot=1, poses=look), dict(particle=2, scan_slot=1, poses=look)], cfg)
    assert np.all(two[0] > 0.0) and np.any(two[0] != two[1])
    dense.release()
    pf.close()
    ctx.map_release(4)


# ---- 3. the carry ------------------------------------------------------------------------------------------------------
def test_the_run_cache_is_carried_within_a_job_and_nowhere_else(pkg, ctx):
    m, scans, cs = S.gm_map(), S.scans(), S.carry_scan()
    pf = a_filter(pkg, ctx, m)
    store_all(pkg, ctx, scans)
    store(pkg, ctx, 6, cs)
    dense = DenseRoute(ctx, pf, S.TILE + 16)
    # groups of four poses equal up to a shift of a fraction of a cell: a pose's first beam ends in the cell the pose
    # before it ended in, and its first run takes that pose's last value
    bases = S.random_poses(24, S.SEED_POSES + 5, reach=0.45)
    bases[:, :2] -= 0.5 * S.TILE * S.SCALE * 0.5  # (towards the observed side)
    shifts = np.array([[0.0, 0.0, 0.0], [2e-4, -1e-4, 0.0], [-1e-4, 3e-4, 0.0], [3e-4, 2e-4, 0.0]])
    chain = np.vstack([b + s for b in bases for s in shifts])
    cfg = cfg_of(pkg, 1, S.TH_FILTER, 1)
    after = dict(particle=1, scan_slot=1, poses=S.random_poses(5, S.SEED_POSES + 6))
    job = dict(particle=0, scan_slot=6, poses=chain)
    as_list = dense.score(cfg, job)
    one_by_one = np.array([dense.score(cfg, dict(particle=0, scan_slot=6, poses=p[None, :]))[0] for p in chain])
    n_diff = int(np.count_nonzero(as_list != one_by_one))
    assert n_diff >= 3, "the scene was meant to make at least three poses carry"
    make_current(pkg, ctx, scans[SLOT_CUR])
    ctx.gm_cache_set(5, -7, 0.25)
    scan_before = ctx.scan_download()
    got = pf.score_particle_poses([job, after], cfg)
    st = pf.particle_score_stats()
    np.testing.assert_array_equal(got[0], as_list)
    assert st["poses_carried"] >= n_diff and st["poses_carried"] > 0 and st["launches"] == 2
    assert ctx.gm_cache_get() == (5, -7, 0.25)
    np.testing.assert_array_equal(ctx.scan_download(), scan_before)
    # every pose as its own job: nothing is carried from job to job
    singles = pf.score_particle_poses([dict(particle=0, scan_slot=6, poses=p[None, :]) for p in chain], cfg)
    assert pf.particle_score_stats()["poses_carried"] == 0
    np.testing.assert_array_equal(np.concatenate(singles), one_by_one)
    assert np.any(np.concatenate(singles) != got[0])
    # the job placed behind the carrying one is what it is alone
    np.testing.assert_array_equal(got[1], pf.score_particle_poses([after], cfg)[0])
    np.testing.assert_array_equal(got[1], dense.score(cfg, after))
    # the same list in a call of more than 160 poses (the 256-thread form)
    pad = dict(particle=2, scan_slot=2, poses=S.random_poses(100, S.SEED_POSES + 8))
    make_current(pkg, ctx, scans[SLOT_CUR])
    wide = pf.score_particle_poses([pad, job, after], cfg)
    np.testing.assert_array_equal(wide[1], as_list)
    np.testing.assert_array_equal(wide[2], got[1])
    dense.release()
    pf.close()
    ctx.map_release(4)


# ---- 4. after a filter step that resamples ---------------------------------------------------------------------------
def test_scores_at_the_filters_own_poses_after_a_resampling(pkg):
    """the scene of test_scans_from_the_filters_own_poses_after_a_resampling (tests/test_gpu_particle_scan_generate.py)"""
    g = load("gmapping_pf_update.npz")
    w, h = [int(v) for v in g["size"]]
    scale, unknown = float(g["scale"]), g["unknown"][:3]
    n = 8
    ctx = pkg.Context(0)
    ctx.map_bind(4, 2, w, h, g["origin"], scale, unknown)
    c0, s0 = pkg.beam_trig(g["step0_angle"])
    ctx.map_append_scan(4, pkg.RULE_GMAPPING, g["step0_delta"], g["step0_range"], c0, s0)
    pf = pkg.GmappingFilter(ctx, pkg.gmapping_params(gp8=[0, 0.1, 0, 0.05, 0, 0, 0, 0], skip_rate=3, pose_trig=1), n,
                            np.arange(3000, 3000 + n, dtype=np.uint32))
    pf.enable_particle_maps(4, extent_tiles=w // S.TILE, pool_tiles=16 + 24 * n)
    n_base = int(g["n_steps"])
    steps = list(range(n_base)) + [1 + (k % (n_base - 1)) for k in range(20)]
    resampled = False
    for it, k in enumerate(steps):
        resampled, idx = pf.step(4, g["step%d_range" % k], g["step%d_angle" % k], None, g["step%d_delta" % k], 7 + it)
        if resampled:
            break
    assert resampled and len(set(idx.tolist())) < n, "the sequence was meant to trigger a resampling"
    cur = ctx.scan_download()  # the filter's last filtered scan: the current one
    assert cur.shape[1] > 0
    poses = pf.state()[0]
    rs = np.random.RandomState(5)
    # job i: particle i's own pose and five poses sampled around it, under the current scan
    jobs = [dict(particle=i, scan_slot=-1, poses=np.vstack([poses[i], poses[i] + rs.randn(5, 3) * [0.05, 0.05, 0.02]])) for i in range(n)]
    cfg = pkg.spe_cfg(oope=pkg.OOPE_GMAPPING, pose_trig=1)
    got = pf.score_particle_poses(jobs, cfg)
    assert pf.particle_score_stats()["launches"] == 2
    np.testing.assert_array_equal(ctx.scan_download(), cur)
    ctx.scan_store(9, *cur)
    half = w // 2 + 64
    for i in range(n):
        ctx.upload_map(DENSE_ID, S.window_map(pf.particle_map(i, -half, -half, 2 * half, 2 * half)[0], -half, -half))
        ctx.gm_cache_reset()
        ctx.scan_select(9)
        np.testing.assert_array_equal(got[i], ctx.score_poses(DENSE_ID, cfg, jobs[i]["poses"]), err_msg="particle %d" % i)
    assert all(s[0] > 0.0 for s in got)  # a matched pose explains its scan
    # duplicates of one source share its tables: equal poses score equally
    src = idx.tolist()
    a, b = next((a, b) for a in range(n) for b in range(a + 1, n) if src[a] == src[b])
    same = pf.score_particle_poses([dict(particle=a, scan_slot=9, poses=poses[a:a + 1]), dict(particle=b, scan_slot=9, poses=poses[a:a + 1])], cfg)
    np.testing.assert_array_equal(same[0], same[1])
    pf.close()
    ctx.close()


# ---- 5. refusals, stats, launch counts ---------------------------------------------------------------------------------
def test_bad_calls_are_refused_and_change_nothing(pkg, ctx):
    m, scans = S.gm_map(), S.scans()
    ctx.upload_map(4, m)
    cfg = cfg_of(pkg, 1, S.TH_FILTER, 0)
    ps = S.random_poses(4)
    bare = pkg.GmappingFilter(ctx, pkg.gmapping_params(), N, np.arange(N, dtype=np.uint32))
    with pytest.raises(pkg.SlamHipError, match="not enabled"):
        bare.score_particle_poses([dict(particle=0, scan_slot=-1, poses=ps)], cfg)
    bare.close()
    pf = a_filter(pkg, ctx, m)
    store_all(pkg, ctx, scans)
    ctx.scan_store(8, np.ones(2049), np.ones(2049), np.zeros(2049), np.ones(2049))
    good = [dict(particle=3, scan_slot=1, poses=ps), dict(particle=0, scan_slot=-1, poses=ps[:2])]
    right = pf.score_particle_poses(good, cfg)
    stats = pf.particle_score_stats()
    assert stats == dict(jobs_scored=2, poses_scored=6, launches=2, poses_carried=stats["poses_carried"])
    ctx.gm_cache_set(3, 4, 0.5)
    cur = ctx.scan_download()

    def refused(jobs, match, c=cfg, code=-1):
        with pytest.raises(pkg.SlamHipError, match=match) as e:
            pf.score_particle_poses(jobs, c)
        assert "slamhip error %d:" % code in str(e.value)
        assert pf.particle_score_stats() == stats and ctx.gm_cache_get() == (3, 4, 0.5)
        np.testing.assert_array_equal(ctx.scan_download(), cur)

    for bad in (-1, N):
        refused([good[0], dict(particle=bad, scan_slot=1, poses=ps)], "particle index")
    for bad in (4096, -2):
        refused([good[0], dict(particle=0, scan_slot=bad, poses=ps)], "scan.slot")
    refused([good[0], dict(particle=0, scan_slot=1, poses=3)], "pose list")  # a count without poses
    refused(good, "GMapping OOPE", pkg.spe_cfg(oope=pkg.OOPE_OBSTACLE))
    refused(good, "SUM_TREE256", pkg.spe_cfg(oope=pkg.OOPE_GMAPPING, sum_order=pkg.SUM_SEQUENTIAL))
    refused(good, "POSE_TRIG", pkg.spe_cfg(oope=pkg.OOPE_GMAPPING, pose_trig=pkg.POSE_TRIG_RAW_EXACT))
    refused(good, "gm_window", pkg.spe_cfg(oope=pkg.OOPE_GMAPPING, gm_window=5))
    refused([good[0], dict(particle=0, scan_slot=8, poses=ps)], "the GMapping kernel holds at most 2048 filtered beams per scan")
    refused([good[0], dict(particle=0, scan_slot=77, poses=ps)], "nothing is stored", code=-4)
    # null arguments, past the Python method; scores_out stays as it was
    dp = C.POINTER(C.c_double)
    table = (pkg.ParticleScoreJob * 1)()
    keep = np.ascontiguousarray(ps)
    table[0].particle, table[0].scan_slot, table[0].n_poses, table[0].poses_xyt = 0, 1, 4, keep.ctypes.data_as(dp)
    out = np.full(4, 7.0)
    fn = pf.L.slamhip_gmapping_particle_score_poses
    assert fn(pf.h, None, 1, table, out.ctypes.data_as(dp)) == -1
    assert fn(pf.h, C.byref(cfg), 1, None, out.ctypes.data_as(dp)) == -1
    assert fn(pf.h, C.byref(cfg), 1, table, None) == -1
    assert fn(None, C.byref(cfg), 1, table, out.ctypes.data_as(dp)) == -1
    table[0].particle = N
    assert fn(pf.h, C.byref(cfg), 1, table, out.ctypes.data_as(dp)) == -1 and np.all(out == 7.0)
    assert pf.particle_score_stats() == stats
    # ... and the next correct call is right
    again = pf.score_particle_poses(good, cfg)
    for k in range(2):
        np.testing.assert_array_equal(again[k], right[k])
    assert pf.particle_score_stats() == stats
    # launches: two whatever the number of jobs, none for a call without poses
    sixteen = [dict(particle=k % N, scan_slot=k % 3, poses=S.random_poses(1 + k % 4, S.SEED_POSES + k)) for k in range(16)]
    got = pf.score_particle_poses(sixteen, cfg)
    st = pf.particle_score_stats()
    assert (st["jobs_scored"], st["poses_scored"], st["launches"]) == (16, sum(1 + k % 4 for k in range(16)), 2)
    np.testing.assert_array_equal(got[5], pf.score_particle_poses(sixteen[5:6], cfg)[0])
    empty = pf.score_particle_poses([dict(particle=0, scan_slot=1, poses=np.zeros((0, 3))), dict(particle=-5, scan_slot=9999, poses=0)], cfg)
    assert [e.size for e in empty] == [0, 0]
    assert pf.particle_score_stats() == dict(jobs_scored=0, poses_scored=0, launches=0, poses_carried=0)
    assert pf.score_particle_poses([], cfg) == [] and pf.particle_score_stats()["launches"] == 0
    # while profiling is on, both kernels are counted
    ctx.profile_enable(True)
    pf.score_particle_poses(good, cfg)
    ms, launches, units = ctx.profile_read()
    ctx.profile_enable(False)
    assert launches == 2 and ms > 0.0 and units == 4 * 90 + 2 * 257
    pf.close()
    ctx.map_release(4)
    # slot -1 without a current scan: a context nothing was uploaded to
    fresh = pkg.Context(0)
    fresh.upload_map(4, m)
    pf2 = pkg.GmappingFilter(fresh, pkg.gmapping_params(), N, np.arange(N, dtype=np.uint32))
    pf2.enable_particle_maps(4, extent_tiles=2, pool_tiles=8)
    with pytest.raises(pkg.SlamHipError, match="no scan uploaded") as e:
        pf2.score_particle_poses([dict(particle=0, scan_slot=-1, poses=ps)], cfg)
    assert "slamhip error -4:" in str(e.value)
    pf2.close()
    fresh.close()
