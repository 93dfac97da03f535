"""GPU suite: laser scans generated from the particles' own maps (slamhip_gmapping_particle_generate_scans: the kernels
k_scan_generate_tiled_wave / _seq of csrc/scan_generate.hip over the copy-on-write tile pool).

Every comparison is exact and made against generate_scans_host (the same per-beam routine on the host, held to the
compiled reference's scans by tests/test_scan_generate_host.py) over the particle's DOWNLOADED window -- payload column
0, unknown outside; the window covers the pool's whole extent with a margin, so both sides read the never-observed cell
beyond it.  Scenes: tests/scan_tiled_scenes.py, shared with tests/test_scan_generate_tiled_host.py."""
import ctypes as C

import numpy as np
import pytest
import scan_tiled_scenes as S
from helpers import load

import __graft_entry__ as ge

pytestmark = pytest.mark.gpu

N = 4
DENSE_JOBS = [0, 1, 2, 3, 4, 5, 8, 9, 10, 11, 12, 16, 17, 18, 19, 20]  # 16 of the 24 poses: anywhere, on centres, beside them
PARTICLES_16 = np.array([0, 1, 2, 3, 3, 2, 1, 0, 0, 0, 2, 1, 3, 3, 1, 2], dtype=np.int32)  # (every particle named four times)


@pytest.fixture(scope="module")
def pkg():
    return ge.load_package()


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def scenes(pkg):
    return S.dense_scene(pkg), S.sparse_scene(pkg)


def a_filter(pkg, ctx, m, n=N, extent_tiles=2):
    ctx.upload_map(4, m)
    pf = pkg.GmappingFilter(ctx, pkg.gmapping_params(), n, np.arange(500, 500 + n, dtype=np.uint32))
    pf.enable_particle_maps(4, extent_tiles=extent_tiles, pool_tiles=48)
    return pf


def downloaded(pf, i, half):
    """particle i's map over the external window [-half, half)^2 as the host routine's flat map"""
    return S.window_map(pf.particle_map(i, -half, -half, 2 * half, 2 * half)[0], -half, -half)


def same(got, want, msg=""):
    np.testing.assert_array_equal(got[1], want[1], err_msg=msg)
    np.testing.assert_array_equal(got[0], want[0], err_msg=msg)


def host_jobs(pkg, maps, particles, poses, angles, max_dist, thr, variant):
    """the host routine job by job, each over its particle's downloaded map"""
    rng, st = np.zeros((len(particles), angles.size)), np.zeros((len(particles), angles.size), np.uint8)
    for k, i in enumerate(particles):
        rng[k], st[k] = [v[0] for v in pkg.generate_scans_host(maps[int(i)], poses[k:k + 1], angles, max_dist, thr, 0, variant)]
    return rng, st


def both_forms(pf, *args, **kw):
    wave = pf.generate_particle_scans(*args, **kw)
    same(pf.generate_particle_scans(*args, sequential=True, **kw), wave, "sequential form")
    return wave


def check_all(pkg, pf, half, particles, poses, angles, max_dist, thr, variants=(0, 1), maps=None):
    maps = maps or {int(i): downloaded(pf, int(i), half) for i in set(np.asarray(particles).tolist())}
    out = None
    for v in variants:
        out = both_forms(pf, particles, angles, max_dist, poses=poses, occ_threshold=thr, variant=v)
        same(out, host_jobs(pkg, maps, particles, poses, angles, max_dist, thr, v), "variant %d threshold %g" % (v, thr))
    return out, maps


def ring_scan(n=90, r=2.0):
    return np.full(n, r), np.linspace(-np.pi, np.pi, n, endpoint=False)


# ---- 1. the common ancestor ------------------------------------------------------------------------------------------
def test_scans_over_the_common_ancestor_equal_the_host_routine(pkg, ctx, scenes):
    (md, dposes, dangles, dmax, dthrs), (ms, sposes, sangles, smax, sthr) = scenes
    pf = a_filter(pkg, ctx, md)
    half = S.TILE + 16
    maps = {i: downloaded(pf, i, half) for i in range(N)}
    np.testing.assert_array_equal(maps[2].payload[16:-16, 16:-16, 0], md.payload[..., 0])  # the ancestor, and unknown around it
    assert np.all(maps[2].payload[:16, :, 0] == -1.0) and np.all(maps[2].payload[:, -16:, 0] == -1.0)
    poses = dposes[DENSE_JOBS]
    for thr in dthrs:
        got, _ = check_all(pkg, pf, half, PARTICLES_16, poses, dangles, dmax, thr, maps=maps)
        assert np.any(got[1] == 1) and (thr == -2.0 or np.any(got[1] == 0))
    # the route the call replaces, for one job: the downloaded window uploaded again as a dense map
    ctx.upload_map(5, maps[1])
    for v in (0, 1):
        got = pf.generate_particle_scans([1], dangles, dmax, poses=poses[6:7], occ_threshold=0.8, variant=v)
        same(got, ctx.generate_scans(5, poses[6:7], dangles, dmax, 0.8, 0, v), "dense re-upload")
    ctx.map_release(5)
    pf.close()
    # the sparse scene: walks of several 64-step rounds across the seams and out of the extent
    pf = a_filter(pkg, ctx, ms)
    particles = np.arange(12, dtype=np.int32) % N
    got, _ = check_all(pkg, pf, half, particles, sposes, sangles, smax, sthr)
    hit = got[1] == 1
    assert hit.mean() >= 0.1 and (~hit).mean() >= 0.1 and np.any(got[0] / S.SCALE > 128)
    # what compact_scans makes of it: the hits in beam order
    scan = pkg.compact_scans(got[0], got[1], sangles)[0]
    np.testing.assert_array_equal(scan[0], got[0][0][hit[0]])
    pf.close()
    ctx.map_release(4)


# ---- 2. diverged maps, 3. growth, 6. stream order ---------------------------------------------------------------------
def test_diverged_and_grown_maps_equal_their_downloads(pkg, ctx, scenes):
    ms, sposes, sangles, smax, sthr = scenes[1]
    pf = a_filter(pkg, ctx, ms)
    half = S.TILE + 16
    rng, ang = ring_scan()
    before = pf.particle_map_stats()
    pf.particle_maps_append([0, 1], [[0.513, 0.277, 0.3], [-0.721, -0.433, -1.1]], rng, ang)
    after = pf.particle_map_stats()
    assert after["cow_copies"] > before["cow_copies"] and after["tiles_shared"] > 0  # clones; 2 and 3 still share the ancestor's
    view = np.array([[0.0131, -0.0171, 0.4]] * N)
    got, maps = check_all(pkg, pf, half, np.arange(N, dtype=np.int32), view, sangles, smax, sthr)
    assert np.any(got[0][0] != got[0][1])  # particles 0 and 1 see different rings from the same pose ...
    same((got[0][2], got[1][2]), (got[0][3], got[1][3]))  # ... 2 and 3 the ancestor
    assert np.count_nonzero(maps[0].payload[..., 0] != maps[1].payload[..., 0]) > 0
    particles = np.arange(12, dtype=np.int32) % N
    check_all(pkg, pf, half, particles, sposes, sangles, smax, sthr, maps=maps)

    # before the growth a beam that leaves the extent reads the never-observed cell: from the last cell inside, looking
    # out, the first cell outside is a hit at -2.0 and nothing is at 0.5
    edge = np.array([[-(S.TILE - 0.5) * S.SCALE + 1e-3, 0.0131, np.pi]])
    out = pf.generate_particle_scans([2], [0.0], 3.0, poses=edge, occ_threshold=-2.0, variant=0)
    assert out[1][0, 0] == 1 and out[0][0, 0] < 2 * S.SCALE
    out = pf.generate_particle_scans([2], [0.0], 3.0, poses=edge, occ_threshold=0.5, variant=0)
    assert out[1][0, 0] == 0
    outside = np.array([[-(S.TILE + 20.5) * S.SCALE + 1e-3, 0.0131, np.pi], [-(S.TILE + 20.5) * S.SCALE + 1e-3, 0.0131, 0.05]])
    for thr in (-2.0, 0.5):
        check_all(pkg, pf, half + 64, [2, 3], outside, sangles, smax, thr, variants=(1,))

    # growth: a scan whose points lie beyond the 2 x 2 tiles on the low-x side -- the extent gains tiles there and the
    # pool's origin moves.  The points are at most 9.3 m (186 cells) from the origin: one tile a side at the most.
    tiles0 = pf.particle_map_stats()["tiles_in_use"]
    fan = np.linspace(-0.5, 0.5, 90)
    pf.particle_maps_append([1, 3], [[-5.013, -1.027, np.pi], [-5.113, 0.933, np.pi - 0.2]], np.full(90, 4.0), fan)
    # (6. stream order: generated directly behind the append, before anything waits for it)
    look = np.array([[-5.013, -1.027, np.pi]] * 2)
    direct = pf.generate_particle_scans([1, 2], sangles, smax, poses=look, occ_threshold=sthr, variant=1)
    assert pf.particle_map_stats()["tiles_in_use"] > tiles0
    big = 3 * S.TILE
    maps = {i: downloaded(pf, i, big) for i in range(N)}
    assert np.any(maps[1].payload[:, :big - S.TILE, 0] != -1.0)  # cells written beyond the old extent
    same(direct, host_jobs(pkg, maps, [1, 2], look, sangles, smax, sthr, 1), "directly behind the append")
    assert np.count_nonzero(direct[1][0] == 1) > np.count_nonzero(direct[1][1] == 1)  # the appended wall is seen
    poses = np.vstack([sposes[:6], outside, look, [[-8.013, -1.213, 0.1], [3.0131, 7.517, -1.6]]])
    particles = np.arange(len(poses), dtype=np.int32) % N
    for thr in (sthr, -2.0):
        check_all(pkg, pf, big, particles, poses, sangles, smax, thr, maps=maps)
    pf.close()
    ctx.map_release(4)


# ---- 4. after a filter step that resamples ---------------------------------------------------------------------------
def test_scans_from_the_filters_own_poses_after_a_resampling(pkg):
    """the scene of run_both in tests/test_gpu_particle_maps.py (its resampling run), without the oracle side"""
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
    _, inc, hs = pkg.to_lsp(0, 270, 90)
    angles = pkg.scan_gen_angles(hs, inc)[:90]
    particles = np.arange(n, dtype=np.int32)
    got = pf.generate_particle_scans(particles, angles, 8.0, occ_threshold=0.5)
    same(pf.generate_particle_scans(particles, angles, 8.0, occ_threshold=0.5, sequential=True), got)
    poses = pf.state()[0]
    half = w // 2 + 64  # (the scans reach 4.7 m = 94 cells from a robot that stays near the origin)
    v = pkg.scan_gen_libm_variant()
    for i in range(n):
        m = downloaded(pf, i, half)
        same((got[0][i:i + 1], got[1][i:i + 1]), pkg.generate_scans_host(m, poses[i:i + 1], angles, 8.0, 0.5, 0, v), "particle %d" % i)
    assert np.count_nonzero(got[1] == 1) > n * angles.size // 4
    # duplicates of one source share its tables and its pose: equal scans
    src = idx.tolist()
    a, b = next((a, b) for a in range(n) for b in range(a + 1, n) if src[a] == src[b])
    if np.array_equal(poses[a], poses[b]):
        same((got[0][a], got[1][a]), (got[0][b], got[1][b]))
    pf.close()
    ctx.close()


# ---- 5. refusals ---------------------------------------------------------------------------------------------------
def test_bad_calls_are_refused_and_the_next_call_is_right(pkg, ctx, scenes):
    md, dposes, dangles, dmax, _ = scenes[0]
    ctx.upload_map(4, md)
    bare = pkg.GmappingFilter(ctx, pkg.gmapping_params(), N, np.arange(N, dtype=np.uint32))
    with pytest.raises(pkg.SlamHipError, match="not enabled"):
        bare.generate_particle_scans([0], dangles, dmax, poses=dposes[:1])
    bare.close()
    pf = a_filter(pkg, ctx, md)
    m0 = downloaded(pf, 0, S.TILE + 16)
    good = dposes[:2]

    def right():
        same(pf.generate_particle_scans([3, 0], dangles, dmax, poses=good, occ_threshold=0.8, variant=1),
             pkg.generate_scans_host(m0, good, dangles, dmax, 0.8, 0, 1))  # (every particle still holds the ancestor)

    right()
    for bad in (-1, N):
        with pytest.raises(pkg.SlamHipError, match="particle index"):
            pf.generate_particle_scans([0, bad], dangles, dmax, poses=good)
        right()
    with pytest.raises(pkg.SlamHipError, match="cell boundary"):
        pf.generate_particle_scans([0, 1], dangles, dmax, poses=[good[0], [0.2, 0.13, 0.0]])
    right()
    with pytest.raises(pkg.SlamHipError, match="angle"):
        pf.generate_particle_scans([0, 1], [0.0, np.nan], dmax, poses=good)
    right()
    with pytest.raises(pkg.SlamHipError):
        pf.generate_particle_scans([0, 1], dangles, 1e9, poses=good)
    with pytest.raises(pkg.SlamHipError, match="variant"):
        pf.generate_particle_scans([0, 1], dangles, dmax, poses=good, variant=2)
    right()
    # unknown flags: past the Python method, which only knows the one flag
    rng, st = np.zeros((2, dangles.size)), np.zeros((2, dangles.size), np.uint8)
    pt = np.array([0, 1], dtype=np.int32)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    call = lambda flags: pf.L.slamhip_gmapping_particle_generate_scans(  # noqa: E731
        pf.h, 1, flags, 2, pt.ctypes.data_as(ip), good.ctypes.data_as(dp), dangles.size, dangles.ctypes.data_as(dp), dmax, 0.8,
        rng.ctypes.data_as(dp), st.ctypes.data)
    assert call(2) != 0 and call(1 | 4) != 0 and not rng.any() and not st.any()
    right()
    assert call(1) == 0 and st.any()
    # no jobs, no angles: fine, and nothing happens
    empty = pf.generate_particle_scans([], dangles, dmax, poses=np.zeros((0, 3)))
    assert empty[0].shape == (0, dangles.size)
    assert pf.generate_particle_scans([0, 1], [], dmax, poses=good)[0].shape == (2, 0)
    right()
    # poses=None: the filter's own
    pf.set(poses=np.vstack([dposes[:N]]))
    same(pf.generate_particle_scans([2, 1], dangles, dmax, occ_threshold=0.8, variant=0),
         pkg.generate_scans_host(m0, dposes[[2, 1]], dangles, dmax, 0.8, 0, 0))
    pf.close()
    ctx.map_release(4)
