"""GPU suite: the per-particle tiled maps (csrc/tile_pool.hip and everything that looks a cell up through its tables) FAR
FROM THE WORLD ORIGIN.

The six GPU files of the particle filter sit on 2 x 2 ... 8 x 8 tiles around (0, 0).  Here a pool GROWS from one or two
tiles at the origin to a Q station of tests/placed_scenes.py (hundreds of tiles at once, on the low sides in three of the
four quadrants), takes ONE batch over the four quadrants (a key window of 40 000 x 30 000 cells: 8-byte keys without the
forced option), is SEEDED at a station, is read there by the pose scorer, the ray caster and the render, MIGRATES between
pools grown differently, and runs the filter's own step with a resampling.  Past 2^20 tiles per table the pool refuses:
the F stations are out of its reach, and that limit is pinned.

Held to: tests/golden/placed.npz -- real UnboundedLazyTiledGridMap GMapping maps of the compiled reference, grown from
(0, 0) to each Q station by three append_scans, both occupancy estimators -- at the bars tests/test_gpu_placed.py sets for
the dense route under the cached provider's arithmetic (the pool combines libm (cos a, sin a) with the pose heading by
angle addition); the oracle's per-particle append and filter (pinned to that golden by
tests/test_oracle_placed_particle_maps.py, which also asserts that the cases below are not vacuous); generate_scans_host
and render_cells over downloaded windows; the dense route the particle scorer replaces.  Helpers:
tests/placed_particle_cases.py."""
import numpy as np
import placed_cases as pc
import placed_particle_cases as pp
import placed_scenes as ps
import pytest
from helpers import load

import __graft_entry__ as ge

pytestmark = pytest.mark.gpu

ANCESTOR_ID, DENSE_ID = 4, 10
UNKNOWN = np.array([-1.0, 0.0, 0.0])  # the never-observed GMapping cell of every scene here
N = 4
EST_IDS = ["const", "area"]
# obstacle means of the const estimator: the dense route's bar at these stations (MEAN_STRICT).  Measured here over every
# station, start extent, batch mode and step: see LOG.md
MEAN_BAR = pp.MEAN_STRICT


@pytest.fixture(scope="module")
def pkg():
    return ge.load_package()


@pytest.fixture(scope="module")
def po():
    import pyoracle
    return pyoracle


@pytest.fixture(scope="module")
def g():
    return pc.golden()


@pytest.fixture()
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def set_mode(pkg, ctx, mode):
    for opt, val in {"fast": (), "key64": ((pkg.OPT_K6_BATCH_KEY64, 1),), "sorted": ((pkg.OPT_K6_BATCH_FAST, 0),)}[mode]:
        ctx.set_option(opt, val)


def origin_pool(pkg, ctx, g, est, extent, n=N, n_total=None, first=0, pool_tiles=64):
    """a filter whose particles share a small never-observed ancestor around (0, 0), in a pool of extent x extent tiles"""
    unk = g["Q1_gmapping_unknown"][:3]
    ctx.map_bind(ANCESTOR_ID, pkg.CELL_GMAPPING, 32, 32, (16, 16), float(g["scale"]), unk)
    pf = pkg.GmappingFilter(ctx, pkg.gmapping_params(), n_total or n, np.arange(800 + first, 800 + first + n, dtype=np.uint32),
                            first=first, count=n)
    pf.enable_particle_maps(ANCESTOR_ID, extent_tiles=extent, pool_tiles=pool_tiles, **pp.device_adder(g, est))
    return pf


def append_at(pf, g, particle, st, k):
    """append k of the station's history into one particle's map"""
    return pf.particle_maps_append([particle], [g[st + "_append_poses"][k]], *pp.raw_scan(g, st))


def unknown_of(g):
    return g["Q1_gmapping_unknown"][:3]


def ring_is_untouched(pf, g, particle, win):
    rx0, ry0, rw, rh = pp.ringed(win)
    p, c = pf.particle_map(particle, rx0, ry0, rw, rh)
    outer = np.ones((rh, rw), bool)
    outer[pp.RING:-pp.RING, pp.RING:-pp.RING] = False
    return pp.never_observed(p[outer], c[outer], unknown_of(g))


def reads_never_observed(pf, g, particle, win):
    p, c = pf.particle_map(particle, *pp.ringed(win))
    return pp.never_observed(p, c, unknown_of(g))


def render_equals_the_download(pkg, pf, particle, windows):
    seen = set()
    for win in windows:
        pay, _ = pf.particle_map(particle, *win)
        for f in (pkg.RENDER_OCCGRID, pkg.RENDER_PGM):
            want = pkg.render_cells(pkg.CELL_GMAPPING, pay, f)
            got = pf.particle_map_render(particle, f, *win)
            np.testing.assert_array_equal(got, want[::-1] if f == pkg.RENDER_PGM else want, err_msg="render %r format %d" % (win, f))
            seen |= set(np.unique(got).tolist()) if f == pkg.RENDER_OCCGRID else set()
    return seen


def seam_windows(extent, win, w=48, h=40):
    """windows that straddle the seams of a pool that started with `extent` inside (or next to) win, and one back at (0, 0)"""
    sx, sy = pp.window_seams(extent, pp.ringed(win, 64))
    cx, cy = win[0] + win[2] // 2, win[1] + win[3] // 2
    out = [(s - w // 2, cy - h // 2, w, h) for s in sx] + [(cx - w // 2, s - h // 2, w, h) for s in sy]
    out += [(x - 5, y - 7, w, h) for x in sx[:1] for y in sy[:1]]  # a seam crossing, off-centre
    return out + [(-w // 2, -h // 2, w, h)]


def grow_to_station(pkg, ctx, g, st, est, mode, extent, check=True, stop_after=3):
    """Part 1: particle 1 of 4 takes the station's three appends into a pool that starts at the origin.  Returns (filter,
    largest relative deviation of an obstacle mean)."""
    set_mode(pkg, ctx, mode)
    pf = origin_pool(pkg, ctx, g, est, extent)
    win = pp.golden_window(g, st)
    before = pf.particle_map_stats()
    assert before["tiles_shared"] > 0
    worst = 0.0
    for k in range(stop_after):
        assert append_at(pf, g, 1, st, k) > 1000
        if not check:
            continue
        what = "%s %s %s extent %d step %d" % (st, EST_IDS[est], mode, extent, k)
        worst = max(worst, pp.check_window(pf.particle_map(1, *win), pp.snapshot(g, st, est, k), est, what, MEAN_BAR))
        assert ring_is_untouched(pf, g, 1, win), what
        for i in (0, 2, 3):
            assert reads_never_observed(pf, g, i, win), "%s: particle %d" % (what, i)
        stats = pf.particle_map_stats()
        assert stats["tiles_in_use"] > before["tiles_in_use"] and stats["tiles_shared"] > 0, what
    return pf, worst


# ---- 1. growth from the origin to a station, against the reference's own maps ----------------------------------------------------
@pytest.mark.parametrize("mode", pp.MODES)
@pytest.mark.parametrize("est", [0, 1], ids=EST_IDS)
@pytest.mark.parametrize("station", ps.Q_STATIONS)
def test_growth_from_the_origin_to_a_station(pkg, ctx, g, station, est, mode):
    """The start extent is the one whose parity puts a tile seam through the golden window in x and in y."""
    extent = pp.START_EXTENT[station]
    pf, worst = grow_to_station(pkg, ctx, g, station, est, mode, extent)
    print("obstacle means, %s %s %s extent %d: largest relative deviation %.3g" % (station, EST_IDS[est], mode, extent, worst))
    win = pp.golden_window(g, station)
    seen = render_equals_the_download(pkg, pf, 1, [win] + seam_windows(extent, win))
    assert {-1, 0} <= seen and max(seen) >= 50  # never observed, free and occupied all occur in the pictures
    assert render_equals_the_download(pkg, pf, 0, [win]) == {-1}
    pf.close()


@pytest.mark.parametrize("est", [0, 1], ids=EST_IDS)
@pytest.mark.parametrize("station", ps.Q_STATIONS)
def test_growth_with_the_other_start_extent(pkg, ctx, g, station, est):
    """The cells the appends WRITE are 58 x 57: a parity puts a seam through them on one axis only.  With the other parity
    it is the other axis (tests/test_oracle_placed_particle_maps.py asserts both)."""
    extent = 3 - pp.START_EXTENT[station]
    pf, worst = grow_to_station(pkg, ctx, g, station, est, "fast", extent)
    print("obstacle means, %s %s fast extent %d: largest relative deviation %.3g" % (station, EST_IDS[est], extent, worst))
    win = pp.golden_window(g, station)
    render_equals_the_download(pkg, pf, 1, [win] + seam_windows(extent, win))
    pf.close()


# ---- 2. one batch over four quadrants ------------------------------------------------------------------------------------------
def four_quadrants(pkg, ctx, g, est, lead, oracle=None, po=None, n_total=None):
    """Particle i stands at Q(i + 1); every append is ONE call for the four of them, the pool starts with ONE tile.  A call
    carries one scan (pp.four_quadrant_jobs): the lead station's.  With an oracle every step is checked: the lead's particle
    against the golden, the other three against the oracle's per-particle append in the pool's arithmetic."""
    from pyoracle_mapupdate import gmapping_enable_particle_maps, gmapping_particle_map, gmapping_particle_map_append
    pf = origin_pool(pkg, ctx, g, est, 1, n_total=n_total)
    wins = {st: pp.wide_window(st) for st in ps.Q_STATIONS}  # (another station's scan leaves the golden window)
    ref = {}
    if oracle is not None:
        for st in ps.Q_STATIONS:
            m, aux = pp.fresh_window_map(g, wins[st])
            opf = oracle.gmapping_create(1, [0.0] * 8, np.zeros(1, dtype=np.uint32))
            gmapping_enable_particle_maps(oracle, opf, m, aux, **pp.oracle_adder(g, est))
            ref[st] = (m, opf)
    worst = 0.0
    for k in range(3):
        poses, r, a, occ = pp.four_quadrant_jobs(g, lead, k)
        order = [0, 1, 2, 3] if k != 1 else [3, 2, 1, 0]  # (the second call lists the jobs backwards)
        nu = pf.particle_maps_append(order, poses[order], r, a, occ)
        assert nu > 4 * 1000
        if oracle is None:
            continue
        tr = device_trig_scan(pkg, po, r, a)
        onu = 0
        for i, st in enumerate(ps.Q_STATIONS):
            what = "four quadrants, lead %s, %s %s step %d" % (lead, st, EST_IDS[est], k)
            m, opf = ref[st]
            onu += gmapping_particle_map_append(oracle, opf, m, 0, poses[i], r, tr.angle, occ, trig=tr)
            if st == lead:
                worst = max(worst, pp.check_window(pf.particle_map(i, *pp.golden_window(g, st)), pp.snapshot(g, st, est, k), est, what,
                                                   MEAN_BAR))
            pp.check_window(pf.particle_map(i, *wins[st]), gmapping_particle_map(oracle, opf, 0), est, what + " (oracle)", MEAN_BAR)
            assert ring_is_untouched(pf, g, i, wins[st]), what
            for other in ps.Q_STATIONS:
                if other != st:
                    assert reads_never_observed(pf, g, i, wins[other]), "%s: particle %d at %s" % (what, i, other)
        assert nu == onu
    return pf, worst


@pytest.mark.parametrize("est", [0, 1], ids=EST_IDS)
@pytest.mark.parametrize("lead", ps.Q_STATIONS)
def test_one_batch_over_four_quadrants(pkg, ctx, po, oracle, g, lead, est):
    """The extent grows on all four sides in one call; the key window spans the four stations, so the batch sorts 8-byte
    keys although nothing forces them (the arithmetic is restated and asserted by the CPU suite)."""
    pf, worst = four_quadrants(pkg, ctx, g, est, lead, oracle, po)
    print("obstacle means, four quadrants, lead %s %s: largest relative deviation %.3g" % (lead, EST_IDS[est], worst))
    for i, st in enumerate(ps.Q_STATIONS):
        win = pp.wide_window(st)
        render_equals_the_download(pkg, pf, i, [win] + seam_windows(1, win))
    pf.close()


# ---- the readers (part 4), run on the final maps of parts 1 and 3 ------------------------------------------------------------------
def device_trig_scan(pkg, po, rng, ang):
    """the scan as the pool's update sees it: libm (cos a, sin a) per beam, combined with the heading by angle addition"""
    cos_a, sin_a = pkg.beam_trig(ang)
    tr = po.ScanData(rng, ang, trig_mode=po.TRIG_CACHED, a_min=0.0, a_delta=1.0, tab_sin=sin_a, tab_cos=cos_a)
    tr.angle = np.arange(len(ang), dtype=np.float64)
    return tr


def downloaded(po, pf, particle, win, scale, unknown):
    x0, y0, w, h = win
    return po.GridMapData(po.CELL_GMAPPING, pf.particle_map(particle, x0, y0, w, h)[0], (-x0, -y0), scale, unknown)


def score_readers(pkg, ctx, po, oracle, pf, particle, extent, scale, scan, poses, carry, win, station, n_particles=N):
    """score_particle_poses over the far-out tiles: bit-equal to the route it replaces (download, dense upload,
    gm_cache_reset, score_poses), within placed_cases' allowance of the oracle's GMapping scorer over the download."""
    dm = downloaded(po, pf, particle, win, scale, UNKNOWN)
    ctx.upload_map(DENSE_ID, dm)
    cos_a, sin_a = pkg.beam_trig(scan.angle)
    cs, chain = carry
    ctx.scan_store(6, cs.range, *pkg.beam_trig(cs.angle), cs.weight)
    other = (particle + 1) % n_particles
    pad = dict(particle=other, scan_slot=-1, poses=poses[:100])
    after = dict(particle=particle, scan_slot=-1, poses=poses[5:10])
    oscan = po.ScanData(scan.range, scan.angle, scan.weight)
    for th in pp.THRESHOLDS:
        what = "%s threshold %g" % (station, th)
        pp.check_shares([pp.window_view(dm, scan, poses, th, extent)], what, need_seam=len(pp.beside_seams(dm, extent, th)) > 0)
        ocfg = po.make_cfg(oope=po.OOPE_GMAPPING, gm_th=th, gm_window=1)
        for trig in (1, 0):
            cfg = pkg.spe_cfg(oope=pkg.OOPE_GMAPPING, gm_th=th, gm_window=1, pose_trig=trig)
            ctx.scan_upload(scan.range, cos_a, sin_a, scan.weight)
            ctx.gm_cache_reset()
            want = ctx.score_poses(DENSE_ID, cfg, poses)
            job = dict(particle=particle, scan_slot=-1, poses=poses)
            got = pf.score_particle_poses([job], cfg)[0]
            np.testing.assert_array_equal(got, want, err_msg="%s trig %d" % (what, trig))
            assert len(poses) <= 160 < len(poses) + 100  # the 1024-thread form | the 256-thread form
            wide = pf.score_particle_poses([pad, job], cfg)
            np.testing.assert_array_equal(wide[1], want, err_msg="%s trig %d, 256-thread form" % (what, trig))
            assert np.count_nonzero(got) > len(poses) // 2
            if trig == 1:  # the oracle over the downloaded window; a pose that sees no full cell at all scores 0 on both sides
                rows = pc.probe(oracle, dm, oscan, ocfg, poses)
                seen = rows[0] > 0
                assert seen.sum() > len(poses) // 2
                np.testing.assert_array_equal(got[~seen], rows[0][~seen])
                pc.compare_non_exact(got[seen], rows[:, seen], po.OOPE_GMAPPING, station, what)
        # the carry job, moved to the station
        cfg = pkg.spe_cfg(oope=pkg.OOPE_GMAPPING, gm_th=th, gm_window=1, pose_trig=1)
        ctx.scan_select(6)
        ctx.gm_cache_reset()
        as_list = ctx.score_poses(DENSE_ID, cfg, chain)
        one_by_one = []
        for p in chain:
            ctx.gm_cache_reset()
            one_by_one.append(ctx.score_poses(DENSE_ID, cfg, p[None, :])[0])
        one_by_one = np.array(one_by_one)
        n_diff = int(np.count_nonzero(as_list != one_by_one))
        assert n_diff >= 3, "the scene was meant to make at least three poses carry"
        ctx.scan_upload(scan.range, cos_a, sin_a, scan.weight)
        ctx.gm_cache_reset()
        want_after = ctx.score_poses(DENSE_ID, cfg, after["poses"])
        ctx.gm_cache_set(5, -7, 0.25)
        cjob = dict(particle=particle, scan_slot=6, poses=chain)
        got = pf.score_particle_poses([cjob, after], cfg)
        stats = pf.particle_score_stats()
        np.testing.assert_array_equal(got[0], as_list, err_msg=what + ": carry")
        np.testing.assert_array_equal(got[1], want_after, err_msg=what + ": the job behind the carrying one")
        assert stats["poses_carried"] >= n_diff and stats["launches"] == 2
        assert ctx.gm_cache_get() == (5, -7, 0.25)
        singles = pf.score_particle_poses([dict(particle=particle, scan_slot=6, poses=p[None, :]) for p in chain], cfg)
        assert pf.particle_score_stats()["poses_carried"] == 0
        np.testing.assert_array_equal(np.concatenate(singles), one_by_one)
    ctx.map_release(DENSE_ID)


def scan_readers(pkg, po, pf, particle, extent, scale, poses, angles, max_dist, win, what):
    """generate_particle_scans, both libm variants, wave and sequential forms: exact against generate_scans_host over the
    downloaded window, in which every beam ends"""
    assert all(pp.window_seams(extent, win)), what
    dm = downloaded(po, pf, particle, win, scale, UNKNOWN)
    particles = np.full(len(poses), particle, dtype=np.int32)
    for thr in (0.5, 0.05):
        for v in (0, 1):
            wave = pf.generate_particle_scans(particles, angles, max_dist, poses=poses, occ_threshold=thr, variant=v)
            seq = pf.generate_particle_scans(particles, angles, max_dist, poses=poses, occ_threshold=thr, variant=v, sequential=True)
            host = pkg.generate_scans_host(dm, poses, angles, max_dist, thr, 0, v)
            for got in (wave, seq):
                np.testing.assert_array_equal(got[1], host[1], err_msg="%s threshold %g variant %d" % (what, thr, v))
                np.testing.assert_array_equal(got[0], host[0], err_msg="%s threshold %g variant %d" % (what, thr, v))
            hit = wave[1] == 1
            assert hit.mean() >= 0.05 and (~hit).mean() >= 0.05, (what, hit.mean())


@pytest.mark.parametrize("station", ps.Q_STATIONS)
def test_readers_over_a_map_grown_to_a_station(pkg, ctx, po, oracle, g, station):
    st, extent = station, pp.START_EXTENT[station]
    pf, _ = grow_to_station(pkg, ctx, g, st, 0, "fast", extent, check=False)
    win = pp.ringed(pp.golden_window(g, st), 64)  # (holds every end point of the poses below)
    final = pc.final_map(g, st, "gmapping")
    poses = pp.golden_reader_poses(g, st, final, extent)
    score_readers(pkg, ctx, po, oracle, pf, 1, extent, float(g["scale"]), pc.golden_scan(g, st, 0), poses, pp.carry_case(g, st), win, st)
    gposes, angles, max_dist, gwin = pp.scan_gen_case(g, st)
    scan_readers(pkg, po, pf, 1, extent, float(g["scale"]), gposes, angles, max_dist, gwin, st)
    pf.close()


# ---- 3. a pool seeded at the station ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("station", ["Q1", "Q3"])
def test_a_pool_seeded_at_the_station(pkg, ctx, po, oracle, g, station):
    from pyoracle_mapupdate import gmapping_enable_particle_maps, gmapping_particle_map, gmapping_particle_map_append
    sc = pc.scene(station, cell_model=po.CELL_GMAPPING, raw=True)
    m = sc["map"]
    w, h, scale = m.width, m.height, m.scale
    extent = pp.smallest_extent(m.origin, w, h)
    assert extent > 150 and extent * extent * N < 500000
    ctx.upload_map(ANCESTOR_ID, m)
    pf = pkg.GmappingFilter(ctx, pkg.gmapping_params(), N, np.arange(N, dtype=np.uint32))
    with pytest.raises(pkg.SlamHipError, match="does not fit"):
        pf.enable_particle_maps(ANCESTOR_ID, extent_tiles=extent - 1, pool_tiles=96)
    pf.enable_particle_maps(ANCESTOR_ID, extent_tiles=extent, pool_tiles=96)
    pad = 96
    x0, y0 = -m.origin[0] - pad, -m.origin[1] - pad
    big = np.tile(np.asarray(m.unknown, dtype=np.float64)[:3], (h + 2 * pad, w + 2 * pad, 1))
    big[pad:-pad, pad:-pad] = m.payload
    for i in range(N):
        p, c = pf.particle_map(i, x0, y0, w + 2 * pad, h + 2 * pad)
        assert p.tobytes() == big.tobytes() and not c.any(), "particle %d" % i
    assert all(pp.window_seams(extent, (-m.origin[0], -m.origin[1], w, h)))
    # one diverging append for two particles, against the oracle's per-particle append over the same moved map
    r, a, occ = sc["raw"]
    r = np.minimum(r, 8.0)  # (every beam ends inside the oracle's padded window)
    rs = np.random.RandomState(40 + ps.SEEDS[station])
    poses = sc["true_pose"] + rs.randn(2, 3) * [0.05, 0.05, 0.02]
    om = po.GridMapData(po.CELL_GMAPPING, big.copy(), (-x0, -y0), scale, m.unknown)
    opf = oracle.gmapping_create(N, [0.0] * 8, np.arange(N, dtype=np.uint32))
    gmapping_enable_particle_maps(oracle, opf, om, None)
    tr = device_trig_scan(pkg, po, r, a)
    nu = pf.particle_maps_append([0, 2], poses, r, a, occ)
    onu = sum(gmapping_particle_map_append(oracle, opf, om, i, poses[k], r, tr.angle, occ, trig=tr) for k, i in enumerate((0, 2)))
    assert nu == onu > 2 * 1000
    for i in range(N):
        got = pf.particle_map(i, x0, y0, w + 2 * pad, h + 2 * pad)
        want = gmapping_particle_map(oracle, opf, i)
        pp.check_window(got, want, 0, "seeded at %s, particle %d" % (station, i), MEAN_BAR)
        assert (i in (0, 2)) == bool(got[1].any())
    win = (x0, y0, w + 2 * pad, h + 2 * pad)
    render_equals_the_download(pkg, pf, 0, [(-m.origin[0], -m.origin[1], w, h)] + seam_windows(extent, (-m.origin[0], -m.origin[1], w, h)))
    # the readers over the seeded and diverged map
    scan = sc["scan"]
    base = pc.synth_poses(sc, "gm")
    dm = downloaded(po, pf, 2, win, scale, m.unknown)  # (particle 2: a job that read another slot's row would show)
    rposes = pp.reader_poses(base, sc["true_pose"], scan, dm, extent, 710 + ps.SEEDS[station])
    carry = pp.carry_from(scan, base[2:14])
    score_readers(pkg, ctx, po, oracle, pf, 2, extent, scale, scan, rposes, carry, win, station)
    # (the synthetic world's walls stand further off than the golden's: 8 m, where a third of the beams hit)
    gposes, angles, max_dist, gwin = pp.scan_gen_poses(sc["true_pose"], scale, 900 + ps.SEEDS[station], max_dist=8.0)
    scan_readers(pkg, po, pf, 2, extent, scale, gposes, angles, max_dist, gwin, "seeded at " + station)
    pf.close()


# ---- 5. migration and resampling at a station -------------------------------------------------------------------------------------
def test_a_map_migrates_across_quadrants(pkg, ctx, g):
    """The Q3 map of the four-quadrant pool, exported and imported into a second filter's pool: same ancestor, a start extent
    of one tile, its own particle already at Q1 -- the import grows it on the LOW sides, tile by tile."""
    src, _ = four_quadrants(pkg, ctx, g, 0, "Q3", n_total=2 * N)  # global particles 0 .. 3
    dst = origin_pool(pkg, ctx, g, 0, 1, n_total=2 * N, first=N)         # global particles 4 .. 7
    assert append_at(dst, g, 0, "Q1", 0) > 1000
    q1, q3 = pp.golden_window(g, "Q1"), pp.golden_window(g, "Q3")
    pp.check_window(dst.particle_map(0, *q1), pp.snapshot(g, "Q1", 0, 0), 0, "receiver at Q1", MEAN_BAR)
    kept = [dst.particle_map(i, *pp.ringed(win)) for i in range(N) for win in (q1, q3)]
    before = dst.particle_map_stats()
    blobs = np.concatenate([src.export(), dst.export()])
    idx = np.array([0, 1, 2, 3, 4, 2, 6, 7], dtype=np.uint32)  # local particle 1 of the receiver takes global particle 2: Q3
    buf = src.export_particle_map(2)
    dst.import_maps(blobs, idx, {2: buf})
    windows = [pp.ringed(q3)] + seam_windows(1, q3)
    for win in windows:
        a_p, a_c = src.particle_map(2, *win)
        b_p, b_c = dst.particle_map(1, *win)
        assert a_p.tobytes() == b_p.tobytes() and a_c.tobytes() == b_c.tobytes(), win
        for f in (pkg.RENDER_OCCGRID, pkg.RENDER_PGM):
            np.testing.assert_array_equal(dst.particle_map_render(1, f, *win), src.particle_map_render(2, f, *win))
    pp.check_window(dst.particle_map(1, *q3), pp.snapshot(g, "Q3", 0, 2), 0, "the migrated map", MEAN_BAR)
    assert reads_never_observed(dst, g, 1, q1)  # (the receiver's own Q1 cells belong to its particle 0 alone)
    now = [dst.particle_map(i, *pp.ringed(win)) for i in range(N) for win in (q1, q3)]
    for k, ((p0, c0), (p1, c1)) in enumerate(zip(kept, now)):
        if k // 2 != 1:  # the receiving filter's other particles are unchanged
            assert p0.tobytes() == p1.tobytes() and c0.tobytes() == c1.tobytes(), k
    assert dst.particle_map_stats()["tiles_in_use"] > before["tiles_in_use"]
    # the receiver goes on: its own particle takes the next append at Q1, the migrated map the next one at Q3 -- one call
    for k in (1, 2):
        nu = dst.particle_maps_append([0] if k == 1 else [0, 1], [g["Q1_append_poses"][k]] if k == 1 else
                                      [g["Q1_append_poses"][k], g["Q3_append_poses"][0]], *pp.raw_scan(g, "Q1"))
        assert nu > 1000
        pp.check_window(dst.particle_map(0, *q1), pp.snapshot(g, "Q1", 0, k), 0, "receiver at Q1, step %d" % k, MEAN_BAR)
    assert dst.particle_map(1, *q3)[1][..., 1].sum() > src.particle_map(2, *q3)[1][..., 1].sum()
    pp.check_window(src.particle_map(2, *q3), pp.snapshot(g, "Q3", 0, 2), 0, "the source after the export", MEAN_BAR)
    # a pool that started with an EVEN extent has its seams elsewhere (the origin keeps its value modulo 128): it says so
    even = origin_pool(pkg, ctx, g, 0, 2, n_total=2 * N, first=N)
    with pytest.raises(pkg.SlamHipError, match="another tile grid"):
        even.import_maps(np.concatenate([src.export(), even.export()]), idx, {2: buf})
    even.close()
    src.close()
    dst.close()


@pytest.mark.parametrize("station", ["Q2", "Q4"])
def test_a_local_copy_shares_tiles_until_it_writes(pkg, ctx, g, station):
    """tests/test_gpu_particle_maps.py::test_particle_maps_vs_reference_copy_on_write_copies, at a station"""
    st = station
    pf, _ = grow_to_station(pkg, ctx, g, st, 1, "fast", pp.START_EXTENT[st], check=False, stop_after=2)
    win = pp.golden_window(g, st)
    s1 = pf.particle_map_stats()
    pf.import_(pf.export(), np.array([0, 1, 2, 1], dtype=np.uint32))  # particle 3 becomes a copy of particle 1
    s2 = pf.particle_map_stats()
    assert s2["cow_copies"] == s1["cow_copies"] and s2["tiles_in_use"] == s1["tiles_in_use"] and s2["tiles_shared"] > s1["tiles_shared"]
    pp.check_window(pf.particle_map(3, *win), pp.snapshot(g, st, 1, 1), 1, "the copy")
    assert append_at(pf, g, 3, st, 2) > 1000
    pp.check_window(pf.particle_map(3, *win), pp.snapshot(g, st, 1, 2), 1, "the copy, one append later")
    pp.check_window(pf.particle_map(1, *win), pp.snapshot(g, st, 1, 1), 1, "the original did not see the copy's writes")
    assert pf.particle_map_stats()["cow_copies"] > s2["cow_copies"]
    assert reads_never_observed(pf, g, 0, win) and reads_never_observed(pf, g, 2, win)
    pf.close()


@pytest.mark.parametrize("station", ["Q3", "Q1"])
def test_the_filters_own_step_at_a_station(pkg, ctx, po, oracle, g, station):
    """run_both of tests/test_gpu_particle_maps.py with everything moved to the station by whole cells: the ancestor's
    window and first pose, and both filters' poses (GmappingFilter.set, OrcGmappingHandle.set).  Six particles, the
    fixture's five steps and nine replayed ones: the 13th resamples.  Bars as near the origin -- resampling indices and
    master flags exact, poses 1e-10, maps as in part 1 -- and for the weights 1e-9 plus placed_cases' allowance of the
    GMapping scorer at the station."""
    from pyoracle_mapupdate import gmapping_enable_particle_maps, gmapping_particle_map
    gg = load("gmapping_pf_update.npz")
    n = pp.PF_N
    w, h, origin, scale, unknown, shift = pp.pf_geometry(gg, station)
    seeds = np.arange(pp.PF_SEED0, pp.PF_SEED0 + n, dtype=np.uint32)
    ctx.map_bind(ANCESTOR_ID, pkg.CELL_GMAPPING, w, h, origin, scale, unknown)
    c0, s0 = pkg.beam_trig(gg["step0_angle"])
    ctx.map_append_scan(ANCESTOR_ID, pkg.RULE_GMAPPING, gg["step0_delta"] + shift, gg["step0_range"], c0, s0)
    pf = pkg.GmappingFilter(ctx, pkg.gmapping_params(gp8=pp.PF_GP, skip_rate=3, pose_trig=1), n, seeds)
    pf.set(poses=np.tile(shift, (n, 1)))
    extent = pp.smallest_extent(origin, w, h)
    pf.enable_particle_maps(ANCESTOR_ID, extent_tiles=extent, pool_tiles=128)
    m, aux, _ = pp.pf_oracle_start(oracle, gg, station)
    opf = oracle.gmapping_create(n, pp.PF_GP, seeds, skip_rate=3)
    opf.set(poses=np.tile(shift, (n, 1)))
    gmapping_enable_particle_maps(oracle, opf, m, aux)
    x0, y0 = -origin[0], -origin[1]
    got_p, got_a = pf.particle_map(n // 2, x0, y0, w, h)  # the ancestor went into the tiles intact
    np.testing.assert_array_equal(got_p[..., 0], m.payload[..., 0])
    np.testing.assert_array_equal(got_a, aux)
    rows = pc.probe(oracle, pc.final_map(g, station, "gmapping"), pc.golden_scan(g, station, 0), po.make_cfg(oope=po.OOPE_GMAPPING),
                    g[station + "_gm_poses"])
    w_rtol = 1e-9 + pc.allowance(rows, po.OOPE_GMAPPING)[0]
    steps = pp.pf_steps(gg, pp.PF_EXTRA)
    resampled_at = []
    for it, k in enumerate(steps):
        extra = np.arange(9000 + 100 * it, 9000 + 100 * it + n, dtype=np.uint32)
        rng, ang, d = gg["step%d_range" % k], gg["step%d_angle" % k], gg["step%d_delta" % k]
        res, idx = pf.step(ANCESTOR_ID, rng, ang, None, d, 7 + it)
        ores, oidx = opf.step(m, rng, ang, None, d, 7 + it, extra)
        poses, wts, ms = pf.state()
        oposes, owts, oms = opf.state()
        assert res == ores, it
        if res:
            resampled_at.append(it)
            np.testing.assert_array_equal(idx, oidx)
        assert np.all(np.isfinite(owts))
        np.testing.assert_array_equal(ms, oms)
        np.testing.assert_allclose(poses, oposes, rtol=0, atol=1e-10, err_msg="step %d" % it)
        np.testing.assert_allclose(wts, owts, rtol=w_rtol, atol=0, err_msg="step %d" % it)
        if it in (0, 4, len(steps) - 1) or res or (resampled_at and it == resampled_at[-1] + 1):
            for i in range(n):
                want = gmapping_particle_map(oracle, opf, i)
                pp.check_window(pf.particle_map(i, x0, y0, w, h), want, 0, "step %d particle %d" % (it, i), MEAN_BAR)
    assert resampled_at and resampled_at[0] < len(steps) - 1, "the sequence was meant to trigger a resampling"
    assert np.abs(poses[:, :2] - shift[:2]).max() < 5.0 and np.abs(shift[:2]).min() > 500.0
    pf.close()


# ---- 6. limits -------------------------------------------------------------------------------------------------------------------
def test_the_f_stations_are_out_of_reach_and_say_so(pkg, ctx, g):
    """A square extent of more than 2^20 tiles (about +- 65 000 cells) is refused by tile_pool_create and tile_pool_grow."""
    (kx, ky), _ = ps.STATIONS["F1"]
    scale, unk = float(g["scale"]), unknown_of(g)
    w, h = [int(v) for v in g["window"]]
    origin = (w // 2 - kx, h // 2 - ky)
    ctx.map_bind(ANCESTOR_ID, pkg.CELL_GMAPPING, w, h, origin, scale, unk)
    pf = pkg.GmappingFilter(ctx, pkg.gmapping_params(), N, np.arange(N, dtype=np.uint32))
    with pytest.raises(pkg.SlamHipError, match="tile table too large"):
        pf.enable_particle_maps(ANCESTOR_ID, extent_tiles=pp.smallest_extent(origin, w, h), pool_tiles=64)
    with pytest.raises(pkg.SlamHipError, match="tile table too large"):
        pf.enable_particle_maps(ANCESTOR_ID, extent_tiles=1025, pool_tiles=64)  # 1024 x 1024 is the last one that fits a table
    with pytest.raises(pkg.SlamHipError, match="not enabled"):
        pf.particle_map(0, 0, 0, 4, 4)
    ctx.map_release(ANCESTOR_ID)
    ctx.map_bind(ANCESTOR_ID, pkg.CELL_GMAPPING, 32, 32, (16, 16), scale, unk)
    pf.enable_particle_maps(ANCESTOR_ID, extent_tiles=2, pool_tiles=64, **pp.device_adder(g, 0))  # the same filter, near the origin
    assert append_at(pf, g, 1, "Q2", 0) > 1000
    pp.check_window(pf.particle_map(1, *pp.golden_window(g, "Q2")), pp.snapshot(g, "Q2", 0, 0), 0, "after the refusal", MEAN_BAR)
    pf.close()


def test_an_append_beyond_the_limit_is_refused_and_changes_nothing(pkg, ctx, g):
    st = "Q1"
    pf, _ = grow_to_station(pkg, ctx, g, st, 0, "fast", pp.START_EXTENT[st], check=False, stop_after=2)
    win = pp.golden_window(g, st)
    windows = [pp.ringed(win), (-24, -20, 48, 40)]
    kept = [pf.particle_map(i, *wn) for i in range(N) for wn in windows]
    stats = pf.particle_map_stats()
    assert stats["cell_updates"] > 2 * 1000
    f1 = ps.shift_m("F1", float(g["scale"])) + [0.05, 0.05, ps.STATIONS["F1"][1]]
    r, a, occ = pp.raw_scan(g, st)
    for particles, poses in (([2], [f1]), ([1, 2], [g[st + "_append_poses"][2], f1])):  # alone | beside a job that would fit
        with pytest.raises(pkg.SlamHipError, match="tile table too large"):
            pf.particle_maps_append(particles, poses, r, a, occ)
        assert pf.particle_map_stats() == stats
        now = [pf.particle_map(i, *wn) for i in range(N) for wn in windows]
        for (p0, c0), (p1, c1) in zip(kept, now):
            assert p0.tobytes() == p1.tobytes() and c0.tobytes() == c1.tobytes()
    assert append_at(pf, g, 1, st, 2) > 1000  # the next append at the station still equals the reference's map
    pp.check_window(pf.particle_map(1, *win), pp.snapshot(g, st, 0, 2), 0, "after the refused append", MEAN_BAR)
    pf.close()
