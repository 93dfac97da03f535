"""CPU suite: what tests/test_gpu_placed_particle_maps.py (the per-particle tiled maps far from the world origin) leans on.

  * the oracle's PER-PARTICLE append (gmapping_particle_map_append: a filter with one private dense map per particle) is
    pinned to tests/golden/placed.npz -- the compiled reference's UnboundedLazyTiledGridMap grown from (0, 0) to each Q
    station -- bit for bit, both occupancy estimators: the GPU suite uses that route where there is no golden (diverged
    maps, the filter's own step);
  * the cases are not vacuous: every window the GPU suite downloads is crossed by a tile seam in x AND in y for the start
    extent it uses, the four-quadrant batch really needs 8-byte keys, the readers' jobs see full and empty windows and a
    best cell across a seam, the carry job carries, the ray caster's beams hit and miss;
  * OrcGmappingHandle.set (orc_gmapping_set), added for the filter's own step at a station: a run started through it at
    shift (0, 0) is today's run bit for bit, and a run started at a station resamples where the GPU test expects it to."""
import numpy as np
import placed_cases as pc
import placed_particle_cases as pp
import placed_scenes as ps
import pytest
from helpers import load
from pyoracle import OOPE_GMAPPING, Oracle, make_cfg
from pyoracle_mapupdate import (RULE_GMAPPING, append_scan_ex, gmapping_enable_particle_maps, gmapping_particle_map,
                                gmapping_particle_map_append)


@pytest.fixture(scope="module")
def g():
    return pc.golden()


@pytest.mark.parametrize("est", [0, 1], ids=["const", "area"])
@pytest.mark.parametrize("station", ps.Q_STATIONS)
def test_particle_append_vs_reference(oracle, g, station, est):
    """The bars of tests/test_oracle_placed.py::test_append_scan_vs_reference for the shared-map oracle: equality."""
    m, aux, _ = pc.fresh_map(g, station, "gmapping")
    opf = oracle.gmapping_create(4, [0.0] * 8, np.arange(4, dtype=np.uint32))
    gmapping_enable_particle_maps(oracle, opf, m, aux, **pp.oracle_adder(g, est))
    r, a, occ = pp.raw_scan(g, station)
    for k in range(3):
        assert gmapping_particle_map_append(oracle, opf, m, 1, g[station + "_append_poses"][k], r, a, occ) > 1000
        got_p, got_a = gmapping_particle_map(oracle, opf, 1)
        want_p, want_a = pp.snapshot(g, station, est, k)
        # (cell_update's GMAPPING case in oracle/map_update_oracle.c does not read `quality`: the golden's 0.9 and the
        # per-particle append's fixed 1.0 are the same update)
        np.testing.assert_array_equal(got_p, want_p, err_msg="%s step %d" % (station, k))
        np.testing.assert_array_equal(got_a, want_a, err_msg="%s step %d" % (station, k))
    for i in (0, 2, 3):  # the other particles' maps are their own
        p, c = gmapping_particle_map(oracle, opf, i)
        assert pp.never_observed(p, c, m.unknown)
    # the three appends stay inside the golden window with RING cells to spare: the GPU suite's ring is a fair check
    _, touched = pp.snapshot(g, station, est, 2)
    ys, xs = np.nonzero(touched[..., 1])
    assert xs.min() >= pp.RING and ys.min() >= pp.RING and xs.max() < touched.shape[1] - pp.RING and ys.max() < touched.shape[0] - pp.RING


def test_every_window_is_crossed_by_a_seam_in_x_and_in_y(g):
    for st in ps.Q_STATIONS:
        win = pp.golden_window(g, st)
        sx, sy = pp.window_seams(pp.START_EXTENT[st], win)
        assert sx and sy, (st, sx, sy)
        # The cells the appends WROTE are fewer (58 x 57): no parity puts a seam through them on both axes at once, but
        # each parity does on one axis -- so the growth test runs with the other start extent as well
        _, touched = pp.snapshot(g, st, 0, 2)
        t = touched[..., 1] > 0
        axes = set()
        for e in (1, 2):
            ex, ey = pp.window_seams(e, win)
            if any(t[:, s - win[0] - 1].any() and t[:, s - win[0]].any() for s in ex):
                axes.add(("x", e))
            if any(t[s - win[1] - 1].any() and t[s - win[1]].any() for s in ey):
                axes.add(("y", e))
        assert {a for a, _ in axes} == {"x", "y"} and {e for _, e in axes} == {1, 2}, (st, axes)
        # one pool over the four quadrants starts with ONE tile (its Q3 map migrates into a pool that starts with one) and
        # is compared over the wide windows: a seam on both axes at every station
        sx1, sy1 = pp.window_seams(1, pp.wide_window(st))
        assert sx1 and sy1, (st, sx1, sy1)
    # the example of the issue: Q1 with an odd start extent
    win = pp.golden_window(g, "Q1")
    assert win == (19957, 9969, 108, 76)
    assert pp.window_seams(1, win) == ([20032], []) and pp.window_seams(2, win) == ([19968], [9984])
    # the seeded pools of part 3 and the filter runs of part 5 state their own extents
    for st in ("Q1", "Q3"):
        sc = ps.place(st, cell_model=2)
        m = sc["map"]
        e = pp.smallest_extent(m.origin, m.width, m.height)
        assert e * e * 4 < 500000 and e * e <= pp.MAX_TABLE
        x0, y0 = -m.origin[0], -m.origin[1]
        sx, sy = pp.window_seams(e, (x0, y0, m.width, m.height))
        assert sx and sy, (st, e)
    assert pp.smallest_extent(ps.place("Q1", cell_model=2)["map"].origin, 240, 240) == 315
    # F1 is out of reach
    (kx, ky), _ = ps.STATIONS["F1"]
    assert pp.smallest_extent((54 - kx, 38 - ky), 108, 76) ** 2 > pp.MAX_TABLE


def test_the_mixed_batch_takes_the_wide_keys(oracle, g):
    scale = float(g["scale"])
    for lead in ps.Q_STATIONS:
        refs = {}
        for st in ps.Q_STATIONS:
            m, aux = pp.fresh_window_map(g, pp.wide_window(st))
            opf = oracle.gmapping_create(1, [0.0] * 8, np.zeros(1, dtype=np.uint32))
            gmapping_enable_particle_maps(oracle, opf, m, aux, **pp.oracle_adder(g, 1))
            refs[st] = (m, opf)
        for k in range(3):
            poses, r, a, occ = pp.four_quadrant_jobs(g, lead, k)
            kw = pp.key_window([pp.scan_bbox(p, r, a, scale) for p in poses])
            assert kw["span"][0] > 40000 and kw["span"][1] > 30000
            # cell bits + job bits + the bit that lets the invalid key sort last: more than a 4-byte key holds
            assert kw["key_w"] == 65536 and kw["cell_bits"] + kw["job_bits"] > 32 and kw["end_bit"] > 32, kw
            assert kw["cell_bits"] + kw["job_bits"] <= 62  # ("batch too large" is far away)
            for i, st in enumerate(ps.Q_STATIONS):
                one = pp.key_window([pp.scan_bbox(poses[i], r, a, scale)])
                assert one["end_bit"] <= 32 and one["key_w"] <= 128, (st, one)  # one station: 4-byte keys unless forced
                # the lead's scan from another station's pose (another heading) leaves that station's golden window but
                # stays inside the wide one, ring to spare: the oracle can follow it there (a cell outside would raise)
                m, opf = refs[st]
                assert gmapping_particle_map_append(oracle, opf, m, 0, poses[i], r, a, occ) > 1000
        for st in ps.Q_STATIONS:
            _, c = gmapping_particle_map(oracle, refs[st][1], 0)
            ys, xs = np.nonzero(c[..., 1])
            assert xs.min() >= pp.RING and ys.min() >= pp.RING and xs.max() < c.shape[1] - pp.RING and ys.max() < c.shape[0] - pp.RING
            if st == lead:  # ... and the lead's own particle repeats the golden's history
                gx0, gy0, gw, gh = pp.golden_window(g, st)
                wx0, wy0, _, _ = pp.wide_window(st)
                np.testing.assert_array_equal(c[gy0 - wy0:gy0 - wy0 + gh, gx0 - wx0:gx0 - wx0 + gw], pp.snapshot(g, st, 1, 2)[1])
            assert len(pp.window_seams(1, pp.wide_window(st))[0]) and len(pp.window_seams(1, pp.wide_window(st))[1])


@pytest.mark.parametrize("station", ps.Q_STATIONS)
def test_the_readers_jobs_are_not_vacuous(oracle, g, station):
    st = station
    m = pc.final_map(g, st, "gmapping")
    scan = pc.golden_scan(g, st, 0)
    ext = pp.START_EXTENT[st]
    poses = pp.golden_reader_poses(g, st, m, ext)
    assert np.array_equal(poses[:len(g[st + "_gm_poses"])], g[st + "_gm_poses"])
    assert len(pp.beside_seams(m, ext, min(pp.THRESHOLDS))) >= 2  # (at 0.8 the maps of Q2 and Q4 have no such cell)
    for th in pp.THRESHOLDS:
        need_seam = len(pp.beside_seams(m, ext, th)) > 0
        pp.check_shares([pp.window_view(m, scan, poses, th, ext)], "%s threshold %g" % (st, th), need_seam)
        cfg = make_cfg(oope=OOPE_GMAPPING, gm_th=th, gm_window=1)
        cs, chain = pp.carry_case(g, st)
        as_list = oracle.score_poses(m, cs, cfg, chain, Oracle.new_gm_cache())
        one_by_one = np.array([oracle.score_poses(m, cs, cfg, p[None, :], Oracle.new_gm_cache())[0] for p in chain])
        assert np.count_nonzero(as_list != one_by_one) >= 3, "the scene was meant to make at least three poses carry"
    # the ray caster: every beam's last cell lies inside the window the GPU test downloads
    poses, angles, max_dist, (x0, y0, w, h) = pp.scan_gen_case(g, st)
    scale = float(g["scale"])
    ex = np.floor((poses[:, 0:1] + max_dist * np.cos(poses[:, 2:3] + angles[None, :])) / scale)
    ey = np.floor((poses[:, 1:2] + max_dist * np.sin(poses[:, 2:3] + angles[None, :])) / scale)
    assert ex.min() >= x0 + 1 and ex.max() < x0 + w - 1 and ey.min() >= y0 + 1 and ey.max() < y0 + h - 1
    assert len(pp.window_seams(pp.START_EXTENT[st], (x0, y0, w, h))[0]) and len(pp.window_seams(pp.START_EXTENT[st], (x0, y0, w, h))[1])


def _pf_run(oracle, station, through_setter, n=pp.PF_N, seed0=pp.PF_SEED0, extra_steps=pp.PF_EXTRA):
    gg = load("gmapping_pf_update.npz")
    m, aux, shift = pp.pf_oracle_start(oracle, gg, station)
    opf = oracle.gmapping_create(n, pp.PF_GP, np.arange(seed0, seed0 + n, dtype=np.uint32), skip_rate=3)
    if through_setter:
        opf.set(poses=np.tile(shift, (n, 1)))
    gmapping_enable_particle_maps(oracle, opf, m, aux)
    log = []
    for it, k in enumerate(pp.pf_steps(gg, extra_steps)):
        extra = np.arange(9000 + 100 * it, 9000 + 100 * it + n, dtype=np.uint32)
        res, idx = opf.step(m, gg["step%d_range" % k], gg["step%d_angle" % k], None, gg["step%d_delta" % k], 7 + it, extra)
        log.append((res, idx.copy() if res else None, [a.copy() for a in opf.state()],
                    [gmapping_particle_map(oracle, opf, i) for i in (0, n - 1)]))
    return log, shift


def test_a_run_started_through_the_setter_at_no_shift_is_todays_run(oracle):
    plain, _ = _pf_run(oracle, "O", False)
    through, shift = _pf_run(oracle, "O", True)
    assert not shift.any()
    assert any(r for r, _, _, _ in plain), "the sequence was meant to trigger a resampling"
    for (r0, i0, s0, m0), (r1, i1, s1, m1) in zip(plain, through):
        assert r0 == r1 and (i0 is None or np.array_equal(i0, i1))
        for a, b in zip(s0, s1):
            assert a.tobytes() == b.tobytes()
        for (p0, c0), (p1, c1) in zip(m0, m1):
            assert p0.tobytes() == p1.tobytes() and c0.tobytes() == c1.tobytes()
    # the setter takes weights as well, and leaves what it is not given
    opf = oracle.gmapping_create(3, [0.0] * 8, np.arange(3, dtype=np.uint32))
    opf.set(weights=[0.2, 0.3, 0.5])
    poses, wts, _ = opf.state()
    assert not poses.any() and wts.tolist() == [0.2, 0.3, 0.5]
    opf.set(poses=np.arange(9.0).reshape(3, 3))
    poses, wts, _ = opf.state()
    assert poses.ravel().tolist() == list(range(9)) and wts.tolist() == [0.2, 0.3, 0.5]


@pytest.mark.parametrize("station", ["Q3", "Q1"])
def test_a_run_started_at_a_station_resamples(oracle, station):
    """what the GPU test of the filter's own step relies on: finite weights and a resampling before the last step"""
    log, shift = _pf_run(oracle, station, True)
    assert np.abs(shift[:2]).min() > 500.0
    resampled = [it for it, (r, _, _, _) in enumerate(log) if r]
    assert resampled and resampled[0] < len(log) - 1
    assert all(np.isfinite(s[1]).all() for _, _, s, _ in log)
    poses = log[-1][2][0]
    assert np.abs(poses[:, :2] - shift[:2]).max() < 5.0  # the particles stay at the station
