"""GPU suite: laser scans generated from resident maps FAR FROM THE WORLD ORIGIN (csrc/scan_generate.hip).

tests/test_gpu_scan_generate.py runs the two kernel forms on maps whose window holds (0, 0).  Here the same kernels run at
the stations of tests/placed_scenes.py, where every tolerance of the reference's walk -- are_equal is RELATIVE,
1e-7 * max(1, |a|, |b|) -- is 10^3 ... 10^5 times as wide as next to the origin:
  * at Q1 - Q4 (1000 ... 2000 m out) against tests/golden/placed_generate.npz, the scans of the compiled reference's
    LaserScanGenerator on maps that grew out there;
  * at every station, O and F1 / F2 (10^5 m out) included, against the host entry generate_scans_host -- held to the same
    golden by tests/test_scan_generate_host.py -- in the random-map scene of test_gpu_scan_generate.py, moved by a whole
    number of cells: both libm variants, every (model, kind), status-2 beams as they come;
  * at F1 / F2, where there is no reference and the host routine shares its code with the kernel, against a property
    stated with the oracle's world_to_cells alone: every hit lies in an occupied cell of the beam's list of cells, and
    the occupied cells before it are few (touches: cells the ray clips so close to a corner that the reference merges
    the two intersections);
  * one 1080-beam, 100 m call and one scan generated behind a deferred update, at a station.
Every comparison is exact."""
import math
import os
import sys

import numpy as np
import placed_scenes as ps
import pytest
from test_gpu_scan_generate import UNKNOWN, a_map, both_forms, random_map

import __graft_entry__ as ge

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
P = np.load(os.path.join(ROOT, "tests", "golden", "placed_generate.npz"))
P_CALLS = [str(c) for c in P["calls"]]
VARIANT = int(P["sincos_variant"])
W, H, SCALE = 141, 93, 0.05  # the random-map scene of test_gpu_scan_generate.py
LOCAL_ORIGIN = (50, 61)
N_POSES = 24


@pytest.fixture(scope="module")
def pkg():
    return ge.load_package()


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def placed_map(name):
    return a_map(int(P[name + "_cell_model"]), P[name + "_payload"], P[name + "_origin"], P[name + "_scale"], P[name + "_unknown"])


@pytest.mark.parametrize("c", P_CALLS)
def test_device_scans_equal_the_references_far_from_the_origin(pkg, ctx, c):
    m = placed_map(str(P[c + "_map"]))
    assert not (0 <= m.origin[0] < m.width) and not (0 <= m.origin[1] < m.height)
    max_dist, fov, pts = P[c + "_lsp"]
    _, inc, hs = pkg.to_lsp(max_dist, fov, int(pts))
    angles = pkg.scan_gen_angles(hs, inc)
    ctx.upload_map(1, m)
    rng, status = both_forms(ctx, 1, P[c + "_poses"], angles, float(max_dist), float(P[c + "_threshold"]), int(P[c + "_occ_kind"]), VARIANT)
    np.testing.assert_array_equal(status, P[c + "_status"])
    np.testing.assert_array_equal(rng, P[c + "_range"])
    ctx.map_release(1)


# ---- the random-map scene, moved ----------------------------------------------------------------------------------------------
def accepts(pkg, m, pose):
    """sg_check_beams through the host entry (one beam of one cell's length: nothing else is computed)"""
    try:
        pkg.generate_scans_host(m, [pose], [0.0], m.scale, 0.5, 0, 0)
    except pkg.SlamHipError as e:
        assert "cell boundary" in str(e)
        return False
    return True


def moved_scene(pkg, station, model, kind):
    """(map, poses, refused): the map and the 24 poses of test_device_equals_the_host_routine_on_a_random_map -- the same
    draws -- moved to the station.  A pose the opening assertion refuses out there (the robot "at" a cell boundary
    under the relative tolerance: at F only the central part of a cell is left) is drawn again, anywhere on the map,
    until sg_check_beams accepts it; `refused` are the candidates that were turned down."""
    rs = np.random.RandomState(100 + 10 * model + kind)
    (kx, ky), _ = ps.STATIONS[station]
    m = a_map(model, random_map(rs, model, W, H), (LOCAL_ORIGIN[0] - kx, LOCAL_ORIGIN[1] - ky), SCALE, UNKNOWN[model])
    poses = np.column_stack([(rs.rand(24) * 1.3 - 0.15) * W * SCALE - 50 * SCALE, (rs.rand(24) * 1.3 - 0.15) * H * SCALE - 61 * SCALE,
                             rs.rand(24) * 6.3 - 3.15])
    cells = np.floor(poses[8:, :2] / SCALE)
    poses[8:16, :2] = (cells[:8] + 0.5) * SCALE
    poses[8:16, 2] = np.arctan2(rs.randint(-3, 4, 8), rs.randint(1, 4, 8))
    poses[16:, :2] = (cells[8:] + 0.5) * SCALE + rs.choice([3e-8, -3e-8, 1e-9, -1e-7], (8, 2))
    poses[16:, 2] = np.arctan2(rs.randint(-3, 4, 8), rs.randint(1, 4, 8))
    shift = ps.shift_m(station, SCALE)
    poses = poses + shift
    refused = []
    for j in range(N_POSES):
        while not accepts(pkg, m, poses[j]):
            refused.append(poses[j].copy())
            poses[j, 0] = (rs.rand() * 1.3 - 0.15) * W * SCALE - 50 * SCALE + shift[0]
            poses[j, 1] = (rs.rand() * 1.3 - 0.15) * H * SCALE - 61 * SCALE + shift[1]
    return m, poses, refused


@pytest.mark.parametrize("model,kind", [(0, 0), (1, 0), (1, 1), (2, 0), (3, 0)])
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("st", ps.ALL)
def test_device_equals_the_host_routine_in_the_moved_scene(pkg, ctx, st, variant, model, kind):
    m, poses, refused = moved_scene(pkg, st, model, kind)
    if st == "O":
        assert not refused and m.origin == LOCAL_ORIGIN  # the control: the old scene, pose for pose
    ctx.upload_map(1, m)
    if st in ps.F_STATIONS:
        # 10^5 m out the tolerance is 0.01 m of a 0.05 m cell: the reference refuses a fifth of each axis
        assert refused, "no candidate pose was refused at " + st
        for bad in refused:  # every candidate the host entry turned down, in both forms, behind a pose that is fine
            for sequential in (False, True):
                with pytest.raises(pkg.SlamHipError, match="cell boundary"):
                    ctx.generate_scans(1, [poses[0], bad], [0.0], 1.0, 0.5, kind, variant, sequential=sequential)
    _, inc, hs = pkg.to_lsp(0, 360, 48)
    angles = pkg.scan_gen_angles(hs, inc)
    asserting = 0
    for max_dist, thr in ((1.7, 0.5), (60.0, 0.55)):
        want = pkg.generate_scans_host(m, poses, angles, max_dist, thr, kind, variant)
        got = both_forms(ctx, 1, poses, angles, max_dist, thr, kind, variant)
        np.testing.assert_array_equal(got[1], want[1])
        np.testing.assert_array_equal(got[0], want[0])
        assert np.any(want[1] == 1) and (thr == 0.5 or np.any(want[1] == 0))
        asserting += int(np.count_nonzero(want[1] == 2))
    print("%s: %d candidate poses refused, %d status-2 beams" % (st, len(refused), asserting))
    assert asserting > 0  # beams on which the reference would trip one of its own assertions: reported alike
    ctx.map_release(1)


def occupancy_of(pkg, m, kind):
    """double(cell) of every cell of the window and of a cell outside it, from the payload alone (model 0: the payload)"""
    assert m.cell_model == pkg.CELL_OCC and kind == 0
    return m.payload[..., 0], float(m.unknown[0])


def is_touch(p, ang, cx, cy, scale):
    """The ray from p along ang only TOUCHES cell (cx, cy): the chord it cuts out of the cell (slab method, plain doubles)
    is so short that the reference's are_equal -- 1e-7 * max(1, |a|, |b|) per coordinate -- merges its two ends into one
    intersection; a ray that passes the cell's corner outside it by no more than that counts alike.  1 % of slack for
    the rounding of this restatement against the reference's line intersections."""
    c, s = math.cos(ang), math.sin(ang)
    lo, hi = -math.inf, math.inf
    for o, d, a, b in ((p[0], c, cx * scale, (cx + 1) * scale), (p[1], s, cy * scale, (cy + 1) * scale)):
        if d == 0.0:
            continue
        t0, t1 = sorted(((a - o) / d, (b - o) / d))
        lo, hi = max(lo, t0), min(hi, t1)
    ends = [(p[0] + t * c, p[1] + t * s) for t in (lo, hi)]
    return all(abs(ends[0][k] - ends[1][k]) <= 1.01e-7 * max(1.0, abs(ends[0][k]), abs(ends[1][k])) for k in (0, 1))


@pytest.mark.parametrize("st", ps.F_STATIONS)
def test_hits_lie_in_occupied_cells_of_the_oracles_walk(pkg, ctx, st):
    """Independent of the per-beam routine: the oracle's world_to_cells list of the beam, the uploaded occupancy, floor."""
    from pyoracle import Oracle
    oracle = Oracle()
    m, poses, _ = moved_scene(pkg, st, 0, 0)
    occ, unknown_occ = occupancy_of(pkg, m, 0)
    ctx.upload_map(1, m)
    _, inc, hs = pkg.to_lsp(0, 360, 48)
    angles = pkg.scan_gen_angles(hs, inc)
    max_dist, thr = 60.0, 0.55
    rng, status = both_forms(ctx, 1, poses, angles, max_dist, thr, 0, VARIANT)
    ctx.map_release(1)
    hits = touches = 0
    for p, r_row, s_row in zip(poses, rng, status):
        for a, r, s in zip(angles, r_row, s_row):
            if s != 1:
                continue
            hits += 1
            ang = a + p[2]
            cells = oracle.world_to_cells(m.scale, p[0], p[1], p[0] + max_dist * math.cos(ang), p[1] + max_dist * math.sin(ang))
            hx, hy = math.floor((p[0] + r * math.cos(ang)) / m.scale), math.floor((p[1] + r * math.sin(ang)) / m.scale)
            at = np.flatnonzero((cells[:, 0] == hx) & (cells[:, 1] == hy))
            assert at.size >= 1, "the scan point floors into no cell of the beam's walk"
            ix, iy = cells[:, 0] + m.origin[0], cells[:, 1] + m.origin[1]
            inside = (ix >= 0) & (ix < m.width) & (iy >= 0) & (iy < m.height)
            o = np.full(len(cells), unknown_occ)
            o[inside] = occ[iy[inside], ix[inside]]
            assert not o[at[0]] < thr, "a hit in a cell below the threshold"
            for j in np.flatnonzero(~(o[:at[0]] < thr)):  # an occupied cell the walk passed: it must be a touch
                assert is_touch(p, ang, int(cells[j, 0]), int(cells[j, 1]), m.scale), "an occupied cell before the hit that the ray crosses"
                touches += 1
    # Every cell at or above the threshold BEFORE the hit was verified above to be one the ray only touched: its two edge
    # intersections are are_equal, i.e. the chord through the cell is shorter than tol = 1e-7 * 10^5 m = 0.01 m of a
    # 0.05 m cell.  So no crossed occupied cell was skipped; the count is a second, coarser bar.  A ray
    # clips a crossed cell that closely with a chance below 2 tol / scale = 0.42, so the touched cells before a hit
    # number less than 0.42 / (1 - 0.42) = 0.72 per hit on average: fewer touches than hits.
    print("%s: %d hits, %d touched cells before them" % (st, hits, touches))
    assert hits > 200 and touches < hits


def test_a_long_scan_of_many_beams_far_from_the_origin(pkg, ctx):
    """1080 beams of 100 m at Q3 on 0.1 m cells: walks of up to 1400 cells -- several 64-step rounds of the wave form,
    beams too long for its margin --, nearly all of them outside the window, on the reference-built cecum and mean maps"""
    _, inc, hs = pkg.to_lsp(100.0, 270, 1080)
    angles = pkg.scan_gen_angles(hs, inc)[:1080]  # (the accumulated list has 1080 or 1081 entries)
    assert angles.size == 1080
    for name, thr in (("Q3_cecum", 1.0), ("Q3_mean", 0.6)):
        m = placed_map(name)
        poses = P["Q3_cecum_long_poses"][:2]
        ctx.upload_map(1, m)
        want = pkg.generate_scans_host(m, poses, angles, 100.0, thr, 0, VARIANT)
        got = both_forms(ctx, 1, poses, angles, 100.0, thr, 0, VARIANT)
        np.testing.assert_array_equal(got[1], want[1])
        np.testing.assert_array_equal(got[0], want[0])
        assert np.count_nonzero(want[1] == 1) > 200 and np.count_nonzero(want[1] == 0) > 200
        ctx.map_release(1)


def test_a_scan_generated_behind_a_deferred_update_sees_it_at_a_station(pkg, ctx):
    st = "Q2"
    (kx, ky), _ = ps.STATIONS[st]
    w, h, scale = 120, 120, 0.1
    m = a_map(0, np.full((h, w, 1), 0.5), (60 - kx, 60 - ky), scale, [0.5])
    ctx.upload_map(1, m)
    _, inc, hs = pkg.to_lsp(0, 270, 90)
    angles = pkg.scan_gen_angles(hs, inc)
    pose = np.array([0.053, 0.047, 0.2]) + ps.shift_m(st, scale)
    before = ctx.generate_scans(1, [pose], angles, 30.0, 0.6, 0, VARIANT)
    assert not np.any(before[1] == 1)
    c, s = pkg.beam_trig(angles)
    ctx.map_set_deferred(True)
    try:
        ctx.map_append_scan(1, pkg.RULE_MEAN, pose, np.full(angles.size, 3.0), c, s, None, quality=0.9)
        after = ctx.generate_scans(1, [pose], angles, 30.0, 0.6, 0, VARIANT)
        ctx.map_drain()
    finally:
        ctx.map_set_deferred(False)
    assert ctx.map_info(1)["origin"] == m.origin  # (the ring lies inside the window: the map did not grow)
    m.payload = ctx.map_download_window(1, 0, 0, w, h, 1)
    want = pkg.generate_scans_host(m, [pose], angles, 30.0, 0.6, 0, VARIANT)
    np.testing.assert_array_equal(after[1], want[1])
    np.testing.assert_array_equal(after[0], want[0])
    assert np.count_nonzero(after[1] == 1) > angles.size // 2
    ctx.map_release(1)
