"""GPU suite (-m gpu): the max-impact map pyramid and its bound scorer FAR FROM THE WORLD ORIGIN (csrc/map_pyramid.hip).

A level's cell is floor(x / 2^k) of an EXTERNAL coordinate, so a map moved by an odd number of cells has other blocks, other
winners and -- one level per doubling until the window fits [-2^k, 2^k) -- many more levels: 16 at the Q stations of
tests/placed_scenes.py, 23 at the F stations, most of them 1 x 1 or 1 x 2 windows whose origin lies far outside the window,
with the 1 x 1 level of infinite scale on top.  tests/test_gpu_pyramid.py never leaves a 37 x 29 map with origin (11, 20).

Here the golden maps 64 / 66 / 67 (that map as GridCell, TBM and Credibilist) stand at every station (pyramid_cases.
moved_golden): levels against the host build and the brute-force statement of the definition, refreshes against rebuilds
with dirty cells on the block corners as they fall THERE, bounds against slamhip_score_poses on the level's own map id and
against the oracle's window scorer on the downloaded level -- the infinite one included.  At the N stations (500 ... 1500
cells out) levels and strict bounds are the compiled reference's (tests/golden/placed_pyramid.npz).  BF_M3RSM (csrc/m3rsm.hip,
m3rsm_engine.cpp, m3rsm_each.cpp) runs at the same stations: a lone match's trace against its own tree and inputs, the
batch forms against the lone match, the expand kernels against the bound scorer.  Every comparison is exact but the
default mode's bounds against the oracle, which follow placed_cases.compare_non_exact.  Station O is the control: the moved
scene is the old scene."""
import os
import sys

import numpy as np
import placed_scenes as ps
import pytest
import placed_cases as pc
from m3rsm_cases import children, host_slots
from pyramid_cases import (FAR_MAPS, FAR_STATIONS, LONE_STATIONS, ORACLE_MAPS, assert_levels_are, assert_same_level, bits,
                           bound_probe_rows, expected_level_count, far_brute_levels, moved_golden, moved_set, placed_counts,
                           placed_golden_map, placed_golden_set, placed_lone_scene, placed_many_scene, placed_raw_scene)
from test_gpu_pyramid import FINE, FIRST, STRICT, DeviceArrays, assert_levels_equal, download_levels, poses_of

import __graft_entry__ as ge

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pkg():
    return ge.load_package()


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def po():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import pyoracle
    return pyoracle


def upload(pkg, ctx, m, s):
    ctx.upload_map(FINE, m)
    ctx.scan_upload(s.scan[:, 0], s.scan[:, 1], s.scan[:, 2], s.scan[:, 3], s.scan[:, 4])
    return pkg.Pyramid(ctx, FINE, m.oie, FIRST)


# ---- levels --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("st", FAR_STATIONS)
@pytest.mark.parametrize("i", FAR_MAPS)
def test_device_levels_far_from_the_origin(pkg, ctx, i, st):
    m = moved_golden(i, st)
    ctx.upload_map(FINE, m)
    pyr = pkg.Pyramid(ctx, FINE, m.oie, FIRST)
    got = download_levels(ctx, pyr, pkg.STRIDE[m.cell_model])
    host = pkg.pyramid_build_host(m, m.oie)
    assert len(got) == expected_level_count(m)
    assert [lv["map_id"] for lv in got] == list(range(FIRST, FIRST + len(host)))
    assert_levels_equal(got, host)  # geometry and payload, bit for bit
    assert_levels_are(got, far_brute_levels(pkg, i, st), m.unknown)
    assert np.isinf(got[-1]["scale"]) and got[-1]["origin"] == (0, 0) and got[-1]["payload"].shape[:2] == (1, 1)
    for lv, h in zip(got, host):  # an ordinary bound map of the fine map's model: geometry and render
        info = ctx.map_info(lv["map_id"])
        assert info["cell_model"] == m.cell_model and info["scale"] == h["scale"] and info["origin"] == h["origin"]
        assert (info["width"], info["height"]) == (h["width"], h["height"])
        img = ctx.map_render(lv["map_id"], pkg.RENDER_OCCGRID)
        np.testing.assert_array_equal(img, pkg.render_cells(m.cell_model, h["payload"], pkg.RENDER_OCCGRID))
    pyr.close()
    ctx.map_release(FINE)


# ---- refresh -------------------------------------------------------------------------------------------------------------------
def corner_cells(m):
    """Internal coordinates of cells next to block borders of EVERY level AS THEY FALL AT THE STATION: per level the first
    external x and y inside the window that are multiples of 2^lv (levels 1 ... 4 always have both in a 37 x 29 window;
    a higher level has one where a border of its blocks happens to cross the window, and then only in x or only in y:
    the other coordinate is the window's middle), the cell there, the cell diagonally before it and the one below or
    beside it; the window's own corners."""
    x_lo, y_lo = -m.origin[0], -m.origin[1]
    out = [(0, 0), (m.width - 1, m.height - 1), (0, m.height - 1)]
    levels_with_a_border = []
    for lv in range(1, expected_level_count(m)):
        bx, by = -((-(x_lo + 1)) >> lv) << lv, -((-(y_lo + 1)) >> lv) << lv  # (the smallest multiple above the first cell)
        in_x, in_y = bx < x_lo + m.width, by < y_lo + m.height
        assert lv > 4 or (in_x and in_y)
        if not (in_x or in_y):
            continue
        levels_with_a_border.append(lv)
        ex, ey = bx if in_x else x_lo + m.width // 2, by if in_y else y_lo + m.height // 2
        for c in ((ex, ey), (ex - 1, ey - 1), (ex, ey - 1), (ex - 1, ey)):
            c = (c[0] - x_lo, c[1] - y_lo)
            if c not in out:
                out.append(c)
    return out, levels_with_a_border


@pytest.mark.parametrize("st", ["Q3", "F1"])
@pytest.mark.parametrize("i", FAR_MAPS)
def test_refresh_at_a_station_equals_rebuild(pkg, ctx, i, st):
    m = moved_golden(i, st)
    stride = pkg.STRIDE[m.cell_model]
    ctx.upload_map(FINE, m)
    pyr = pkg.Pyramid(ctx, FINE, m.oie, FIRST)
    before = download_levels(ctx, pyr, stride)
    top = before[-1]["payload"][0, 0]
    known = ~np.all(bits(m.payload) == bits(m.unknown), axis=-1)
    donors = m.payload[known]
    low = np.array([1.0 / 1024]) if stride == 1 else np.array([0.1, 0.9, 0.0, 0.0])  # an impact below every donor's
    high = np.array([1.0]) if stride == 1 else np.array([0.0, 0.0, 1.0, 0.0])  # impact 1: above every donor's
    unknown = np.asarray(m.unknown, dtype=np.float64)[:stride]
    coords, bordered = corner_cells(m)
    # Q3: borders of the blocks of levels 5 ... 8 cross the window too (x = -10016, -9984); F1: x = 2^21 itself, a border of
    # every finite level's blocks
    assert bordered == ({"Q3": [1, 2, 3, 4, 5, 6, 7, 8], "F1": list(range(1, 22))}[st])
    vals = [donors[(7 * j + 3) % len(donors)] for j in range(len(coords))]
    coords.append((coords[4][0] + 1, coords[4][1]))  # a cell that becomes unknown again
    vals.append(unknown)
    for y, x in np.argwhere(np.all(bits(m.payload) == bits(top), axis=-1)):  # the map's maximum goes DOWN
        if (int(x), int(y)) not in coords:
            coords.append((int(x), int(y)))
            vals.append(low)
    changed = m.payload.copy()
    m2 = type(m)(**{**vars(m), "payload": changed})

    def apply(cells, new, window):
        ctx.map_apply_dirty(FINE, cells, np.asarray(new))
        pyr.refresh(*window)
        for (x, y), v in zip(cells, new):
            changed[y, x] = v
        got = download_levels(ctx, pyr, stride)
        assert_levels_equal(got, pkg.pyramid_build_host(m2, m.oie))
        return got

    xs, ys = [c[0] for c in coords], [c[1] for c in coords]
    refreshed = apply(coords, vals, (min(xs), min(ys), max(xs) - min(xs) + 1, max(ys) - min(ys) + 1))
    pyr.rebuild()
    assert_levels_equal(refreshed, download_levels(ctx, pyr, stride))
    assert sum(not np.array_equal(bits(a["payload"]), bits(b["payload"])) for a, b in zip(before, refreshed)) >= 3
    # the two interior windows of test_refresh_of_a_window_equals_rebuild: across block borders that lie elsewhere here
    for x0, y0, w, h in ((8, 17, 6, 5), (34, 27, 3, 2)):
        cells = [(x0 + dx, y0 + dy) for dy in range(h) for dx in range(w)]
        new = [donors[(11 * j + 5) % len(donors)] for j in range(len(cells))]
        new[1] = unknown
        apply(cells, new, (x0, y0, w, h))
    # one cell alone changes the winner of every level above it, the 1 x 1 level of infinite scale included
    was = download_levels(ctx, pyr, stride)
    assert not np.array_equal(bits(was[-1]["payload"][0, 0]), bits(high))
    now = apply([(20, 3)], [high], (20, 3, 1, 1))
    np.testing.assert_array_equal(bits(now[-1]["payload"][0, 0]), bits(high))
    assert all(not np.array_equal(bits(a["payload"]), bits(b["payload"])) for a, b in zip(was, now))
    pyr.close()
    ctx.map_release(FINE)


# ---- bounds --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("st", FAR_STATIONS)
@pytest.mark.parametrize("i,n", [(64, 1), (64, 63), (64, 65), (64, 206), (66, 65), (66, 206), (67, 63), (67, 206)])
def test_score_matches_equals_score_poses_on_the_level_far_out(pkg, ctx, st, i, n):
    m, s = moved_set(i, st)
    pyr = upload(pkg, ctx, m, s)
    rot206, rect206 = pkg.m3rsm_root_candidates((1.0, 1.0, 2 * 0.087), 0.0017)
    rot = np.concatenate([s.cand[s.n_roots - 2:, 0], rot206])[:n]
    rect = np.concatenate([s.cand[s.n_roots - 2:, 1:5], rect206])[:n]
    ids = pyr.level_map_ids()
    poses = poses_of(s.pose, rot, rect)
    seen = set()
    for sum_order in (pkg.SUM_TREE256, pkg.SUM_SEQUENTIAL):
        for pose_trig in (pkg.POSE_TRIG_DEVICE, pkg.POSE_TRIG_HOST):
            mode = dict(sum_order=sum_order, pose_trig=pose_trig)
            got, level = pyr.score_matches(pkg.spe_cfg(oope=pkg.OOPE_MAX, oie=m.oie, area=(9, 9, 9, 9), **mode), s.pose, rot, rect)
            assert got.shape == (n,) and np.all((level >= 0) & (level < len(ids)))
            want = np.array([ctx.score_poses(ids[level[k]], pkg.spe_cfg(oope=pkg.OOPE_MAX, oie=m.oie, area=rect[k], **mode), poses[k:k + 1])[0]
                             for k in range(n)])
            np.testing.assert_array_equal(bits(got), bits(want), err_msg="%s %r" % (st, mode))
            seen |= set(level.tolist())
    if n > 1:
        assert len(seen) >= 3  # mixed levels in one launch
    pyr.close()
    ctx.map_release(FINE)


@pytest.mark.parametrize("i", FAR_MAPS)
def test_device_resident_candidates_far_out(pkg, ctx, i):
    m, s = moved_set(i, "F1")
    pyr = upload(pkg, ctx, m, s)
    rot, rect = s.cand[:, 0].copy(), s.cand[:, 1:5].copy()
    n = rot.size
    dev = DeviceArrays()
    d_rot, d_rect = dev.put(rot), dev.put(rect)
    d_score, d_level = dev.put(np.zeros(n)), dev.put(np.zeros(n, np.int32))
    cfg = pkg.spe_cfg(oope=pkg.OOPE_MAX, oie=m.oie)
    pyr.score_matches_device(cfg, s.pose, n, d_rot, d_rect, d_score, d_level)
    ctx.synchronize()
    got, level = dev.get(d_score, np.zeros(n)), dev.get(d_level, np.zeros(n, np.int32))
    want, want_level = pyr.score_matches(cfg, s.pose, rot, rect)
    np.testing.assert_array_equal(bits(got), bits(want))
    np.testing.assert_array_equal(level, want_level)
    dev.free()
    pyr.close()
    ctx.map_release(FINE)


@pytest.mark.parametrize("st", ["Q1", "F2"])
@pytest.mark.parametrize("i", [64, 66])  # (the models the oracle scores)
def test_large_rectangles_reach_every_level(pkg, ctx, po, oracle, i, st):
    """Rectangles with sides 2^k * scale for every k up to the plan's last, and one larger: level k -- at last the level of
    infinite scale -- is selected, and the bound is the oracle's window scorer (strict arithmetic) run on the DOWNLOADED
    level as a plain map of that scale and origin."""
    m, s = moved_set(i, st)
    pyr = upload(pkg, ctx, m, s)
    stride = pkg.STRIDE[m.cell_model]
    levels = [dict(origin=m.origin, scale=m.scale, payload=m.payload)] + download_levels(ctx, pyr, stride)
    n_lv = len(levels)
    assert n_lv == expected_level_count(m) + 1
    sides, side = [], m.scale
    for k in range(n_lv - 1):
        assert side == levels[k]["scale"]
        sides.append(side)
        side = side * 2
    sides.append(side)  # larger than the last finite level's cell
    # off-centre rectangles (the centre is added to the pose: up to 1600 m at Q1), square, wide and tall ones; halves and
    # quarters only, so that the larger side IS the level's scale, bit for bit
    shapes = (lambda v: (0.0, v, -0.5 * v, 0.5 * v), lambda v: (-0.5 * v, 0.5 * v, -v, 0.0), lambda v: (-0.5 * v, 0.5 * v, -0.25 * v, 0.25 * v))
    rect = np.array([shapes[k % 3](v) for k, v in enumerate(sides)])
    assert np.array_equal(np.maximum(rect[:, 1] - rect[:, 0], rect[:, 3] - rect[:, 2]), sides)
    rot = np.linspace(-0.3, 0.3, len(sides))
    got, level = pyr.score_matches(pkg.spe_cfg(oope=pkg.OOPE_MAX, oie=m.oie, **STRICT), s.pose, rot, rect)
    assert level.tolist() == list(range(n_lv))  # every level once, the infinite one last
    assert np.isinf(levels[level[-1]]["scale"])
    poses = poses_of(s.pose, rot, rect)
    tab = po.ScanData(s.scan[:, 0], np.arange(s.scan.shape[0], dtype=np.float64), s.scan[:, 3], s.scan[:, 4], po.TRIG_CACHED, 0.0, 1.0,
                      np.ascontiguousarray(s.scan[:, 2]), np.ascontiguousarray(s.scan[:, 1]))
    for k in range(n_lv):
        lv = levels[k]
        plain = po.GridMapData(m.cell_model, lv["payload"], lv["origin"], lv["scale"], m.unknown)
        want = oracle.score_poses(plain, tab, po.make_cfg(oope=po.OOPE_MAX, oie=m.oie, area=tuple(rect[k])), poses[k:k + 1])
        np.testing.assert_array_equal(bits(got[k:k + 1]), bits(want), err_msg="%s level %d of %d" % (st, k, n_lv))
    assert np.all(np.isfinite(got)) and len(set(got.tolist())) > 3
    pyr.close()
    ctx.map_release(FINE)


@pytest.mark.parametrize("st", FAR_STATIONS)
@pytest.mark.parametrize("i", ORACLE_MAPS)
def test_bounds_equal_the_oracles_on_the_level_far_out(pkg, ctx, po, oracle, i, st):
    """An independent value for both modes: the oracle's window scorer on the level the candidate is scored on.  Strict
    mode equals it bit for bit.  The default mode (device sincos, tree sum) is held to it by the rule of
    placed_cases.compare_non_exact: OOPE_MAX is piecewise constant, so candidates whose ORACLE score changes when x / y
    move by one ulp are left out -- at most MAX_LEFT_OUT of the set (tests/test_pyramid_host.py asserts that the oracle
    alone stays under the cap) -- and the others keep the near-origin 1e-12; station O keeps it for every candidate."""
    m, s = moved_set(i, st)
    pyr = upload(pkg, ctx, m, s)
    rot, rect = s.cand[:, 0], s.cand[:, 1:5]
    rows = bound_probe_rows(pkg, po, oracle, i, st)
    strict, level = pyr.score_matches(pkg.spe_cfg(oope=pkg.OOPE_MAX, oie=m.oie, **STRICT), s.pose, rot, rect)
    np.testing.assert_array_equal(level, s.cand[:, 7])
    np.testing.assert_array_equal(bits(strict), bits(rows[0]), err_msg="%s map %d" % (st, i))
    dflt, _ = pyr.score_matches(pkg.spe_cfg(oope=pkg.OOPE_MAX, oie=m.oie), s.pose, rot, rect)
    rtol, left_out = pc.compare_non_exact(dflt, rows, po.OOPE_MAX, st, "default-mode bounds, map %d" % i)
    print("%s map %d: rtol %.3g, %.1f %% of %d candidates left out" % (st, i, rtol, 100 * left_out, rot.size))
    pyr.close()
    ctx.map_release(FINE)


@pytest.mark.parametrize("st", FAR_STATIONS)
@pytest.mark.parametrize("i", FAR_MAPS)
def test_no_child_bound_exceeds_its_parents_far_out(pkg, ctx, i, st):
    """the reference's own assertion (m3rsm_engine.h:352-354) over a golden candidate set moved to the station; at O the
    bounds and levels ARE the golden's"""
    m, s = moved_set(i, st)
    pyr = upload(pkg, ctx, m, s)
    rot, rect, parent = s.cand[:, 0], s.cand[:, 1:5], s.cand[:, 5].astype(int)
    kids = parent >= 0
    assert kids.sum() >= 30
    for mode in (STRICT, {}):
        sc, level = pyr.score_matches(pkg.spe_cfg(oope=pkg.OOPE_MAX, oie=m.oie, **mode), s.pose, rot, rect)
        assert np.all(sc[kids] <= sc[parent[kids]] + 1e-5), "%s mode %r" % (st, mode)
        np.testing.assert_array_equal(level, s.cand[:, 7])  # (the level depends on the rectangle alone)
        if st == "O":
            if mode:
                np.testing.assert_array_equal(sc, s.cand[:, 6])
            else:
                np.testing.assert_allclose(sc, s.cand[:, 6], rtol=1e-12, atol=0)
    pyr.close()
    ctx.map_release(FINE)


# ---- the compiled reference at the N stations (tests/golden/placed_pyramid.npz) ---------------------------------------------------
@pytest.mark.parametrize("st", ps.N_STATIONS)
def test_device_levels_equal_the_references_at_the_n_stations(pkg, ctx, st):
    for i in range(placed_counts()[0]):
        m = placed_golden_map(st, i)
        ctx.upload_map(FINE, m)
        pyr = pkg.Pyramid(ctx, FINE, m.oie, FIRST)
        got = download_levels(ctx, pyr, pkg.STRIDE[m.cell_model])
        assert_levels_equal(got, pkg.pyramid_build_host(m, m.oie))
        assert len(got) == len(m.levels)
        for k, (lv, want) in enumerate(zip(got, m.levels), 1):
            assert lv["scale"] == want["scale"]
            assert_same_level(lv["payload"], lv["origin"], want["payload"], want["origin"], m.unknown, "%s map %d level %d" % (st, i, k))
        pyr.close()
        ctx.map_release(FINE)


@pytest.mark.parametrize("st", ps.N_STATIONS)
def test_strict_bounds_equal_the_references_at_the_n_stations(pkg, ctx, st):
    """every golden match set of the station: the level the reference's map was left at and Match::prob_upper_bound, bit
    for bit in the strict mode; no child above its parent in either mode"""
    levels_seen = set()
    for j in range(placed_counts()[1]):
        s = placed_golden_set(st, j)
        m = placed_golden_map(st, s.map)
        pyr = upload(pkg, ctx, m, s)
        rot, rect, parent, want, want_level = s.cand[:, 0], s.cand[:, 1:5], s.cand[:, 5].astype(int), s.cand[:, 6], s.cand[:, 7]
        strict, level = pyr.score_matches(pkg.spe_cfg(oope=pkg.OOPE_MAX, oie=m.oie, **STRICT), s.pose, rot, rect)
        np.testing.assert_array_equal(level, want_level, err_msg="%s set %d" % (st, j))
        np.testing.assert_array_equal(bits(strict), bits(want), err_msg="%s set %d" % (st, j))
        dflt, level = pyr.score_matches(pkg.spe_cfg(oope=pkg.OOPE_MAX, oie=m.oie), s.pose, rot, rect)
        np.testing.assert_array_equal(level, want_level)
        kids = parent >= 0
        assert kids.sum() >= 30
        for sc in (strict, dflt):
            assert np.all(sc[kids] <= sc[parent[kids]] + 1e-5), "%s set %d" % (st, j)
        levels_seen |= set(level.tolist())
        pyr.close()
        ctx.map_release(FINE)
    assert len(levels_seen) >= 4 and 0 in levels_seen


# ---- BF_M3RSM --------------------------------------------------------------------------------------------------------------------
# At the Q and F stations there is no reference, and the engine never sees a world coordinate except through scores: so
# its INPUTS (every traced score against score_poses and the oracle on the traced level) and its TREE (every traced call
# a child of an earlier one by m3rsm_cases.children, the result the first best zero-size call) are checked, and the batch
# forms against the lone match.
LIMITS = (0.4, 0.4, np.deg2rad(5.0), np.deg2rad(1.0), 0.05)  # max_x, max_y, max_th, rotation step, translation step
ID_STRIDE = 40  # map ids per request: the fine map and up to 23 levels behind it


def m3rsm_cfg(pkg, oie, strict):
    return pkg.spe_cfg(oope=pkg.OOPE_MAX, oie=oie, sum_order=pkg.SUM_SEQUENTIAL if strict else pkg.SUM_TREE256,
                       pose_trig=pkg.POSE_TRIG_HOST if strict else pkg.POSE_TRIG_DEVICE)


def lone_match(pkg, ctx, pyr, fine_id, oie, strict, pose, limits=LIMITS, cfg=None):
    """process_scan of a fresh matcher over the selected scan: (result, trace)"""
    mt = pkg.Matcher(ctx, "BF_M3RSM", m3rsm_cfg(pkg, oie, strict) if cfg is None else cfg, [pyr, *limits])
    r = mt.process_scan(fine_id, pose)
    trace = mt.m3rsm_trace()
    r["scorer_calls"] = mt.stats()["scorer_calls"]
    mt.close()
    return r, trace


def assert_trace_is_a_tree_with_its_result(pkg, trace, r):
    rot_roots, rect_roots = pkg.m3rsm_root_candidates((LIMITS[0], LIMITS[1], 2 * LIMITS[2]), LIMITS[3])
    n_roots = rot_roots.size
    assert len(trace) > n_roots
    np.testing.assert_array_equal(bits(trace[:n_roots, 0]), bits(rot_roots))
    np.testing.assert_array_equal(bits(trace[:n_roots, 1:5]), bits(rect_roots))
    born = {}  # (rotation, rectangle) -> made by an earlier call
    for k, row in enumerate(trace):
        key = row[:5].tobytes()
        assert k < n_roots or key in born, "call %d is no child of an earlier call" % k
        for kid in children(row[1:5], LIMITS[4]):
            born.setdefault(np.array([row[0], *kid]).tobytes(), k)
    point = (trace[:, 1] == trace[:, 2]) & (trace[:, 3] == trace[:, 4])
    assert point.any()
    best = np.flatnonzero(point & (trace[:, 5] == trace[point, 5].max()))[0]  # the first among equals
    assert r["prob"] == trace[best, 5]
    np.testing.assert_array_equal(bits(r["delta"]), bits(np.array([trace[best, 3], trace[best, 1], trace[best, 0]])))


@pytest.mark.parametrize("st", ps.Q_STATIONS + ps.F_STATIONS + ["O"])
@pytest.mark.parametrize("i", FAR_MAPS)
def test_a_far_match_scores_its_inputs_and_walks_its_tree(pkg, ctx, po, oracle, i, st):
    m, s = moved_set(i, st)
    pyr = upload(pkg, ctx, m, s)
    ids = pyr.level_map_ids()
    r, trace = lone_match(pkg, ctx, pyr, FINE, m.oie, True, s.pose)
    assert_trace_is_a_tree_with_its_result(pkg, trace, r)
    rot, rect, score, level = trace[:, 0], trace[:, 1:5], trace[:, 5], trace[:, 6].astype(int)
    poses = poses_of(s.pose, rot, rect)
    # a few hundred calls: every one against score_poses on the traced level's own map id
    cfg = lambda k: pkg.spe_cfg(oope=pkg.OOPE_MAX, oie=m.oie, area=rect[k], **STRICT)
    want = np.array([ctx.score_poses(ids[level[k]], cfg(k), poses[k:k + 1])[0] for k in range(len(trace))])
    np.testing.assert_array_equal(bits(score), bits(want))
    assert len(set(level.tolist())) >= 3 and 0 in level
    if i in ORACLE_MAPS:  # ... and against the oracle on the downloaded level
        levels = [dict(origin=m.origin, scale=m.scale, payload=m.payload)] + download_levels(ctx, pyr, pkg.STRIDE[m.cell_model])
        plain = [po.GridMapData(m.cell_model, lv["payload"], lv["origin"], lv["scale"], m.unknown) for lv in levels]
        tab = po.ScanData(s.scan[:, 0], np.arange(s.scan.shape[0], dtype=np.float64), s.scan[:, 3], s.scan[:, 4], po.TRIG_CACHED, 0.0, 1.0,
                          np.ascontiguousarray(s.scan[:, 2]), np.ascontiguousarray(s.scan[:, 1]))
        want = np.array([oracle.score_poses(plain[level[k]], tab, po.make_cfg(oope=po.OOPE_MAX, oie=m.oie, area=tuple(rect[k])), poses[k:k + 1])[0]
                         for k in range(len(trace))])
        np.testing.assert_array_equal(bits(score), bits(want))
    # the default mode (device sincos, tree sum): its own tree, its own inputs -- exact again; how far its scores lie from
    # the oracle's is test_bounds_equal_the_oracles_on_the_level_far_out's matter
    d, dtrace = lone_match(pkg, ctx, pyr, FINE, m.oie, False, s.pose)
    assert_trace_is_a_tree_with_its_result(pkg, dtrace, d)
    rect, level = dtrace[:, 1:5], dtrace[:, 6].astype(int)
    poses = poses_of(s.pose, dtrace[:, 0], rect)
    want = np.array([ctx.score_poses(ids[level[k]], pkg.spe_cfg(oope=pkg.OOPE_MAX, oie=m.oie, area=rect[k]), poses[k:k + 1])[0]
                     for k in range(len(dtrace))])
    np.testing.assert_array_equal(bits(dtrace[:, 5]), bits(want))
    if st == "O":  # the control keeps the near-origin bar: the strict mode's match
        np.testing.assert_array_equal(bits(d["delta"]), bits(r["delta"]))
        assert abs(d["prob"] - r["prob"]) <= 1e-12 * abs(r["prob"])
    pyr.close()
    ctx.map_release(FINE)


# ---- whole matches of the compiled reference at the N stations (placed_pyramid.npz: lone_*, many_*) ----------------------------
@pytest.mark.parametrize("st", ps.N_STATIONS)
def test_strict_mode_is_the_references_match_call_for_call_at_the_n_stations(pkg, ctx, st):
    s = placed_lone_scene(st)
    assert s.name == LONE_STATIONS[st]
    pyr = upload(pkg, ctx, s, s)
    assert len(pyr.info()) == 12
    r, trace = lone_match(pkg, ctx, pyr, FINE, s.oie, True, s.pose, s.limits)
    print("%s at %s: %d calls, prob %.17g (reference %.17g)" % (s.name, st, len(trace), r["prob"], s.prob))
    np.testing.assert_array_equal(bits(trace), bits(s.trace))
    np.testing.assert_array_equal(bits(r["delta"]), bits(s.delta))
    assert r["prob"] == s.prob and r["scorer_calls"] == len(s.trace)
    # the default mode (device sincos, tree sum) finds the reference's match: the near-origin bar of tests/test_gpu_m3rsm.py
    d, _ = lone_match(pkg, ctx, pyr, FINE, s.oie, False, s.pose, s.limits)
    np.testing.assert_array_equal(d["delta"], s.delta)
    assert abs(d["prob"] - s.prob) <= 1e-12 * abs(s.prob)
    pyr.close()
    ctx.map_release(FINE)


@pytest.fixture
def stations_scene(pkg, ctx):
    """the many-to-many golden resident on the device: map j (the origin, N1, N2, N3) is map id 40 j with its levels
    behind it, request k's scan in slot k"""
    s = placed_many_scene()
    pyr = []
    for j, m in enumerate(s.maps):
        ctx.upload_map(ID_STRIDE * j, m)
        pyr.append(pkg.Pyramid(ctx, ID_STRIDE * j, s.oie, ID_STRIDE * j + 1))
    for k, r in enumerate(s.requests):
        ctx.scan_store(k, r.scan[:, 0], r.scan[:, 1], r.scan[:, 2], r.scan[:, 3], r.scan[:, 4])
    s.pyr = pyr
    s.table = [(pyr[r.map], k, r.pose) for k, r in enumerate(s.requests)]
    assert [len(p.info()) for p in pyr] == [6, 12, 12, 12]
    yield s
    for p in pyr:
        p.close()
    for j in range(len(s.maps)):
        ctx.map_release(ID_STRIDE * j)


def test_many_to_many_over_four_stations_is_the_references_shared_search(pkg, ctx, stations_scene):
    s = stations_scene
    mt = pkg.Matcher(ctx, "BF_M3RSM", m3rsm_cfg(pkg, s.oie, True), [s.pyr[0], *s.limits])
    r = mt.m3rsm_match_many(s.table)
    np.testing.assert_array_equal(bits(mt.m3rsm_trace_many()), bits(s.trace))
    assert r["request"] == s.winner != 0 and r["prob"] == s.prob
    np.testing.assert_array_equal(bits(r["delta"]), bits(s.delta))
    mt.close()
    mt = pkg.Matcher(ctx, "BF_M3RSM", m3rsm_cfg(pkg, s.oie, False), [s.pyr[0], *s.limits])
    d = mt.m3rsm_match_many(s.table)
    assert d["request"] == s.winner and abs(d["prob"] - s.prob) <= 1e-12 * abs(s.prob)
    np.testing.assert_array_equal(d["delta"], s.delta)
    mt.close()


@pytest.mark.parametrize("threads", [1, 4])
def test_independent_matches_at_four_stations_are_the_references_lone_matches(pkg, ctx, stations_scene, threads):
    s = stations_scene
    mt = pkg.Matcher(ctx, "BF_M3RSM", m3rsm_cfg(pkg, s.oie, True), [s.pyr[0], *s.limits])
    mt.set_m3rsm_threads(threads)
    got = mt.m3rsm_match_each(s.table)
    for k, g in enumerate(got):  # lone [K, 5]: delta, prob, calls of the reference's lone match of request k
        np.testing.assert_array_equal(bits(g["delta"]), bits(s.lone[k, :3]), err_msg="request %d" % k)
        assert g["prob"] == s.lone[k, 3] and mt.m3rsm_each_stats(k)["scorer_calls"] == s.lone[k, 4]
    mt.close()
    mt = pkg.Matcher(ctx, "BF_M3RSM", m3rsm_cfg(pkg, s.oie, False), [s.pyr[0], *s.limits])
    mt.set_m3rsm_threads(threads)
    for k, g in enumerate(mt.m3rsm_match_each(s.table)):
        np.testing.assert_array_equal(g["delta"], s.lone[k, :3])
        assert abs(g["prob"] - s.lone[k, 3]) <= 1e-12 * abs(s.lone[k, 3])
    mt.close()


# ---- the reference's default trig provider (SLAMHIP_POSE_TRIG_RAW_EXACT) far out: no reference, the route's own inputs ---------
@pytest.fixture(scope="module")
def variant(pkg):
    v = pkg.libm_variant()
    if v < 0:
        pytest.skip("this host's libm is neither build of glibc's sin / cos / exp: no exact modes here")
    return v


def test_strict_mode_is_the_references_match_under_its_default_provider_at_n1(pkg, ctx, variant):
    """placed_pyramid.npz raw_*: the edge scene (end points on cell edges, directions exactly (1, 0) at every other
    rotation) 1000 cells out, under RawTrigonometryProvider: the trace call for call, as tests/test_gpu_m3rsm_rawtrig.py
    holds it next to the origin"""
    s = placed_raw_scene()
    pyr = upload(pkg, ctx, s, s)
    ctx.scan_set_angles(s.angle)
    raw = dict(oope=pkg.OOPE_MAX, oie=s.oie, pose_trig=pkg.POSE_TRIG_RAW_EXACT)
    r, trace = lone_match(pkg, ctx, pyr, FINE, s.oie, True, s.pose, s.limits, cfg=pkg.spe_cfg(sum_order=pkg.SUM_SEQUENTIAL, **raw))
    print("%s at N1: %d calls (cached provider: %d), libm variant %d (golden %d)"
          % (s.name, len(trace), s.n_cached_calls, variant, s.libm_variant))
    np.testing.assert_array_equal(bits(trace), bits(s.trace))
    np.testing.assert_array_equal(bits(r["delta"]), bits(s.delta))
    assert r["prob"] == s.prob
    d, _ = lone_match(pkg, ctx, pyr, FINE, s.oie, False, s.pose, s.limits, cfg=pkg.spe_cfg(sum_order=pkg.SUM_TREE256, **raw))
    np.testing.assert_array_equal(d["delta"], s.delta)
    assert abs(d["prob"] - s.prob) <= 1e-12 * abs(s.prob)
    pyr.close()
    ctx.map_release(FINE)


@pytest.mark.parametrize("st", ["O", "Q3", "F1", "N2"])
@pytest.mark.parametrize("i", FAR_MAPS)
def test_a_far_match_under_the_raw_provider_scores_its_inputs_and_walks_its_tree(pkg, ctx, po, oracle, variant, i, st):
    """The tabulation of glibc's cos / sin((rotation + heading) + angle) per distinct rotation, through the bound and the
    expand launches of a whole match: every traced score against score_poses under the same provider on the traced
    level's map id and against the ORACLE's raw provider on the downloaded level, bit for bit; the trace a tree."""
    m, s = moved_set(i, st)
    pyr = upload(pkg, ctx, m, s)
    angle = np.arctan2(s.scan[:, 2], s.scan[:, 1])
    ctx.scan_set_angles(angle)
    ids = pyr.level_map_ids()
    raw = dict(oope=pkg.OOPE_MAX, oie=m.oie, sum_order=pkg.SUM_SEQUENTIAL, pose_trig=pkg.POSE_TRIG_RAW_EXACT)
    r, trace = lone_match(pkg, ctx, pyr, FINE, m.oie, True, s.pose, cfg=pkg.spe_cfg(**raw))
    assert_trace_is_a_tree_with_its_result(pkg, trace, r)
    rot, rect, score, level = trace[:, 0], trace[:, 1:5], trace[:, 5], trace[:, 6].astype(int)
    poses = poses_of(s.pose, rot, rect)
    want = np.array([ctx.score_poses(ids[level[k]], pkg.spe_cfg(area=rect[k], **raw), poses[k:k + 1])[0] for k in range(len(trace))])
    np.testing.assert_array_equal(bits(score), bits(want))
    if i in ORACLE_MAPS:
        levels = [dict(origin=m.origin, scale=m.scale, payload=m.payload)] + download_levels(ctx, pyr, pkg.STRIDE[m.cell_model])
        plain = [po.GridMapData(m.cell_model, lv["payload"], lv["origin"], lv["scale"], m.unknown) for lv in levels]
        rawscan = po.ScanData(s.scan[:, 0], angle, s.scan[:, 3], s.scan[:, 4])
        want = np.array([oracle.score_poses(plain[level[k]], rawscan, po.make_cfg(oope=po.OOPE_MAX, oie=m.oie, area=tuple(rect[k])), poses[k:k + 1])[0]
                         for k in range(len(trace))])
        np.testing.assert_array_equal(bits(score), bits(want))
    assert len(np.unique(rot)) == 11  # one row of the table per distinct rotation of the root layer
    pyr.close()
    ctx.map_release(FINE)


class FiveRequests:
    """K = 5 requests at O, Q2, Q4, F1 and N1, each over its own pyramid (6, 16, 16, 23 and 12 levels) of map 64 moved
    there, with scans of 67, 1, 65, 257 and 67 beams in the slots 0 ... 4"""
    STATIONS = ["O", "Q2", "Q4", "F1", "N1"]

    def __init__(self, pkg, ctx):
        from test_gpu_m3rsm import synthetic_scan
        self.pkg, self.ctx, self.pyr, self.table, self.fine = pkg, ctx, [], [], []
        for k, (st, n) in enumerate(zip(self.STATIONS, (None, 1, 65, 257, None))):
            m, s = moved_set(64, st)
            self.oie = m.oie
            scan = s.scan if n is None else np.column_stack(synthetic_scan(n, 11 + n))
            if n is not None:
                scan[:, 0] *= 0.6  # (the ranges stay inside the map)
            ctx.upload_map(ID_STRIDE * k, m)
            self.pyr.append(pkg.Pyramid(ctx, ID_STRIDE * k, m.oie, ID_STRIDE * k + 1))
            ctx.scan_store(k, scan[:, 0], scan[:, 1], scan[:, 2], scan[:, 3], scan[:, 4])
            self.table.append((self.pyr[k], k, s.pose + np.array([0.01 * k, -0.02 * k, 0.004 * k])))
            self.fine.append(ID_STRIDE * k)
        assert [len(p.info()) for p in self.pyr] == [6, 16, 16, 23, 12]

    def lone(self, strict):
        out = []
        for k, (pyr, slot, pose) in enumerate(self.table):
            self.ctx.scan_select(slot)
            out.append(lone_match(self.pkg, self.ctx, pyr, self.fine[k], self.oie, strict, pose))
        return out

    def close(self):
        for p in self.pyr:
            p.close()
        for f in self.fine:
            self.ctx.map_release(f)


@pytest.fixture
def five(pkg, ctx):
    f = FiveRequests(pkg, ctx)
    yield f
    f.close()


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "default"])
def test_match_each_over_five_stations_is_the_lone_match_per_request(pkg, ctx, five, strict):
    lone = five.lone(strict)
    if strict:
        for r, trace in lone:
            assert_trace_is_a_tree_with_its_result(pkg, trace, r)
    mt = pkg.Matcher(ctx, "BF_M3RSM", m3rsm_cfg(pkg, five.oie, strict), [five.pyr[0], *LIMITS])
    for threads in (1, 4):
        mt.set_m3rsm_threads(threads)
        got = mt.m3rsm_match_each(five.table)
        for k, (r, trace) in enumerate(lone):
            np.testing.assert_array_equal(bits(got[k]["delta"]), bits(r["delta"]), err_msg=five.STATIONS[k])
            np.testing.assert_array_equal(bits([got[k]["prob"]]), bits([r["prob"]]), err_msg=five.STATIONS[k])
            np.testing.assert_array_equal(bits(mt.m3rsm_trace_each(k)), bits(trace), err_msg=five.STATIONS[k])
    assert len({r["prob"] for r, _ in lone}) == 5 and all(np.isfinite(r["prob"]) for r, _ in lone)
    # many-to-many over the same table: ONE search, which ends at the request whose lone match is the most probable
    many = mt.m3rsm_match_many(five.table)
    k_best = int(np.argmax([r["prob"] for r, _ in lone]))
    assert many["request"] == k_best and many["prob"] == lone[k_best][0]["prob"]
    np.testing.assert_array_equal(bits(many["delta"]), bits(lone[k_best][0]["delta"]))
    mt.close()


def test_request_launches_over_five_stations_equal_the_single_request_launches(pkg, ctx, five):
    from test_gpu_m3rsm import PARENTS, STEP
    n = 45
    rect = PARENTS[np.arange(n) % len(PARENTS)]
    rot = np.random.RandomState(5).uniform(-0.1, 0.1, n)
    req = (np.arange(n) * 7 + np.arange(n) // 9) % 5
    assert {(int(a), int(b)) for a, b in zip(req, np.arange(n) % len(PARENTS))} == {(a, b) for a in range(5) for b in range(len(PARENTS))}
    ok = (rect[:, 0] <= rect[:, 1]) & (rect[:, 2] <= rect[:, 3])
    for strict in (True, False):
        cfg = m3rsm_cfg(pkg, five.oie, strict)
        for depth in (1, 3):
            got = pkg.Pyramid.expand_requests(ctx, cfg, five.table, req, rot, rect, STEP, depth)
            for k, (pyr, slot, pose) in enumerate(five.table):
                mine = req == k
                ctx.scan_select(slot)
                want = pyr.expand_matches(cfg, pose, rot[mine], rect[mine], STEP, depth)
                for g, w in zip(got, want):
                    np.testing.assert_array_equal(bits(g[mine].astype(np.float64)), bits(w.astype(np.float64)), err_msg=five.STATIONS[k])
                assert np.isfinite(want[1]).sum() > 0
        got_score, got_level = pkg.Pyramid.score_requests(ctx, cfg, five.table, req[ok], rot[ok], rect[ok])
        for k, (pyr, slot, pose) in enumerate(five.table):
            mine = req[ok] == k
            ctx.scan_select(slot)
            want_score, want_level = pyr.score_matches(cfg, pose, rot[ok][mine], rect[ok][mine])
            np.testing.assert_array_equal(bits(got_score[mine]), bits(want_score), err_msg=five.STATIONS[k])
            np.testing.assert_array_equal(got_level[mine], want_level)


@pytest.mark.parametrize("st", ["Q3", "F1"])
@pytest.mark.parametrize("i", FAR_MAPS)
def test_expand_matches_equals_score_matches_on_host_splits_far_out(pkg, ctx, i, st):
    from test_gpu_m3rsm import PARENTS, STEP
    m, s = moved_set(i, st)
    pyr = upload(pkg, ctx, m, s)
    n = 27
    rect = PARENTS[np.arange(n) % len(PARENTS)]
    rot = np.random.RandomState(3).uniform(-0.1, 0.1, n)
    for depth in (1, 2, 3):
        want_rect = np.stack([host_slots(r, STEP, depth) for r in rect])
        there = ~np.isnan(want_rect[..., 0])
        for strict in (True, False):
            cfg = m3rsm_cfg(pkg, m.oie, strict)
            got_rect, got_score, got_level = pyr.expand_matches(cfg, s.pose, rot, rect, STEP, depth)
            np.testing.assert_array_equal(bits(got_rect[there]), bits(want_rect[there]))
            assert np.all(np.isnan(got_rect[~there])) and np.all(np.isnan(got_score[~there])) and np.all(got_level[~there] == -1)
            slot_rot = np.broadcast_to(rot[:, None], there.shape)[there]
            want_score, want_level = pyr.score_matches(cfg, s.pose, slot_rot, want_rect[there])
            np.testing.assert_array_equal(bits(got_score[there]), bits(want_score))
            np.testing.assert_array_equal(got_level[there], want_level)
            assert np.all(np.isfinite(want_score))
    pyr.close()
    ctx.map_release(FINE)


@pytest.mark.parametrize("st", ["Q3", "F1"])
def test_a_match_after_refresh_of_a_far_pyramid_equals_a_match_over_a_fresh_one(pkg, ctx, st):
    m, s = moved_set(66, st)
    pyr = upload(pkg, ctx, m, s)
    before, trace_before = lone_match(pkg, ctx, pyr, FINE, m.oie, True, s.pose)
    # the scan written into the map at half its ranges from a pose beside the true one (so that every beam ends inside the
    # 37 x 29 window): walls where there were none, impacts change on every level
    pose = s.pose + np.array([0.1, -0.1, 0.06])
    assert ctx.map_append_scan(FINE, pkg.RULE_TBM, pose, 0.5 * s.scan[:, 0], s.scan[:, 1], s.scan[:, 2]) > 0
    assert ctx.map_info(FINE)["origin"] == m.origin  # (the map did not grow)
    pyr.refresh(0, 0, m.width, m.height)
    after, trace_after = lone_match(pkg, ctx, pyr, FINE, m.oie, True, s.pose)
    assert len(trace_after) != len(trace_before) or not np.array_equal(bits(trace_after), bits(trace_before))
    pyr.close()
    pyr = pkg.Pyramid(ctx, FINE, m.oie, FIRST)
    fresh, trace_fresh = lone_match(pkg, ctx, pyr, FINE, m.oie, True, s.pose)
    np.testing.assert_array_equal(bits(trace_after), bits(trace_fresh))
    np.testing.assert_array_equal(bits(after["delta"]), bits(fresh["delta"]))
    assert after["prob"] == fresh["prob"] and np.isfinite(before["prob"])
    pyr.close()
    ctx.map_release(FINE)
