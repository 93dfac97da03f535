"""GPU suite: K6 map update on windows that are NO squares, touched far from their middle -- every pipeline
(SLAMHIP_OPT_K6_PATH gather / counting / radix), the window's growth and the per-particle tile pool.

Everything else the suite binds for a map update is symmetric in x and y: square windows, equal origin components,
the robot next to the world origin.  An exchange of width and height, of origin_x and origin_y, of the robot cell's
two internal coordinates or of the key window's two sides passes all of it.  Here every window has width != height,
origin_x != origin_y and a width that is no multiple of 16 (pitch != width):
  a. tests/golden/map_update_oblong.npz (the compiled reference on 203 x 131 cells, robot near (+4.3, -2.1) m) at the
     bars of test_gpu_mapupdate.py (cached provider) and test_gpu_libm_exact.py (raw provider: bit for bit);
  b. the same on the golden's crop box bound as its own map: origin (-13, 42) in 60 x 40 cells -- negative in x,
     beyond the extent in y;
  c. beams that leave a 77 x 45 window across each rim and each corner: the documented error, and the cells inside
     the window updated exactly like the oracle's on a window that holds everything;
  d. key windows one cell high, one cell wide and of one cell;
  e. growth from a 21 x 13 window against the oracle on a fixed one;
  f. the tile pool seeded from a 150 x 70 ancestor, growing by a tile column and by no row.
The oracle is pinned to the reference on the same geometry by tests/test_oracle_mapupdate_oblong.py; where it is the
expected value its trigonometry is the device's (a cached provider with one table entry per beam), so the bar is
assert_array_equal."""
import numpy as np
import pytest
from mapupdate_oblong_cases import (AUX_STRIDE, MODELS, RUN_IDS, RUNS, STRIDE, UNKNOWN, fresh_map, geometry, golden,
                                    oracle_step, step_args, tag)

import __graft_entry__ as ge

pytestmark = pytest.mark.gpu

K6_PATHS = {"gather": 0, "counting": 1, "radix": 2}
AUX = AUX_STRIDE  # rule -> update counters per cell
SCALE = 0.1
RIM_W, RIM_H, RIM_ORIGIN = 77, 45, (9, 31)


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
def _default_k6_path(pkg, ctx):
    yield
    ctx.set_option(pkg.OPT_K6_PATH, K6_PATHS["gather"])


def one_entry_per_beam(pkg, rng, ang):
    """The scan for the oracle with the device's arithmetic: a cached trigonometry provider whose table holds the
    device's per-beam cos / sin, one entry per beam (test_append_scan_full_size_vs_oracle_and_rescoring)."""
    import pyoracle as po
    c, s = pkg.beam_trig(ang)
    tr = po.ScanData(rng, ang, None, None, po.TRIG_CACHED, 0.0, 1.0, s, c)
    tr.angle = np.arange(len(rng), dtype=np.float64)  # index == beam
    return c, s, tr


def bind_fresh(pkg, ctx, map_id, *geometry):
    """map_bind on an id that holds nothing: a test that failed before its map_release leaves its window bound, and a
    re-bind alone keeps the cells of a bound window at their external place -- the next test would start from them."""
    try:
        ctx.map_release(map_id)
    except pkg.SlamHipError:
        pass  # (nothing bound under this id: the usual case)
    ctx.map_bind(map_id, *geometry)


def oracle_map(cell_model, width, height, origin, n_aux):
    import pyoracle as po
    unknown = UNKNOWN[cell_model]
    payload = np.empty((height, width, STRIDE[cell_model]))
    payload[:] = unknown
    return po.GridMapData(cell_model, payload, origin, SCALE, unknown), (np.zeros((height, width, n_aux)) if n_aux else None)


# ---- a, b: the reference's golden, full window and re-based crop box ---------------------------------------------------
def _golden_on_device(pkg, ctx, oracle, name, est, path, window, raw):
    g = golden()
    ctx.set_option(pkg.OPT_K6_PATH, K6_PATHS[path])
    cell_model, rule = MODELS[name]
    st = STRIDE[cell_model]
    w, h, origin = geometry(g, name, window)
    assert w != h and origin[0] != origin[1] and w % 16
    bind_fresh(pkg, ctx, 2, cell_model, w, h, origin, float(g["scale"]), g[name + "_unknown"][:st])
    x0, y0, x1, y1 = [int(v) for v in g["crop"]] if window == "full" else (0, 0, w, h)
    m, aux, _ = fresh_map(g, name, window)  # the oracle alongside: the update counts
    for k in range(int(g["n_steps"])):
        kw, ex = step_args(g, name, est, k)
        if est:
            kw.update(estimator=1, shift_amount=ex["shift_amount"])
        pose, rng, ang, occ = g["step%d_pose" % k], g["step%d_range" % k], g["step%d_angle" % k], g["step%d_occ" % k]
        if raw:
            nu = ctx.map_append_scan_raw(2, rule, pose, rng, ang, occ, **kw)
        else:
            c, s = pkg.beam_trig(ang)
            nu = ctx.map_append_scan(2, rule, pose, rng, c, s, occ, **kw)
        assert nu == oracle_step(oracle, g, name, est, k, m, aux, rule) > 1000
        got = ctx.map_download_window(2, x0, y0, x1 - x0, y1 - y0, st)
        want = g[tag(name, est, k) + "payload"]
        msg = "%s step %d" % (name, k)
        if raw:
            np.testing.assert_array_equal(got, want, err_msg=msg)
        elif est:
            # the area split depends continuously on the end point: raw-provider end points of the reference differ
            # from the angle-addition form in the last ulp (test_gpu_mapupdate.py's bar)
            np.testing.assert_allclose(got, want, rtol=1e-11, atol=1e-13, err_msg=msg)
        elif name == "gmapping":
            np.testing.assert_array_equal(got[..., 0], want[..., 0], err_msg=msg)
            np.testing.assert_allclose(got[..., 1:], want[..., 1:], rtol=1e-13, atol=1e-15, err_msg=msg)  # obstacle means
        else:
            np.testing.assert_array_equal(got, want, err_msg=msg)
        if rule in AUX:
            np.testing.assert_array_equal(ctx.map_download_aux(2, x0, y0, x1 - x0, y1 - y0, AUX[rule]),
                                          g[tag(name, est, k) + "aux"], err_msg=msg)
    if window == "full":  # nothing outside the crop box: an update in the wrong place would show here
        whole = ctx.map_download_window(2, 0, 0, w, h, st)
        outside = np.ones((h, w), bool)
        outside[y0:y1, x0:x1] = False
        assert (whole[outside] == g[name + "_unknown"][:st]).all()
        if rule in AUX:
            assert not ctx.map_download_aux(2, 0, 0, w, h, AUX[rule])[outside].any()
    ctx.map_release(2)


@pytest.mark.parametrize("window", ["full", "crop"])
@pytest.mark.parametrize("path", list(K6_PATHS))
@pytest.mark.parametrize("name,est", RUNS, ids=RUN_IDS)
def test_append_scan_oblong_vs_reference_golden(pkg, ctx, oracle, name, est, path, window):
    """map_append_scan (the cached provider's angle addition) at test_gpu_mapupdate.py's bars: const estimator bit for
    bit but GMapping's obstacle means (1e-13), area estimator 1e-11, counters and update counts exact."""
    _golden_on_device(pkg, ctx, oracle, name, est, path, window, raw=False)


@pytest.mark.parametrize("window", ["full", "crop"])
@pytest.mark.parametrize("path", list(K6_PATHS))
@pytest.mark.parametrize("name,est", RUNS, ids=RUN_IDS)
def test_append_scan_raw_oblong_vs_reference_golden_bit_for_bit(pkg, ctx, oracle, variant, name, est, path, window):
    """map_append_scan_raw (the reference's own cos / sin(theta + a)): assert_array_equal throughout."""
    _golden_on_device(pkg, ctx, oracle, name, est, path, window, raw=True)


# ---- c: beams that leave the window, every rim and every corner --------------------------------------------------------
def rim_placements():
    """Internal robot cells two cells inside each rim and each corner of the RIM_W x RIM_H window."""
    lo, hx, hy, mx, my = 2, RIM_W - 3, RIM_H - 3, RIM_W // 2, RIM_H // 2
    return {"left": (lo, my), "right": (hx, my), "bottom": (mx, lo), "top": (mx, hy),
            "bottom-left": (lo, lo), "bottom-right": (hx, lo), "top-left": (lo, hy), "top-right": (hx, hy)}


RIM_COMBOS = [(name, path, 0) for name in ("mean", "tbm", "gmapping") for path in K6_PATHS] + \
             [(name, "gather", 1) for name in ("mean", "tbm", "gmapping")]


@pytest.mark.parametrize("name,path,est", RIM_COMBOS, ids=["%s-%s-%s" % (n, p, "area" if e else "const") for n, p, e in RIM_COMBOS])
def test_beams_across_every_rim_update_the_cells_inside(pkg, ctx, oracle, name, path, est):
    """slamhip_map_append_scan's contract for a beam that leaves the bound window: SLAMHIP_ERR_STATE, "cells inside the
    window were updated".  64 beams over 360 degrees, 0.3 ... 3 m, from two cells inside each rim and each corner of a
    77 x 45 window with origin (9, 31): some beams stay inside, some cross one rim, at a corner two.  Expected: the oracle
    on a window 40 cells larger on every side, cropped.  Then a scan that stays inside, on the same context.

    What keeps a rim-crossing record off memory outside the allocation:
      * gather: k_mu_cells stores only cells of the key window, which the host clips to the map (wx0 .. wy1) -- a far
        thread is `inside` only below key_x0 + key_w / key_y0 + key_h, a near wave only within all four sides; an
        irregular beam's cells pass `oob = ix >= w || iy >= h` on unsigned internal coordinates (map_update_gather.h)
        before they become keys or marker words, everything else is the padding key ~0;
      * counting: k_mu_emit and the sequential walks turn every cell with `ix >= w || iy >= h` (unsigned: negative
        coordinates too) into the padding key ~0, which is no bin of the clipped key window: k_mu_scatter / k_mu_rank
        see only keys < n_bins, and the apply kernels decode those back into cells of the map;
      * radix: the same `oob` test with the whole map as key window (key = iy * pitch + ix < pitch * height); ~0 sorts
        behind every valid key and k_mu_gather / the apply kernels stop at it."""
    from pyoracle_mapupdate import append_scan_ex
    ctx.set_option(pkg.OPT_K6_PATH, K6_PATHS[path])
    cell_model, rule = MODELS[name]
    st, n_aux = STRIDE[cell_model], AUX.get(rule, 0)
    pad = 40
    rs = np.random.RandomState(41)
    ang = np.deg2rad(np.linspace(-180.0, 180.0, 64, endpoint=False))
    ex_o = dict(est_kind=1, shift_amount=0.01 * SCALE) if est else {}
    ex_d = dict(estimator=1, shift_amount=0.01 * SCALE) if est else {}
    for where, (rx, ry) in rim_placements().items():
        for blur in (0.3, 0.0):
            msg = "%s, blur %g" % (where, blur)
            pose = np.array([(rx - RIM_ORIGIN[0] + 0.37) * SCALE, (ry - RIM_ORIGIN[1] + 0.61) * SCALE, 0.3])
            rng = rs.uniform(0.3, 3.0, ang.size)
            occ = (rs.rand(ang.size) < 0.8).astype(np.int32)
            ex = np.floor((pose[0] + rng * np.cos(ang + pose[2])) / SCALE) + RIM_ORIGIN[0]
            ey = np.floor((pose[1] + rng * np.sin(ang + pose[2])) / SCALE) + RIM_ORIGIN[1]
            n_in = np.count_nonzero((ex >= 0) & (ex < RIM_W) & (ey >= 0) & (ey < RIM_H))
            assert 8 <= n_in <= ang.size - 8, msg  # some beams stay inside, some cross
            m, aux = oracle_map(cell_model, RIM_W + 2 * pad, RIM_H + 2 * pad, (RIM_ORIGIN[0] + pad, RIM_ORIGIN[1] + pad), n_aux)
            c, s, tr = one_entry_per_beam(pkg, rng, ang)
            append_scan_ex(oracle, m, aux, rule, pose, rng, tr.angle, occ, quality=0.9, blur=blur, trig=tr, **ex_o)
            beyond = m.payload.copy()
            beyond[pad:pad + RIM_H, pad:pad + RIM_W] = UNKNOWN[cell_model]
            assert np.count_nonzero((beyond != UNKNOWN[cell_model]).any(axis=2)) > 50, msg  # the oracle did go beyond the rim
            bind_fresh(pkg, ctx, 3, cell_model, RIM_W, RIM_H, RIM_ORIGIN, SCALE, UNKNOWN[cell_model])
            with pytest.raises(pkg.SlamHipError, match=r"slamhip error -4: .*a beam leaves the bound map window"):
                ctx.map_append_scan(3, rule, pose, rng, c, s, occ, quality=0.9, blur=blur, **ex_d)
            for rnd in range(2):
                got = ctx.map_download_window(3, 0, 0, RIM_W, RIM_H, st)
                np.testing.assert_array_equal(got, m.payload[pad:pad + RIM_H, pad:pad + RIM_W], err_msg=msg)
                if n_aux:
                    np.testing.assert_array_equal(ctx.map_download_aux(3, 0, 0, RIM_W, RIM_H, n_aux),
                                                  aux[pad:pad + RIM_H, pad:pad + RIM_W], err_msg=msg)
                if rnd == 0:
                    # a following scan that stays inside updates correctly: 16 beams into the quadrant that points away
                    # from the rims, 5 cells ... as far as that quadrant has room (21 ... 30 cells: near cells, far
                    # cells, records of every pipeline on the first call after the error)
                    sx, sy = (1 if rx < RIM_W / 2 else -1), (1 if ry < RIM_H / 2 else -1)
                    room = min(RIM_W - 1 - rx if sx > 0 else rx, RIM_H - 1 - ry if sy > 0 else ry)
                    t = np.deg2rad(np.linspace(5.0, 85.0, 16))
                    ang2 = np.arctan2(sy * np.sin(t), sx * np.cos(t)) - pose[2]
                    rng2 = np.linspace(0.5, min(3.0, (room - 1) * SCALE), 16)[::-1].copy()
                    assert rng2.max() > 1.7  # (beyond the 16 cells around the robot the counting form keeps bitmaps for)
                    c2, s2, tr2 = one_entry_per_beam(pkg, rng2, ang2)
                    nu_o = append_scan_ex(oracle, m, aux, rule, pose, rng2, tr2.angle, None, quality=0.8, blur=blur, trig=tr2,
                                          **ex_o)
                    assert ctx.map_append_scan(3, rule, pose, rng2, c2, s2, None, quality=0.8, blur=blur, **ex_d) == nu_o
            ctx.map_release(3)  # (a re-bind alone would keep the cells)


# ---- d: key windows one cell high, one cell wide, one cell -------------------------------------------------------------
@pytest.mark.parametrize("path", list(K6_PATHS))
@pytest.mark.parametrize("name", list(MODELS))
def test_key_windows_of_one_row_one_column_and_one_cell(pkg, ctx, oracle, name, path):
    """Scans whose beams all run along one axis from a cell centre: the key window between the robot's cell and the end
    cells is 1 cell high or 1 cell wide and 22 ... 47 cells long (the gather form's far_blocks = tiles_x * tiles_y with
    one factor 1); a scan of zero-length beams: a window of one cell.  Payload, counters and update counts = the oracle's."""
    from pyoracle_mapupdate import append_scan_ex
    ctx.set_option(pkg.OPT_K6_PATH, K6_PATHS[path])
    cell_model, rule = MODELS[name]
    st, n_aux = STRIDE[cell_model], AUX.get(rule, 0)
    rix, riy = 30, 22  # internal robot cell: 46 cells to the right rim, 30 to the left, 22 up and down
    pose = np.array([(rix - RIM_ORIGIN[0] + 0.5) * SCALE, (riy - RIM_ORIGIN[1] + 0.5) * SCALE, 0.0])
    m, aux = oracle_map(cell_model, RIM_W, RIM_H, RIM_ORIGIN, n_aux)
    bind_fresh(pkg, ctx, 3, cell_model, RIM_W, RIM_H, RIM_ORIGIN, SCALE, UNKNOWN[cell_model])
    n = 33
    scans = [(np.full(n, a), np.linspace(1.7, reach, n)) for a, reach in
             ((0.0, 4.6), (np.pi, 2.9), (np.pi / 2, 2.2), (-np.pi / 2, 2.2))] + [(np.linspace(-3.0, 3.0, n), np.zeros(n))]
    for k, (ang, rng) in enumerate(scans):
        occ = (np.arange(n) % 4 != 1).astype(np.int32)
        c, s, tr = one_entry_per_beam(pkg, rng, ang)
        # the key window the host will build: robot cell .. end cells
        ex = np.floor((pose[0] + rng * c) / SCALE).astype(int) + RIM_ORIGIN[0]
        ey = np.floor((pose[1] + rng * s) / SCALE).astype(int) + RIM_ORIGIN[1]
        kw_, kh_ = max(ex.max(), rix) - min(ex.min(), rix) + 1, max(ey.max(), riy) - min(ey.min(), riy) + 1
        assert (kw_, kh_) == [(47, 1), (30, 1), (1, 23), (1, 23), (1, 1)][k]
        nu_o = append_scan_ex(oracle, m, aux, rule, pose, rng, tr.angle, occ, quality=0.9, blur=0.3, trig=tr)
        nu = ctx.map_append_scan(3, rule, pose, rng, c, s, occ, quality=0.9, blur=0.3)
        assert nu == nu_o, "scan %d" % k
        np.testing.assert_array_equal(ctx.map_download_window(3, 0, 0, RIM_W, RIM_H, st), m.payload, err_msg="scan %d" % k)
        if n_aux:
            np.testing.assert_array_equal(ctx.map_download_aux(3, 0, 0, RIM_W, RIM_H, n_aux), aux, err_msg="scan %d" % k)
    ctx.map_release(3)


# ---- e: growth from an oblong start ------------------------------------------------------------------------------------
GROW_COMBOS = [(name, path, 0) for name in ("mean", "tbm", "gmapping") for path in K6_PATHS] + \
              [("mean", "gather", 1), ("tbm", "counting", 1), ("gmapping", "radix", 1)]


@pytest.mark.parametrize("name,path,est", GROW_COMBOS, ids=["%s-%s-%s" % (n, p, "area" if e else "const") for n, p, e in GROW_COMBOS])
def test_window_grows_from_an_oblong_start_like_the_oracles_fixed_window(pkg, ctx, oracle, name, path, est):
    """slamhip_map_set_auto_grow from 21 x 13 cells with origin (3, 10): the crafted scans of test_gpu_mapupdate_edges
    make the window grow on every side, by different amounts in x and y.  Expected: the oracle on a fixed 400 x 400
    window -- equal cells by external coordinate, the prototype everywhere else, payload and counters."""
    from pyoracle_mapupdate import append_scan_ex
    from test_gpu_mapupdate_edges import crafted_scans
    ctx.set_option(pkg.OPT_K6_PATH, K6_PATHS[path])
    cell_model, rule = MODELS[name]
    st, n_aux = STRIDE[cell_model], AUX.get(rule, 0)
    size = 400
    m, aux = oracle_map(cell_model, size, size, (size // 2, size // 2), n_aux)
    bind_fresh(pkg, ctx, 4, cell_model, 21, 13, (3, 10), SCALE, UNKNOWN[cell_model])
    ctx.map_set_auto_grow(4, True)
    ex_o = dict(est_kind=1, shift_amount=0.01 * SCALE) if est else {}
    ex_d = dict(estimator=1, shift_amount=0.01 * SCALE) if est else {}
    for k, (pose, rng, ang, occ, blur, max_range) in enumerate(crafted_scans()):
        c, s, tr = one_entry_per_beam(pkg, rng, ang)
        nu_o = append_scan_ex(oracle, m, aux, rule, pose, rng, tr.angle, occ, quality=0.8, blur=blur, max_range=max_range,
                              trig=tr, **ex_o)
        nu = ctx.map_append_scan(4, rule, pose, rng, c, s, occ, quality=0.8, blur=blur, max_range=max_range, **ex_d)
        assert nu == nu_o, "scan %d" % k
    info = ctx.map_info(4)
    W, H = info["width"], info["height"]
    ox, oy = info["origin"]
    assert info["times_grown"] >= 2 and W != H and W > 21 and H > 13 and info["cell_model"] == cell_model
    got = ctx.map_download_window(4, 0, 0, W, H, st)
    x0, y0 = size // 2 - ox, size // 2 - oy  # fixed-window coordinates of the grown window's cell (0, 0)
    bx0, by0, bx1, by1 = max(x0, 0), max(y0, 0), min(x0 + W, size), min(y0 + H, size)
    assert bx1 - bx0 > 150 and by1 - by0 > 150
    np.testing.assert_array_equal(got[by0 - y0:by1 - y0, bx0 - x0:bx1 - x0], m.payload[by0:by1, bx0:bx1])
    outside = np.ones((size, size), bool)
    outside[by0:by1, bx0:bx1] = False
    assert (m.payload[outside] == np.array(UNKNOWN[cell_model])).all()  # the oracle touched nothing the window lacks
    inside = np.zeros((H, W), bool)
    inside[by0 - y0:by1 - y0, bx0 - x0:bx1 - x0] = True
    assert (got[~inside] == np.array(UNKNOWN[cell_model])).all()
    if n_aux:
        got_aux = ctx.map_download_aux(4, 0, 0, W, H, n_aux)
        np.testing.assert_array_equal(got_aux[by0 - y0:by1 - y0, bx0 - x0:bx1 - x0], aux[by0:by1, bx0:bx1])
        assert not aux[outside].any() and not got_aux[~inside].any()
    ctx.map_release(4)


# ---- f: the tile pool --------------------------------------------------------------------------------------------------
def _tile_positions(blob):
    """External (x, y) of the first cell of every tile a particle's exported map refers to (the export's header)."""
    n = int(np.frombuffer(blob[:8].tobytes(), np.int64)[0])
    ent = np.frombuffer(blob[8:8 + 16 * n].tobytes(), np.int32).reshape(n, 4)
    return ent[:, 0], ent[:, 1]


@pytest.mark.parametrize("mode", ["fast", "sorted", "key64"])
def test_tile_pool_from_an_oblong_ancestor_grows_unevenly(pkg, oracle, mode):
    """Per-particle maps seeded from a 150 x 70 window with origin (20, 50) that holds one scan from (+4.3, -2.1).  The
    pool refuses an ancestor its start extent does not hold (test_particle_maps_argument_checks), and this one is wider
    than a tile (128 x 128 cells) and lies off the extent's middle: extent_tiles = 3 is the smallest square extent that
    takes it (its virtual columns 172 ... 321 of 384).  Three particles around (+9, -2) append a scan whose beams along
    +x are 9 ... 11 m long -- beyond the extent's right rim, which grows by a tile column and by no row --, then one
    from around (+4, +6): tile_pool_grow / tile_pool_make_private with different counts in x and y, in the default
    batch pipeline, the fully sorted one and the one with 8-byte keys.
    Expected: the oracle's private dense maps (run_both's bars: occupancy and counters exact, obstacle means 1e-12)."""
    import pyoracle as po
    from pyoracle_mapupdate import (RULE_GMAPPING, append_scan_ex, gmapping_enable_particle_maps, gmapping_particle_map,
                                    gmapping_particle_map_append)
    options = {"fast": (), "key64": ((pkg.OPT_K6_BATCH_KEY64, 1),), "sorted": ((pkg.OPT_K6_BATCH_FAST, 0),)}[mode]
    n = 3
    unknown = UNKNOWN[po.CELL_GMAPPING]
    rs = np.random.RandomState(7)
    ang0 = np.deg2rad(np.linspace(-135.0, 135.0, 180))
    rng0, pose0 = rs.uniform(0.5, 2.5, ang0.size), np.array([4.3, -2.1, 0.4])
    ctx = pkg.Context(0)
    pf = None
    try:
        for opt, val in options:
            ctx.set_option(opt, val)
        ctx.map_bind(4, po.CELL_GMAPPING, 150, 70, (20, 50), SCALE, unknown)
        c0, s0, tr0 = one_entry_per_beam(pkg, rng0, ang0)
        nu0 = ctx.map_append_scan(4, pkg.RULE_GMAPPING, pose0, rng0, c0, s0, None, blur=0.2)
        seeds = np.arange(n, dtype=np.uint32)
        pf = pkg.GmappingFilter(ctx, pkg.gmapping_params(), n, seeds)
        with pytest.raises(pkg.SlamHipError, match="does not fit the tile extent"):
            pf.enable_particle_maps(4, extent_tiles=1, pool_tiles=16 + 24 * n, blur=0.2)
        pf.enable_particle_maps(4, extent_tiles=3, pool_tiles=16 + 24 * n, blur=0.2)
        # the oracle: a dense window that holds everything (external x -70 .. 229, y -75 .. 114), one private copy per particle
        W, H, OX, OY = 300, 190, 70, 75
        m, aux = oracle_map(po.CELL_GMAPPING, W, H, (OX, OY), 2)
        assert append_scan_ex(oracle, m, aux, RULE_GMAPPING, pose0, rng0, tr0.angle, None, blur=0.2, trig=tr0) == nu0
        opf = oracle.gmapping_create(n, [0.0] * 8, seeds)
        gmapping_enable_particle_maps(oracle, opf, m, aux, blur=0.2)

        def compare(what):
            for i in range(n):
                got_p, got_a = pf.particle_map(i, -OX, -OY, W, H)
                want_p, want_a = gmapping_particle_map(oracle, opf, i)
                np.testing.assert_array_equal(got_p[..., 0], want_p[..., 0], err_msg="%s, particle %d" % (what, i))
                np.testing.assert_allclose(got_p[..., 1:], want_p[..., 1:], rtol=1e-12, atol=1e-14)
                np.testing.assert_array_equal(got_a, want_a, err_msg="%s, particle %d" % (what, i))

        compare("ancestor")
        ang = np.deg2rad(np.linspace(-135.0, 135.0, 360))
        for step, centre in enumerate([(9.0, -2.0), (4.0, 6.0)]):
            poses = np.array([[centre[0] + 0.31 * i, centre[1] + 0.23 * i, 0.05 * (i - 1)] for i in range(n)])
            rng = rs.uniform(1.0, 4.0, ang.size)
            along_x = np.abs(ang) < 0.3
            rng[along_x] = rs.uniform(9.0, 11.0, np.count_nonzero(along_x))
            occ = (rs.rand(ang.size) < 0.85).astype(np.int32)
            _, _, tr = one_entry_per_beam(pkg, rng, ang)
            nu = pf.particle_maps_append(np.arange(n), poses, rng, ang, occ)
            nu_o = sum(gmapping_particle_map_append(oracle, opf, m, i, poses[i], rng, tr.angle, occ, trig=tr) for i in range(n))
            assert nu == nu_o > n * 360 * 10
            compare("append %d" % step)
        # slamhip_gmapping_particle_map_stats does not report the extent; the tiles a particle's map refers to do (the
        # export's header holds their external positions), and the extent holds them all: the ancestor's two tile columns
        # and the one the long beams added, two rows -- at external x = 192 and beyond lies the column the growth made
        for i in range(n):
            tx, ty = _tile_positions(pf.export_particle_map(i))
            cols, rows = len(np.unique(tx)), len(np.unique(ty))
            assert (cols, rows) == (3, 2), (i, cols, rows)
            assert (np.ptp(tx) // 128 + 1, np.ptp(ty) // 128 + 1) == (3, 2) and tx.max() == 192 and tx.min() == -64
        assert pf.particle_map_stats()["tiles_in_use"] > 2
    finally:  # (a filter that outlives its context at interpreter exit aborts the process)
        if pf is not None:
            pf.close()
        ctx.close()
