"""GPU suite: resident maps rendered to occupancy-grid / PGM bytes on the device (csrc/map_render.hip;
slamhip_map_render, slamhip_gmapping_particle_map_render).

The golden bytes of tests/golden/map_render.npz come from the compiled reference (GridMapToPgmDumber::dump_map itself,
the cell loop of OccupancyGridPublisher::on_map_update); tests/test_map_render_host.py holds the host conversion
(render_cells) to them, and the kernels are held to both: to the golden bytes on the golden maps, to render_cells of the
downloaded payload everywhere else.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest
from helpers import load

import __graft_entry__ as ge

pytestmark = pytest.mark.gpu

CLASSES = ("affine", "mean", "tbm_consistent", "tbm_unknown_even", "gmapping", "credibilist")
UNKNOWN = {0: [0.5], 1: [1.0, 0.0, 0.0, 0.0], 2: [-1.0, 0.0, 0.0], 3: [1.0, 0.0, 0.0, 0.0]}


@pytest.fixture(scope="module")
def pkg():
    return ge.load_package()


@pytest.fixture(scope="module")
def golden():
    return load("map_render.npz")


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def upload_golden(pkg, ctx, g, name, map_id):
    model = int(g[name + "_model"])
    payload = g[name + "_payload"]
    h, w = payload.shape[:2]
    ctx.map_bind(map_id, model, w, h, [int(v) for v in g["map_origin"]], float(g["map_scale"]), UNKNOWN[model])
    ctx.map_upload_window(map_id, 0, 0, payload)
    return model, int(g[name + "_occ_kind"]), w, h


@pytest.mark.parametrize("name", CLASSES)
def test_whole_map_render_equals_the_reference_bytes(pkg, ctx, golden, name):
    model, kind, w, h = upload_golden(pkg, ctx, golden, name, 1)
    occ = ctx.map_render(1, pkg.RENDER_OCCGRID, kind)
    assert occ.dtype == np.int8 and occ.shape == (h, w)
    np.testing.assert_array_equal(occ, golden[name + "_occgrid"])
    pgm = ctx.map_render(1, pkg.RENDER_PGM, kind)
    assert pgm.dtype == np.uint8 and pgm.shape == (h, w)
    np.testing.assert_array_equal(pgm, golden[name + "_pgm"])
    # the complete file: the dumper's header in front of the same pixels
    assert ctx.map_render_pgm(1, kind) == b"P5\n%d\n%d\n255\n" % (w, h) + golden[name + "_pgm"].tobytes()
    # the hand-made edge cells as a one-row map (every cell whose reference conversion is defined)
    edge = golden[name + "_edge_payload"]
    n = edge.shape[0]
    ctx.map_bind(2, model, n, 1, [n // 2, 0], 0.1, UNKNOWN[model])
    ctx.map_upload_window(2, 0, 0, edge[None])
    ok = golden[name + "_edge_occgrid_ok"]
    e_occ = ctx.map_render(2, pkg.RENDER_OCCGRID, kind)[0]
    np.testing.assert_array_equal(e_occ[ok], golden[name + "_edge_occgrid"][ok])
    np.testing.assert_array_equal(e_occ, pkg.render_cells(model, edge, pkg.RENDER_OCCGRID, kind))  # the rest: host = device
    np.testing.assert_array_equal(ctx.map_render(2, pkg.RENDER_PGM, kind)[0], golden[name + "_edge_pgm"])
    ctx.map_release(2)
    ctx.map_release(1)


@pytest.mark.parametrize("name", ["mean", "tbm_consistent", "gmapping"])
def test_every_window_edge_equals_the_same_slice_of_the_whole_render(pkg, ctx, golden, name):
    """one-double and four-double cells: windows narrower than a pack, not a multiple of it, starting at odd and even
    columns (aligned and unaligned loads, output rows that start inside a pack), touching the last row and column"""
    _, kind, W, H = upload_golden(pkg, ctx, golden, name, 1)
    whole = {f: ctx.map_render(1, f, kind) for f in (pkg.RENDER_OCCGRID, pkg.RENDER_PGM)}
    n = 0
    for w in (1, 3, 7, 8, 9, 17):
        for h in (1, 2):
            for x0 in sorted({0, 1, 4, 5, 16, W - w - 1, W - w}):
                for y0 in (0, 3, H - h):
                    for f in (pkg.RENDER_OCCGRID, pkg.RENDER_PGM):
                        got = ctx.map_render(1, f, kind, window=(x0, y0, w, h))
                        if f == pkg.RENDER_PGM:  # the whole picture's rows run top-down
                            want = whole[f][::-1][y0:y0 + h, x0:x0 + w][::-1]
                        else:
                            want = whole[f][y0:y0 + h, x0:x0 + w]
                        np.testing.assert_array_equal(got, want, err_msg="window %r format %d" % ((x0, y0, w, h), f))
                        n += 1
    assert n > 400
    # a taller window whose rows start at every offset inside a pack
    for w in (5, 13, W):
        got = ctx.map_render(1, pkg.RENDER_PGM, kind, window=(2 if w < W else 0, 1, w, H - 1))
        np.testing.assert_array_equal(got, whole[pkg.RENDER_PGM][::-1][1:H, (2 if w < W else 0):(2 if w < W else 0) + w][::-1])
    ctx.map_release(1)


def test_a_render_is_ordered_behind_deferred_updates_and_writes_nothing(pkg):
    from synth import CELL_TBM, make_scene
    ctx = pkg.Context(0, testing=True)
    sc = make_scene(cell_model=CELL_TBM, size=200, scale=0.1, n_beams=180, seed=11)
    scan = sc["scan"]
    ctx.upload_map(0, sc["map"])
    c, s = pkg.beam_trig(scan.angle)
    ctx.scan_upload(scan.range, c, s, scan.weight, scan.factor)
    ctx.score_poses(0, pkg.spe_cfg(), sc["init_pose"][None] + np.zeros((4, 3)))  # the probability plane exists from here on

    def plane():
        valid, bad = C.c_int(-1), C.c_longlong(-1)
        assert ctx.L.slamhip_map_debug_prob_plane(ctx.h, 0, C.byref(valid), C.byref(bad)) == 0
        return valid.value, bad.value

    assert plane() == (1, 0)
    before = ctx.map_render(0, pkg.RENDER_OCCGRID, pkg.OCC_TBM_UNKNOWN_EVEN)
    ctx.map_set_auto_grow(0, True)
    ctx.map_set_deferred(True)
    rs = np.random.RandomState(3)
    for k in range(2):
        pose = sc["true_pose"] + rs.randn(3) * [0.3, 0.3, 0.1]
        assert ctx.map_append_scan(0, pkg.RULE_TBM, pose, scan.range, c, s, None, quality=0.9, base=(0.95, 0.04, 0.01, 0.003), blur=0.1) == -1
    got = {(f, k): ctx.map_render(0, f, k) for f in (pkg.RENDER_OCCGRID, pkg.RENDER_PGM) for k in (0, 1)}
    assert ctx.map_drain() > 1000
    info = ctx.map_info(0)
    pay = ctx.map_download_window(0, 0, 0, info["width"], info["height"], 4)
    for (f, k), img in got.items():
        want = pkg.render_cells(pkg.CELL_TBM, pay, f, k)
        np.testing.assert_array_equal(img, want[::-1] if f == pkg.RENDER_PGM else want)
    assert got[(pkg.RENDER_OCCGRID, 1)].shape != before.shape or \
        np.count_nonzero(got[(pkg.RENDER_OCCGRID, 1)] != before) > 200  # the queued updates were seen
    # nothing is written: payload and probability plane are what they were
    for f in (pkg.RENDER_OCCGRID, pkg.RENDER_PGM):
        ctx.map_render(0, f, 0)
        ctx.map_render(0, f, 1, window=(3, 5, 50, 9))
    np.testing.assert_array_equal(ctx.map_download_window(0, 0, 0, info["width"], info["height"], 4), pay)
    assert plane() == (1, 0)
    ctx.map_set_deferred(False)
    ctx.close()


def test_particle_maps_render_through_the_tile_tables(pkg):
    g = load("gmapping_pf_update.npz")
    scale, unknown, n = float(g["scale"]), g["unknown"][:3], 3
    r0, a0, pose0 = g["step0_range"], g["step0_angle"], g["step0_delta"]
    ctx = pkg.Context(0)
    ctx.map_bind(4, pkg.CELL_GMAPPING, 128, 128, [64, 64], scale, unknown)
    c0, s0 = pkg.beam_trig(a0)
    ctx.map_append_scan(4, pkg.RULE_GMAPPING, pose0, r0, c0, s0, max_range=2.5)
    pf = pkg.GmappingFilter(ctx, pkg.gmapping_params(gp8=g["gp"], skip_rate=3, pose_trig=1), n, np.arange(5000, 5000 + n, dtype=np.uint32))
    pf.enable_particle_maps(4, extent_tiles=1, pool_tiles=16 + 40 * n)  # one tile: the appends below grow the extent
    poses = np.array([pose0 + [0.4, 0.2, 0.3], pose0 + [-0.5, 0.3, -0.2]])
    assert pf.particle_maps_append([0, 2], poses, r0, a0) > 1000
    st = pf.particle_map_stats()
    assert st["cow_copies"] > 0  # the two own private tiles where particle 1 still shares the ancestor's

    def check(p, x0, y0, w, h):
        pay, _ = pf.particle_map(p, x0, y0, w, h)
        out = {}
        for f in (pkg.RENDER_OCCGRID, pkg.RENDER_PGM):
            want = pkg.render_cells(pkg.CELL_GMAPPING, pay, f)
            got = pf.particle_map_render(p, f, x0, y0, w, h)
            np.testing.assert_array_equal(got, want[::-1] if f == pkg.RENDER_PGM else want,
                                          err_msg="particle %d window %r format %d" % (p, (x0, y0, w, h), f))
            out[f] = got
        return pay, out

    # tiles are 128 cells and the extent started as one tile around the origin (virtual = external + 64, grown by whole
    # tiles): tile boundaries lie at external 64 + 128 k.  The windows that straddle one are (56, ..) and (-72, ..) in x,
    # (.., 56) and (.., -72) in y and (61, 61) in both; (120, 0, 20, 4) lies inside one tile -- it is the issue's
    # "x from 120 to 140", which straddles a boundary only in virtual coordinates (external 56 to 76, the first window)
    windows = [(56, -10, 20, 6), (-72, 3, 20, 5), (120, 0, 20, 4), (-10, 56, 9, 20), (-5, -72, 3, 17), (61, 61, 7, 7),
               (-300, -300, 600, 600), (-70, -70, 5, 3), (0, 0, 1, 1)]
    imgs = {}
    for p in range(n):
        for win in windows:
            pay, out = check(p, *win)
            if win[2] == 600:
                imgs[p] = (pay, out[pkg.RENDER_OCCGRID])
    # the three maps differ where the two scans went
    assert np.count_nonzero(imgs[0][1] != imgs[1][1]) > 100 and np.count_nonzero(imgs[2][1] != imgs[1][1]) > 100
    assert np.count_nonzero(imgs[0][1] != -1) > 1000 and np.count_nonzero(imgs[0][1] == -1) > 3000
    # far outside the extent, negative coordinates included: the never-observed cell
    for win in ((-5000, -4000, 30, 5), (4000, 5000, 5, 30)):
        for p in (0, 1):
            _, out = check(p, *win)
            assert np.all(out[pkg.RENDER_OCCGRID] == -1) and np.all(out[pkg.RENDER_PGM] == 127)
    pf.close()
    ctx.close()


def test_bad_arguments_are_errors(pkg, ctx, golden):
    _, kind, W, H = upload_golden(pkg, ctx, golden, "affine", 1)
    upload_golden(pkg, ctx, golden, "tbm_consistent", 2)
    upload_golden(pkg, ctx, golden, "gmapping", 3)
    upload_golden(pkg, ctx, golden, "credibilist", 5)
    assert ctx.L.slamhip_map_render(ctx.h, 1, 0, 0, 0, 0, W, H, None) == -1       # null out
    bad = [dict(map_id=1, fmt=2), dict(map_id=1, fmt=-1),                          # unknown format
           dict(map_id=1, fmt=0, occ_kind=1), dict(map_id=3, fmt=0, occ_kind=1), dict(map_id=5, fmt=1, occ_kind=1),  # not TBM
           dict(map_id=2, fmt=0, occ_kind=2), dict(map_id=2, fmt=0, occ_kind=-1),
           dict(map_id=1, fmt=0, window=(0, 0, W + 1, H)), dict(map_id=1, fmt=0, window=(0, 0, W, H + 1)),  # outside the map
           dict(map_id=1, fmt=0, window=(-1, 0, 4, 4)), dict(map_id=1, fmt=0, window=(0, -1, 4, 4)),
           dict(map_id=1, fmt=0, window=(W - 3, 0, 4, 1)), dict(map_id=1, fmt=0, window=(0, H - 1, 1, 2)),
           dict(map_id=1, fmt=0, window=(0, 0, 0, 4)), dict(map_id=1, fmt=0, window=(0, 0, 4, 0)),
           dict(map_id=1, fmt=0, window=(2 ** 31 - 2, 0, 4, 1)),
           dict(map_id=7, fmt=0, window=(0, 0, 1, 1)), dict(map_id=4, fmt=0, window=(0, 0, 1, 1)),  # unbound map
           dict(map_id=-1, fmt=0, window=(0, 0, 1, 1))]
    for kw in bad:
        with pytest.raises(pkg.SlamHipError):
            ctx.map_render(**kw)
    assert ctx.map_render(2, 0, 1).shape == (H, W)  # ... and the TBM map takes either kind
    # the filter's entry: no particle maps, unknown particle, null out, unknown format, empty window
    g = load("gmapping_pf_update.npz")
    pf = pkg.GmappingFilter(ctx, pkg.gmapping_params(gp8=g["gp"], skip_rate=3, pose_trig=1), 2, np.arange(2, dtype=np.uint32))
    with pytest.raises(pkg.SlamHipError):
        pf.particle_map_render(0, pkg.RENDER_PGM, 0, 0, 4, 4)
    pf.enable_particle_maps(3, extent_tiles=1, pool_tiles=96)
    assert pf.particle_map_render(1, pkg.RENDER_PGM, -2, -2, 4, 4).shape == (4, 4)
    for args in ((2, 0, 0, 0, 4, 4), (-1, 0, 0, 0, 4, 4), (0, 2, 0, 0, 4, 4), (0, 0, 0, 0, 0, 4), (0, 0, 0, 0, 4, -1)):
        with pytest.raises(pkg.SlamHipError):
            pf.particle_map_render(*args)
    assert ctx.L.slamhip_gmapping_particle_map_render(pf.h, 0, 0, 0, 0, 4, 4, None) == -1
    pf.close()
    for m in (1, 2, 3, 5):
        ctx.map_release(m)
