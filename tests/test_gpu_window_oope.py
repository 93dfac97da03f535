"""GPU suite (-m gpu): the window observation-probability estimators (max / mean / overlap; window_probability,
csrc/score_device.h) on analysis areas that are no squares -- oblong, off-centre, lines, the point, sub-cell, one that
underflows, 30 x 21 cells, rectangles across the window's rim -- through the three sites that turn sp_analysis_area into
half extents on their own: k_score_window (score_kernels.hip; the host-driven matchers and the brute-force sweep score
through it), the WIN instantiation of the co-resident hill-climbing chain (hc_resident.hip) and k_pyr_score
(map_pyramid.hip).

References: tests/golden/window_oope.npz (the compiled reference, tests/golden/make_golden_window_oope.py) and the CPU
oracle, which tests/test_window_oope_golden.py holds to that golden bit for bit.  Bars:
  * beam-order sum + host pose trig (the cached provider's arithmetic) or SLAMHIP_POSE_TRIG_RAW_EXACT (the raw one's):
    bit-equal;
  * default mode (canonical tree sum, device sincos): 1e-12 relative, the bar of
    tests/test_gpu_parity.py::test_window_oopes_vs_reference; identical matcher decisions and poses.
The BOUNDARY points (end points and edges ON cell boundaries) are scored as one-beam scans of range 0 at heading 0,
where the device's trigonometry is exact."""
import types

import numpy as np
import pytest
from helpers import assert_trace_equal
from pyramid_cases import golden_map as pyramid_map
from synth import CELL_OCC, CELL_TBM, make_scene
from window_oope_cases import OOPES, SCAN_MAPS, SCAN_SIZES, TRIGS, golden_map, golden_scan, load_golden, recentred

import __graft_entry__ as ge

pytestmark = pytest.mark.gpu

STRICT = dict(sum_order=1, pose_trig=1)  # SLAMHIP_SUM_SEQUENTIAL, SLAMHIP_POSE_TRIG_HOST
DEFAULT_RTOL = 1e-12
OFF_CENTRE, ZERO_HEIGHT = (-0.02, 0.10, -0.07, 0.01), (0.0, 0.0, -0.12, 0.12)


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
    import pyoracle
    return pyoracle


@pytest.fixture(scope="module")
def g():
    return load_golden()


def table_scan(po, rng, cos_a, sin_a, weight, factor):
    """the oracle's view of a scan uploaded as (range, cos a, sin a): a cached trig provider whose table holds exactly
    those values -- the angle-addition arithmetic of SLAMHIP_POSE_TRIG_HOST"""
    n = len(rng)
    return po.ScanData(rng, np.arange(n, dtype=np.float64), weight, factor, po.TRIG_CACHED, 0.0, 1.0, sin_a, cos_a)


def credibilist_impact(p):
    """credibilist_probability (csrc/slamhip_internal.h) over an array of (u, e, o, c) payloads, operation for operation;
    tests/test_credibilist_host.py holds the C function to the reference"""
    t0, t2 = p[..., 0] + p[..., 1], p[..., 2] + p[..., 3]
    tot = ((t0 + 0.0) + t2) + 0.0
    s = np.where(tot == 0.0, 0.0, t2 / np.where(tot == 0.0, 1.0, tot))
    return 1.0 - (1.0 - s)


def as_impact_map(po, m):
    """a CREDIBILIST window as the occupancy map of its cells' probabilities: under the occupancy OIE the oracle's
    estimators then see the values the device derives from the beliefs"""
    unk = credibilist_impact(np.asarray(m.unknown, dtype=np.float64)[None, :4])
    return po.GridMapData(po.CELL_OCC, credibilist_impact(m.payload)[:, :, None], m.origin, m.scale, unk)


def one_beam(pkg, ctx):
    ctx.scan_upload([0.0], [1.0], [0.0], [1.0])


def score_points(pkg, ctx, pts, oope, oie, area):
    poses = np.concatenate([pts, np.zeros((len(pts), 1))], axis=1)
    return ctx.score_poses(0, pkg.spe_cfg(oope=oope, oie=oie, area=area, **STRICT), poses)


# ---- per point ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,plane", [("occ10", 1), ("occ07", 1), ("tbm10", 1), ("tbm10", 0)])
def test_every_point_area_and_estimator_equals_the_reference(pkg, ctx, po, oracle, g, name, plane):
    m, pts, areas = golden_map(g, name), g[name + "_points"], g[name + "_areas"]
    ctx.set_option(pkg.OPT_TBM_PLANE, plane)
    try:
        ctx.upload_map(0, m)
        one_beam(pkg, ctx)
        oies = [("d", pkg.OIE_DISCREPANCY)] + ([("o", pkg.OIE_OCCUPANCY)] if m.cell_model == po.CELL_OCC else [])
        for oname, oie in oies:
            want = g["%s_prob_%s" % (name, oname)]
            got = np.array([[score_points(pkg, ctx, pts, kind, oie, area) for _n, kind in OOPES] for area in areas])
            bad = np.argwhere(got != want)
            print(name, "OIE", oname, "plane", plane, ":", got.size, "values,", len(bad), "differ")
            np.testing.assert_array_equal(got, want, err_msg="first (area, OOPE, point) that differs: %r" % (bad[:1].tolist(),))
        # the BOUNDARY points the reference itself refuses (one of its assertions fires): the oracle's answer
        dropped = g[name + "_dropped"]
        for area in areas if len(dropped) else ():
            for _n, kind in OOPES:
                want = [oracle.oope_probability(m, po.make_cfg(oope=kind), x, y, recentred(area, x, y)) for x, y in dropped]
                np.testing.assert_array_equal(score_points(pkg, ctx, dropped, kind, pkg.OIE_DISCREPANCY, area), want)
    finally:
        ctx.set_option(pkg.OPT_TBM_PLANE, 1)


def test_credibilist_cells_equal_the_oracle_on_the_same_areas_and_points(pkg, ctx, po, oracle, g):
    t = golden_map(g, "tbm10")
    m = types.SimpleNamespace(cell_model=pkg.CELL_CREDIBILIST, payload=t.payload, width=t.width, height=t.height,
                              origin=t.origin, scale=t.scale, unknown=t.unknown)
    occ = as_impact_map(po, m)
    assert len(np.unique(occ.payload)) > 23 * 17 // 2
    ctx.upload_map(0, m)
    one_beam(pkg, ctx)
    pts = g["tbm10_points"]
    for area in g["tbm10_areas"]:
        for _n, kind in OOPES:
            cfg = po.make_cfg(oope=kind, oie=po.OIE_OCCUPANCY)
            want = [oracle.oope_probability(occ, cfg, x, y, recentred(area, x, y)) for x, y in pts]
            np.testing.assert_array_equal(score_points(pkg, ctx, pts, kind, pkg.OIE_DISCREPANCY, area), want, err_msg=_n)


# ---- scan level --------------------------------------------------------------------------------------------------------
def upload_golden_scan(pkg, ctx, scan):
    # the table's entries for the cached provider, libm for the raw one
    cos_a, sin_a = scan.beam_trig() if scan.trig_mode == 1 else pkg.beam_trig(scan.angle)
    ctx.scan_upload(scan.range, cos_a, sin_a, scan.weight, scan.factor)
    ctx.scan_set_angles(scan.angle)


@pytest.mark.parametrize("n", SCAN_SIZES)
@pytest.mark.parametrize("mname", SCAN_MAPS)
def test_scan_scores_equal_the_reference(pkg, ctx, g, mname, n):
    ctx.upload_map(0, golden_map(g, mname))
    poses = g["scan_poses"]
    areas = g[mname + "_areas"][g["scan_area_idx"]]
    for tname, trig in TRIGS:
        upload_golden_scan(pkg, ctx, golden_scan(g, n, trig))
        exact = dict(sum_order=pkg.SUM_SEQUENTIAL, pose_trig=pkg.POSE_TRIG_HOST if tname == "cached" else pkg.POSE_TRIG_RAW_EXACT)
        want = g["scan%d_%s_%s" % (n, mname, tname)]
        for ai, area in enumerate(areas):
            for oi, (oname, kind) in enumerate(OOPES):
                got = ctx.score_poses(0, pkg.spe_cfg(oope=kind, area=area, **exact), poses)
                dflt = ctx.score_poses(0, pkg.spe_cfg(oope=kind, area=area), poses)
                print(mname, n, tname, "area", ai, oname, ": strict max |diff| %g, default max rel %g"
                      % (np.max(np.abs(got - want[ai, oi])), np.max(np.abs(dflt / want[ai, oi] - 1))))
                np.testing.assert_array_equal(got, want[ai, oi], err_msg="%s area %d %s" % (tname, ai, oname))
                np.testing.assert_allclose(dflt, want[ai, oi], rtol=DEFAULT_RTOL, atol=0, err_msg="%s area %d %s" % (tname, ai, oname))


def test_any_split_of_the_pose_batch_gives_the_same_bits(pkg, ctx, g):
    ctx.upload_map(0, golden_map(g, "occ10"))
    upload_golden_scan(pkg, ctx, golden_scan(g, 257, 0))
    rs = np.random.RandomState(3)
    poses = np.concatenate([g["scan_poses"], g["scan_poses"][rs.randint(0, 16, 34)] + rs.randn(34, 3) * [0.05, 0.05, 0.3]])
    assert len(poses) == 50
    for area in g["occ10_areas"][g["scan_area_idx"]]:
        for _n, kind in OOPES:
            for mode in (dict(), STRICT):
                cfg = pkg.spe_cfg(oope=kind, area=area, **mode)
                full = ctx.score_poses(0, cfg, poses)
                assert len(np.unique(full)) > 30
                for chunk in (1, 7, 33):
                    parts = np.concatenate([ctx.score_poses(0, cfg, poses[k:k + chunk]) for k in range(0, len(poses), chunk)])
                    np.testing.assert_array_equal(parts, full, err_msg="chunks of %d" % chunk)


# ---- matchers ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scenes(pkg, po):
    out = {}
    for cell, weighting in ((CELL_OCC, "even"), (CELL_TBM, "viny")):
        sc = make_scene(cell_model=cell, size=200, scale=0.1, n_beams=180, seed=5, weighting=weighting)
        sc["cos_a"], sc["sin_a"] = pkg.beam_trig(sc["scan"].angle)
        sc["oracle_scan"] = table_scan(po, sc["scan"].range, sc["cos_a"], sc["sin_a"], sc["scan"].weight, sc["scan"].factor)
        out[cell] = sc
    return out


def upload_scene(ctx, sc):
    ctx.upload_map(0, sc["map"])
    ctx.scan_upload(sc["scan"].range, sc["cos_a"], sc["sin_a"], sc["scan"].weight, sc["scan"].factor)


@pytest.mark.parametrize("cell", [CELL_OCC, CELL_TBM])
@pytest.mark.parametrize("oname,kind", OOPES)
def test_hill_climbing_over_oblong_and_line_areas_equals_the_oracle(pkg, ctx, po, oracle, scenes, cell, oname, kind):
    sc = scenes[cell]
    upload_scene(ctx, sc)
    prm = [6, 0.1, 0.1]
    for area in (OFF_CENTRE, ZERO_HEIGHT):
        want = oracle.process_scan(oracle.enumerator(po.SM_HC, prm), sc["map"], sc["oracle_scan"],
                                   po.make_cfg(oope=kind, area=area), sc["init_pose"])
        assert want["n_calls"] > 30
        strict = pkg.Matcher(ctx, "HC", pkg.spe_cfg(oope=kind, area=area, **STRICT), prm)
        strict.set_device_chain(0)
        assert_trace_equal(strict.process_scan(0, sc["init_pose"], trace=True), want)  # bit for bit
        for mode in (2, 1, 0):  # the co-resident launch, a kernel per super-step, host-driven batches
            m = pkg.Matcher(ctx, "HC", pkg.spe_cfg(oope=kind, area=area), prm)
            m.set_device_chain(mode)
            assert_trace_equal(m.process_scan(0, sc["init_pose"], trace=True), want, exact_scores=False, rtol=DEFAULT_RTOL)
            if mode == 2:
                assert m.resident_stats() == dict(matches=1, gave_up=0)
            m.close()
        strict.close()


def test_brute_force_and_monte_carlo_over_oblong_and_line_areas_equal_the_oracle(pkg, ctx, po, oracle, scenes):
    for cell, kind_name, okind, prm, oope, area in (
            (CELL_OCC, "BF", po.SM_BF, [-0.2, 0.2, 0.05, -0.1, 0.1, 0.05, -0.04, 0.04, 0.02], pkg.OOPE_OVERLAP, OFF_CENTRE),
            (CELL_TBM, "MC", po.SM_MC, [666666, 0.2, 0.1, 20, 100], pkg.OOPE_MEAN, ZERO_HEIGHT)):
        sc = scenes[cell]
        upload_scene(ctx, sc)
        want = oracle.process_scan(oracle.enumerator(okind, prm), sc["map"], sc["oracle_scan"],
                                   po.make_cfg(oope=oope, area=area), sc["init_pose"])
        assert want["n_calls"] > 20
        m = pkg.Matcher(ctx, kind_name, pkg.spe_cfg(oope=oope, area=area, **STRICT), prm)
        assert_trace_equal(m.process_scan(0, sc["init_pose"], trace=True), want)
        d = pkg.Matcher(ctx, kind_name, pkg.spe_cfg(oope=oope, area=area), prm)
        assert_trace_equal(d.process_scan(0, sc["init_pose"], trace=True), want, exact_scores=False, rtol=DEFAULT_RTOL)
        m.close()
        d.close()


# ---- pyramid -----------------------------------------------------------------------------------------------------------
PYR_RECTS = np.array([(-0.03, 0.03, -0.04, 0.05), OFF_CENTRE, (-0.03, 0.03, -0.17, 0.17), (-0.17, 0.17, -0.03, 0.03), ZERO_HEIGHT,
                      (-0.3, 0.3, 0.0, 0.0), (0.0, 0.0, 0.0, 0.0), (-0.1, 0.5, -0.7, 0.9), (-0.45, 0.05, -0.1, 0.2)])


@pytest.mark.parametrize("i", [64, 66, 67])  # 37 x 29, origin (11, 20), scale 0.1: GridCell, TBM, Credibilist
def test_pyramid_bounds_over_oblong_and_line_rectangles_equal_the_oracle(pkg, ctx, po, oracle, i):
    m = pyramid_map(i)
    ctx.upload_map(0, m)
    rs = np.random.RandomState(i)
    n = 70
    rng, ang = rs.uniform(0.2, 1.5, n), rs.uniform(-np.pi, np.pi, n)
    cos_a, sin_a = pkg.beam_trig(ang)
    weight, factor = rs.rand(n) + 0.1, np.where(rs.rand(n) < 0.2, rs.rand(n), 1.0)
    ctx.scan_upload(rng, cos_a, sin_a, weight, factor)
    scan = table_scan(po, rng, cos_a, sin_a, weight, factor)
    pyr = pkg.Pyramid(ctx, 0, m.oie, 1)
    try:
        stride = pkg.STRIDE[m.cell_model]
        levels = [m] + [types.SimpleNamespace(cell_model=m.cell_model, origin=lv["origin"], scale=lv["scale"], unknown=m.unknown,
                                              payload=ctx.map_download_window(lv["map_id"], 0, 0, lv["width"], lv["height"], stride))
                        for lv in pyr.info()]
        if m.cell_model == pkg.CELL_CREDIBILIST:
            views, ooie = [as_impact_map(po, lv) for lv in levels], po.OIE_OCCUPANCY
        else:
            views = [po.GridMapData(lv.cell_model, lv.payload, lv.origin, lv.scale, lv.unknown) for lv in levels]
            ooie = m.oie
        base = np.array([0.31, -0.27, 0.4])
        rect = PYR_RECTS
        rot = rs.uniform(-0.5, 0.5, len(rect))
        cx, cy = rect[:, 2] + (rect[:, 3] - rect[:, 2]) / 2, rect[:, 0] + (rect[:, 1] - rect[:, 0]) / 2
        poses = np.stack([base[0] + cx, base[1] + cy, rot + base[2]], axis=1)  # LightWeightRectangle::center() added to the pose
        for oname, kind in OOPES:
            got, level = pyr.score_matches(pkg.spe_cfg(oope=kind, oie=m.oie, **STRICT), base, rot, rect)
            assert len(set(level.tolist())) >= 4 and level[0] == 0
            want = np.array([oracle.score_poses(views[level[k]], scan, po.make_cfg(oope=kind, oie=ooie, area=rect[k]), poses[k])[0]
                             for k in range(len(rect))])
            np.testing.assert_array_equal(got, want, err_msg=oname)
            assert len(np.unique(got)) >= len(rect) - 1
    finally:
        pyr.close()
        ctx.map_release(0)


# ---- limits ------------------------------------------------------------------------------------------------------------
def test_the_cap_on_cells_per_beam_and_reversed_areas(pkg, ctx, po, oracle, scenes):
    sc = scenes[CELL_OCC]
    ctx.upload_map(0, sc["map"])
    rs = np.random.RandomState(8)
    rng, ang, weight = rs.uniform(0.5, 3.0, 4), rs.uniform(-2, 2, 4), rs.rand(4) + 0.1
    cos_a, sin_a = pkg.beam_trig(ang)
    ctx.scan_upload(rng, cos_a, sin_a, weight)
    scan = table_scan(po, rng, cos_a, sin_a, weight, np.ones(4))
    poses = np.array([[0.33, -0.41, 0.7], [-2.05, 1.52, -2.4]])
    big = (-4.8, 4.8, -4.8, 4.8)  # 9.6 m at 0.1 m: (96 + 2)^2 = 9 604 cells, under the cap of 10^4
    for _n, kind in OOPES:
        got = ctx.score_poses(0, pkg.spe_cfg(oope=kind, area=big, **STRICT), poses)
        np.testing.assert_array_equal(got, oracle.score_poses(sc["map"], scan, po.make_cfg(oope=kind, area=big), poses))
        with pytest.raises(pkg.SlamHipError, match="more than 10\\^4 cells"):  # 9.9 m: 101^2 = 10 201
            ctx.score_poses(0, pkg.spe_cfg(oope=kind, area=(-4.95, 4.95, -4.95, 4.95)), poses)
        for bad in ((0.1, -0.1, 0.0, 0.2), (0.0, 0.2, 0.1, -0.1)):  # bot > top, left > right
            with pytest.raises(pkg.SlamHipError, match="bot <= top and left <= right"):
                ctx.score_poses(0, pkg.spe_cfg(oope=kind, area=bad), poses)
