"""CPU suite: the C restatement (oracle/slam_oracle.c) against tests/golden/window_oope.npz -- the window observation-probability
estimators (max / mean / overlap) of the compiled reference on oblong, off-centre, empty and rim-crossing analysis areas
(tests/golden/make_golden_window_oope.py) -- bit for bit, and the condition on the golden's inputs that keeps the GPU
suite's default-mode comparisons (device sincos) honest."""
import numpy as np
import pytest
from pyoracle import CELL_OCC, OIE_DISCREPANCY, OIE_OCCUPANCY, make_cfg
from window_oope_cases import (MAPS, MARGIN_CELLS, OOPES, SCAN_MAPS, SCAN_SIZES, TRIGS, area_margin, end_points, golden_map,
                               golden_scan, load_golden, recentred)


@pytest.fixture(scope="module")
def g():
    return load_golden()


def test_the_golden_holds_what_the_issue_lists(g):
    assert g["area_names"].tolist() == ["wide", "tall", "off_centre", "zero_width", "zero_height", "point", "one_cell",
                                        "two_by_one", "half_by_1p5", "tiny", "underflow", "cells_30x21"]
    for name in MAPS:
        m, areas = golden_map(g, name), g[name + "_areas"]
        assert (m.width, m.height, m.origin) == (23, 17, (11, 8))
        assert len(np.unique(m.payload.reshape(23 * 17, -1), axis=0)) == 23 * 17  # every cell a distinct value
        assert np.all(areas[:, 0] <= areas[:, 1]) and np.all(areas[:, 2] <= areas[:, 3])
        side_v, side_h = areas[:, 1] - areas[:, 0], areas[:, 3] - areas[:, 2]
        assert np.sum(side_v * side_h == 0) == 4  # two lines, the point, and the area that underflows ...
        assert side_v[10] > 0 and side_h[10] > 0  # ... although its sides do not
        assert np.sum((side_v == 0) ^ (side_h == 0)) == 2
        assert len(g[name + "_points"]) >= int(g["n_generic"]) + 60
        assert g[name + "_prob_d"].shape == (12, 3, len(g[name + "_points"]))
    assert golden_map(g, "occ07").scale == 0.07 and golden_map(g, "tbm10").cell_model != CELL_OCC
    outside = [2, 9]  # poses with every end point outside the window: the prototype cell alone
    for n in SCAN_SIZES:
        pts = end_points(golden_scan(g, n, 0), g["scan_poses"][outside])
        assert np.all((np.abs(pts[:, 0]) > 10) & (np.abs(pts[:, 1]) > 10))
        f, w = g["scan%d_factor" % n], g["scan%d_weight" % n]
        assert np.any(f != 1.0) and (n == 1 or len(np.unique(w)) > n // 2)


@pytest.mark.parametrize("name", MAPS)
def test_oracle_equals_the_reference_per_point(oracle, g, name):
    m, pts = golden_map(g, name), g[name + "_points"]
    oies = [("d", OIE_DISCREPANCY)] + ([("o", OIE_OCCUPANCY)] if m.cell_model == CELL_OCC else [])
    for oname, oie in oies:
        want = g["%s_prob_%s" % (name, oname)]
        got = np.zeros_like(want)
        for ai, area in enumerate(g[name + "_areas"]):
            for oi, (_n, kind) in enumerate(OOPES):
                cfg = make_cfg(oope=kind, oie=oie)
                got[ai, oi] = [oracle.oope_probability(m, cfg, x, y, recentred(area, x, y)) for x, y in pts]
        np.testing.assert_array_equal(got, want)
        # the values tell vertical from horizontal: wide against tall, the zero-width line against the zero-height one
        gen = want[:, :, :int(g["n_generic"])]
        for a, b in ((0, 1), (3, 4)):
            assert np.all(np.mean(gen[a] != gen[b], axis=1) > 0.5), (a, b)


@pytest.mark.parametrize("n", SCAN_SIZES)
def test_oracle_equals_the_reference_scan_level(oracle, g, n):
    poses = g["scan_poses"]
    for mname in SCAN_MAPS:
        m = golden_map(g, mname)
        for tname, trig in TRIGS:
            scan = golden_scan(g, n, trig)
            want = g["scan%d_%s_%s" % (n, mname, tname)]
            for ai, area in enumerate(g[mname + "_areas"][g["scan_area_idx"]]):
                for oi, (_n, kind) in enumerate(OOPES):
                    got = oracle.score_poses(m, scan, make_cfg(oope=kind, area=area), poses)
                    np.testing.assert_array_equal(got, want[ai, oi], err_msg="%s %s area %d %s" % (mname, tname, ai, _n))


def test_generic_inputs_keep_clear_of_cell_boundaries(g):
    """No GENERIC point, no (pose, beam) end point of the scan-level part and no edge of an analysis area around one lies
    within 1e-9 cells of a cell boundary: there the last ulp of the device's sincos cannot move an end point or an edge
    into another cell, so the default-mode bars of the GPU suite compare like with like.  (The BOUNDARY set is exempt:
    it is scored only where the device's trigonometry is exact -- range 0, heading 0.)"""
    worst = np.inf
    for name in MAPS:
        scale = float(g[name + "_map_scale"])
        pts = g[name + "_points"][:int(g["n_generic"])]
        worst = min([worst] + [area_margin(pts, a, scale) for a in g[name + "_areas"]])
    for n in SCAN_SIZES:
        pts = end_points(golden_scan(g, n, 0), g["scan_poses"])
        assert len(pts) == n * 16
        worst = min([worst] + [area_margin(pts, a, 0.1) for a in g["occ10_areas"][g["scan_area_idx"]]])
    print("smallest distance from a cell boundary: %.3g cells" % worst)
    assert worst > MARGIN_CELLS
