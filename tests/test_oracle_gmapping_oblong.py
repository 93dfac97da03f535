"""CPU suite: the C restatement of the GMapping scorer (oracle/slam_oracle.c) on windows that are NO squares, against the
compiled reference (tests/golden/gmapping_oblong.npz, tests/golden/make_golden_gmapping_oblong.py): 77 x 45 cells with
origin (38, 22) and 45 x 77 with origin (22, 38), end cells on, one cell inside, one and two cells outside every rim, in
every corner and far away.

Every other GMapping input of the suite is symmetric in x and y or keeps 60 cells between its end cells and the rims.
  * the oracle equals the reference bit for bit: every score (fullness_th 0.1 and 0.5, one OOPE cache per sequence), the
    HC trace of either map and three filter steps -- the bar of test_oracle_golden.py;
  * the input can tell: with the cells transposed, with the origin's components exchanged, with width and height exchanged
    in the binding alone, EVERY rim group differs from the golden in at least one score.  A group for which this fails
    detects no swap on the device either (tests/test_gpu_gmapping_oblong.py uses the same groups)."""
import numpy as np
import pytest
from gmapping_oblong_cases import (GROUPS, MAPS, MARGIN_CELLS, RIM_GROUPS, SCALE, SCANS, all_poses, end_cells, golden,
                                   golden_map, golden_scan, group_poses, group_scores, group_slices, hc_scan, pf_step,
                                   reaches, run_spans, single_cells, transposed)
from helpers import assert_trace_equal, trace
from pyoracle import OOPE_GMAPPING, SM_HC, Oracle, make_cfg


def score_groups(oracle, m, scan, g, name, key, th=0.1, groups=GROUPS):
    """group -> the oracle's scores of its sequence, one cache per sequence as the generator's one scorer object"""
    cfg = make_cfg(oope=OOPE_GMAPPING, gm_th=th)
    return {grp: oracle.score_poses(m, scan, cfg, group_poses(g, name, key, grp), Oracle.new_gm_cache()) for grp in groups}


def test_the_golden_is_oblong_and_reaches_every_rim():
    """what the generator asserted, from the file: a fixture that lost a case does not pass"""
    g = golden()
    assert len(GROUPS) == 18 and len(RIM_GROUPS) == 16 and g["group_len"].sum() == 92
    spans = {63: False, 255: False}
    for name, (W, H) in MAPS.items():
        m = golden_map(g, name)
        assert (m.width, m.height) == (W, H) and W != H and m.origin[0] != m.origin[1]
        assert all(side % 4 for side in (W, H))
        occ = m.payload[..., 0]
        for ix, iy, full in single_cells(W, H):
            assert (occ[iy, ix] >= 0.1) == full
        full = occ >= 0.1
        for x, y in ((0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)):
            assert full[y, x]
        assert full[:, 0].sum() >= 3 and full[:, W - 1].sum() >= 3 and full[0].sum() >= 3 and full[H - 1].sum() >= 3
        # the full cells are no fixed set of a transposition
        cells = set(zip(*np.nonzero(full)[::-1]))
        assert 2 * len(cells & set((y, x) for x, y in cells)) < len(cells)
        rx, ry = g[name + "_robot_pose"][:2]
        assert min(abs(rx), abs(ry)) >= 1.0 and abs(abs(rx) - abs(ry)) > 0.1
        for key in SCANS:
            scan = golden_scan(g, name, key)
            assert scan.n == int(key[1:].rstrip("c")) and len(np.unique(scan.weight)) == 1
            for grp in GROUPS:
                ec, margin = end_cells(scan, group_poses(g, name, key, grp), m.origin)
                assert margin > MARGIN_CELLS and reaches(grp, W, H, ec), (name, key, grp)
                for first in spans:
                    spans[first] |= run_spans(ec, full, first, W, H)
    assert spans[63] and spans[255]


@pytest.mark.parametrize("key", SCANS)
@pytest.mark.parametrize("name", list(MAPS))
def test_scores_vs_reference(oracle, name, key):
    g = golden()
    m, scan = golden_map(g, name), golden_scan(g, name, key)
    for th in (0.1, 0.5):
        got = score_groups(oracle, m, scan, g, name, key, th)
        for grp in GROUPS:
            np.testing.assert_array_equal(got[grp], group_scores(g, name, key, grp, th), err_msg="%s th %g" % (grp, th))
    # the thresholds are told apart, and the far group sees nothing
    assert scan.n == 1 or not np.array_equal(g["%s_%s_scores" % (name, key)][0], g["%s_%s_scores" % (name, key)][1])
    assert not group_scores(g, name, key, "far").any()


@pytest.mark.parametrize("name", list(MAPS))
def test_hc_trace_across_the_rims_vs_reference(oracle, name):
    g = golden()
    m = golden_map(g, name)
    full = g[name + "_s1080_range"]
    kept = oracle.filter_scan(m, full, g["wide_s1080_angle"], None, g[name + "_hc_init"], skip_rate=3)
    s3 = hc_scan(g, name)
    np.testing.assert_array_equal(full[kept], s3.range)
    e = oracle.enumerator(SM_HC, [6, 0.1, 0.1])
    t = oracle.process_scan(e, m, s3, make_cfg(oope=OOPE_GMAPPING), g[name + "_hc_init"], cache=Oracle.new_gm_cache())
    assert_trace_equal(t, trace(g, name + "_hc6_skip3_"))
    acc = t["poses"][t["accepted"] != 0]
    ec, _ = end_cells(s3, acc, m.origin)
    W, H = MAPS[name]
    inside = (ec[..., 0] >= 0) & (ec[..., 0] < W) & (ec[..., 1] >= 0) & (ec[..., 1] < H)
    on_rim = inside & ((ec[..., 0] == 0) | (ec[..., 0] == W - 1) | (ec[..., 1] == 0) | (ec[..., 1] == H - 1))
    assert np.count_nonzero((~inside).any(axis=1) & on_rim.any(axis=1)) >= 3


def test_filter_steps_vs_reference(oracle):
    """three GmappingParticleFilter steps on the wide map, the robot near (+1.3, -1.2) m"""
    g = golden()
    m = golden_map(g, "wide")
    n = len(g["pf_seeds"])
    pf = oracle.gmapping_create(n, g["pf_gp"], g["pf_seeds"], skip_rate=3)
    for k in range(int(g["pf_n_steps"])):
        st = pf_step(g, k)
        extra = np.arange(5000 + 100 * k, 5000 + 100 * k + n, dtype=np.uint32)
        res, _idx = pf.step(m, st["range"], st["angle"], None, st["delta"], 7 + k, extra)
        poses, w, ms = pf.state()
        assert res == st["resampled"], k
        np.testing.assert_array_equal(ms, st["master"])
        np.testing.assert_array_equal(poses, st["poses"])
        np.testing.assert_array_equal(w, st["weights"])
        assert min(np.abs(poses[:, 0]).min(), np.abs(poses[:, 1]).min()) >= 1.0


@pytest.mark.parametrize("how", ["payload", "origin", "binding"])
@pytest.mark.parametrize("name", list(MAPS))
def test_a_transposition_is_noticed_by_every_rim_group(oracle, name, how):
    """Discriminating power without a GPU, per group and not over the whole file: a group counts as noticing if at least
    one of its scores (any scan) is not the golden's.  (The lone beam of the 1-beam scan aimed two cells outside reaches
    nothing in either window: hence over the scans.)"""
    g = golden()
    mt = transposed(golden_map(g, name), how)
    noticed = {grp: 0 for grp in GROUPS}
    for key in SCANS:
        got = score_groups(oracle, mt, golden_scan(g, name, key), g, name, key)
        for grp in GROUPS:
            noticed[grp] += np.count_nonzero(got[grp] != group_scores(g, name, key, grp))
    for grp in RIM_GROUPS + ("inner",):
        assert noticed[grp] >= 1, "%s does not notice (%s, %s)" % (grp, name, how)
    assert noticed["far"] == 0
    assert all_poses(g, name, "s1080").shape == (92, 3) and len(group_slices(g)) == len(GROUPS) and SCALE == float(g["scale"])
