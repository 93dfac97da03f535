"""CPU suite: the oracle (oracle/slam_oracle.c, map_update_oracle.c) against the compiled reference FAR FROM THE WORLD
ORIGIN -- tests/golden/placed.npz, recorded by make_golden_placed.py at the four Q stations of tests/placed_scenes.py (one
per quadrant, 1000 ... 2000 m out, window origins outside the windows).  The same equality as the near-origin
oracle-vs-golden tests: bit for bit.  Plus what the GPU suite (tests/test_gpu_placed.py) leans on: the placed helper is
make_scene at station O, and the oracle alone leaves at most 2 % of any case's poses ill-conditioned."""
import numpy as np
import placed_cases as pc
import placed_scenes as ps
import pytest
import synth
from helpers import assert_trace_equal
from pyoracle import (OOPE_GMAPPING, OOPE_OBSTACLE, SM_BF, SM_HC, SM_MC, SUM_TREE256, TRIG_CACHED, TRIG_RAW, Oracle,
                      make_cfg)

TRIGS = (("cached", TRIG_CACHED), ("raw", TRIG_RAW))


@pytest.fixture(scope="module")
def g():
    return pc.golden()


@pytest.mark.parametrize("cell_model", [synth.CELL_OCC, synth.CELL_TBM, synth.CELL_GMAPPING])
def test_station_o_is_make_scene_bit_for_bit(cell_model):
    for weighting in ("even", "viny"):
        a = synth.make_scene(cell_model=cell_model, size=240, scale=0.1, n_beams=360, seed=ps.SEEDS["O"], weighting=weighting)
        b = ps.place("O", cell_model, size=240, scale=0.1, n_beams=360, weighting=weighting, raw=True)
        assert a["map"].origin == b["map"].origin and (a["map"].width, a["map"].height) == (b["map"].width, b["map"].height)
        np.testing.assert_array_equal(a["map"].payload, b["map"].payload)
        np.testing.assert_array_equal(a["map"].unknown, b["map"].unknown)
        for k in ("range", "angle", "weight", "factor"):
            np.testing.assert_array_equal(getattr(a["scan"], k), getattr(b["scan"], k))
        for k in ("init_pose", "true_pose", "gt"):
            np.testing.assert_array_equal(a[k], b[k])
        assert b["true_pose"][2] == np.pi / 2 and not b["shift"].any()
        r, an, occ = b["raw"]
        np.testing.assert_array_equal(r[occ == 1], b["scan"].range)
        np.testing.assert_array_equal(an[occ == 1], b["scan"].angle)


@pytest.mark.parametrize("station", ps.Q_STATIONS + ps.F_STATIONS)
def test_a_moved_scene_is_the_local_scene_with_another_origin(station):
    """Only the origin, the poses and GMapping's obstacle means move; the window's origin lies outside the window."""
    (kx, ky), h = ps.STATIONS[station]
    for cell_model, scale, size in ((synth.CELL_OCC, 0.1, 240), (synth.CELL_GMAPPING, 0.05, 400)):
        far = ps.place(station, cell_model, size=size, scale=scale, n_beams=360)
        m = far["map"]
        assert m.origin == (size // 2 - kx, size // 2 - ky)
        assert not 0 <= m.origin[0] < m.width and not 0 <= m.origin[1] < m.height
        s = np.array([kx * scale, ky * scale, 0.0])
        np.testing.assert_array_equal(far["true_pose"], np.array([scale / 2, scale / 2, h]) + s)
        np.testing.assert_array_equal(far["init_pose"], np.array([scale / 2, scale / 2, h]) + ps.INIT_OFFSET + s)
        assert np.floor(far["true_pose"][0] / scale) == kx and np.floor(far["true_pose"][1] / scale) == ky
        local = synth.build_map(cell_model, size, scale, far["local"], far["scan"].range, far["scan"].angle,
                                blur_m=0.0 if cell_model == synth.CELL_GMAPPING else 0.3)
        np.testing.assert_array_equal(m.payload[..., 0], local.payload[..., 0])
        if cell_model == synth.CELL_GMAPPING:
            known = local.payload[..., 0] != -1.0
            assert known.sum() > 1000
            np.testing.assert_array_equal(m.payload[..., 1][known], local.payload[..., 1][known] + s[0])
            np.testing.assert_array_equal(m.payload[..., 2][known], local.payload[..., 2][known] + s[1])
            np.testing.assert_array_equal(m.payload[~known], local.payload[~known])
            occupied = local.payload[..., 1] != 0.0  # the means of the cells that hold an obstacle lie in their cells, out there
            cx = np.floor(m.payload[..., 1][occupied] / scale).astype(np.int64) + m.origin[0]
            assert occupied.sum() > 100 and cx.min() >= 0 and cx.max() < m.width


def test_the_golden_holds_what_the_tests_rely_on(g):
    signs = {"Q1": (1, 1), "Q2": (-1, 1), "Q3": (-1, -1), "Q4": (1, -1)}
    w, h = [int(v) for v in g["window"]]
    assert w <= 128 and h <= 96 and w != h and w % 16
    for st in ps.Q_STATIONS:
        ox, oy = g[st + "_origin"]
        assert not 0 <= ox < w and not 0 <= oy < h
        assert tuple(np.sign(g[st + "_true_pose"][:2])) == signs[st] and np.abs(g[st + "_true_pose"][:2]).min() > 1000.0
        assert g[st + "_true_pose"][2] == ps.STATIONS[st][1]
        sc = ps.place(st, size=int(g["raster"]), scale=float(g["scale"]), n_beams=int(g["n_beams"]), raw=True)
        np.testing.assert_array_equal(sc["raw"][0], g[st + "_raw_range"])  # the helper still makes the recorded scene
        np.testing.assert_array_equal(sc["init_pose"], g[st + "_init_pose"])
        np.testing.assert_array_equal(ps.candidates(sc, 64, 100 + ps.SEEDS[st]), g[st + "_poses"])
        for name in ("hc6", "hc128", "mc", "bf"):
            assert g["%s_mean_cached_%s_accepted" % (st, name)][1:].any(), (st, name)
        for name in ("hc128", "hc128tiny"):
            assert pc.oracle_tail(pc.trace(g, "%s_mean_cached_%s_" % (st, name))) >= 6 * 64
        for name, est in pc.UPDATE_RUNS:
            assert pc.has_snapshot(g, st, name, est, 2) and (pc.has_snapshot(g, st, name, est, 0) or (name, est) == ("tbm", 1))


@pytest.mark.parametrize("station", ps.Q_STATIONS)
def test_filter_and_scores_vs_reference(oracle, g, station):
    st = station
    for tname, trig in TRIGS:
        for name, weighting in (("mean", "even"), ("tbm", "viny")):
            m = pc.final_map(g, st, name)
            kept = oracle.filter_scan(m, g[st + "_raw_range"], g[st + "_raw_angle"], g[st + "_raw_occ"], g[st + "_init_pose"],
                                      trig=pc.raw_trig(g, st, trig))
            np.testing.assert_array_equal(kept, g[st + "_kept"])
            scan = pc.golden_scan(g, st, trig, weighting)
            if weighting == "viny":
                np.testing.assert_array_equal(oracle.weights("viny", scan.range, scan.angle), g[st + "_viny_weight"])
            key = "%s_%s_%s_" % (st, name, tname)
            s = oracle.score_poses(m, scan, make_cfg(), g[st + "_poses"])
            np.testing.assert_array_equal(s, g[key + "scores"])
            assert s[0] == s[1] and len(np.unique(s)) > 40
            tree = oracle.score_poses(m, scan, make_cfg(sum_order=SUM_TREE256), g[st + "_poses"])
            np.testing.assert_allclose(tree, g[key + "scores"], rtol=1e-13, atol=0)
            for kname, kind in pc.WIN_OOPES:
                sw = oracle.score_poses(m, scan, make_cfg(oope=kind, area=g["win_area"]), g[st + "_poses"][:24])
                np.testing.assert_array_equal(sw, g[key + "win_" + kname], err_msg=key + kname)
        m, scan = pc.final_map(g, st, "gmapping"), pc.golden_scan(g, st, trig)
        s = oracle.score_poses(m, scan, make_cfg(oope=OOPE_GMAPPING), g[st + "_gm_poses"], Oracle.new_gm_cache())
        np.testing.assert_array_equal(s, g["%s_gmapping_%s_scores" % (st, tname)])
        assert len(np.unique(s)) > 40


def test_single_oope_probabilities_of_end_points_far_out(oracle, g):
    """oracle.oope_probability at the end points of the first beams under the station pose: the value the scan-level
    golden is the weighted mean of.  One beam, weight 1: estimate_scan_probability IS that beam's probability."""
    for st in ps.Q_STATIONS:
        m = pc.final_map(g, st, "mean")
        scan = pc.golden_scan(g, st, TRIG_RAW)
        pose = g[st + "_poses"][0]
        for b in (0, 7, 100):
            x = pose[0] + scan.range[b] * np.cos(pose[2] + scan.angle[b])
            y = pose[1] + scan.range[b] * np.sin(pose[2] + scan.angle[b])
            from pyoracle import ScanData
            one = ScanData(scan.range[b:b + 1], scan.angle[b:b + 1], np.ones(1))
            for kname, kind in pc.WIN_OOPES:
                a = g["win_area"]
                hv, hh = (a[1] - a[0]) / 2, (a[3] - a[2]) / 2
                p = oracle.oope_probability(m, make_cfg(oope=kind), x, y, [y - hv, y + hv, x - hh, x + hh])
                s = oracle.score_poses(m, one, make_cfg(oope=kind, area=a), pose)[0]
                assert 0.0 <= p <= 1.0 and abs(s - p) <= 1e-12, (st, b, kname, s, p)


@pytest.mark.parametrize("station", ps.Q_STATIONS)
def test_matcher_traces_vs_reference(oracle, g, station):
    st = station
    m, scan = pc.final_map(g, st, "mean"), pc.golden_scan(g, st, TRIG_CACHED)
    for name, kind, prm in (("hc6", SM_HC, g["hc6_params"]), ("hc128", SM_HC, g["hc128_params"]),
                            ("hc128tiny", SM_HC, g["hc128tiny_params"]), ("mc", SM_MC, g["mc_params"]), ("bf", SM_BF, g["bf_params"])):
        t = oracle.process_scan(oracle.enumerator(kind, prm), m, scan, make_cfg(), g[st + "_init_pose"])
        assert_trace_equal(t, pc.trace(g, "%s_mean_cached_%s_" % (st, name)))
    m, scan = pc.final_map(g, st, "tbm"), pc.golden_scan(g, st, TRIG_RAW, "viny")
    t = oracle.process_scan(oracle.enumerator(SM_HC, g["hc6_params"]), m, scan, make_cfg(), g[st + "_init_pose"])
    assert_trace_equal(t, pc.trace(g, st + "_tbm_raw_hc6_"))
    m, scan = pc.final_map(g, st, "gmapping"), pc.golden_scan(g, st, TRIG_RAW)
    t = oracle.process_scan(oracle.enumerator(SM_HC, g["hc6_params"]), m, scan, make_cfg(oope=OOPE_GMAPPING), g[st + "_init_pose"],
                            cache=Oracle.new_gm_cache())
    assert_trace_equal(t, pc.trace(g, st + "_gmapping_raw_hc6_"))


@pytest.mark.parametrize("name,est", pc.UPDATE_RUNS, ids=pc.UPDATE_IDS)
@pytest.mark.parametrize("station", ps.Q_STATIONS)
def test_append_scan_vs_reference(oracle, g, station, name, est):
    m, aux, rule = pc.fresh_map(g, station, name)
    checked = 0
    for k in range(3):
        assert pc.oracle_append(oracle, g, station, name, est, k, m, aux, rule) > 1000
        if not pc.has_snapshot(g, station, name, est, k):
            continue
        t = pc.tag(station, name, est, k)
        np.testing.assert_array_equal(m.payload, g[t + "payload"], err_msg=t)
        if aux is not None:
            np.testing.assert_array_equal(aux, g[t + "aux"], err_msg=t)
        checked += 1
    assert checked == (1 if (name, est) == ("tbm", 1) else 3)
    if name == "gmapping":  # the obstacle means are world metres out there, in the station's quadrant
        occupied = aux[..., 0] > 0
        sx, sy = np.sign(g[station + "_true_pose"][:2])
        assert occupied.sum() > 100 and (np.sign(m.payload[..., 1][occupied]) == sx).all() and (np.sign(m.payload[..., 2][occupied]) == sy).all()
        assert np.abs(m.payload[..., 1:][occupied]).min() > 990.0


def test_the_oracle_alone_leaves_few_poses_ill_conditioned(oracle):
    """The GPU suite leaves a pose out of a non-exact comparison of a piecewise-constant scorer when the ORACLE's score of
    it changes under a one-ulp move of x or y.  That exclusion must not be where a failure hides: over every case of the
    GPU suite at most 2 % of the poses, by the oracle alone.  The allowances of the continuous scorers are printed for
    LOG.md (pytest -s)."""
    lines = []
    for cid, st, m, scan, oope, area, poses in pc.scorer_cases():
        rows = pc.probe(oracle, m, scan, make_cfg(oope=oope, area=area), poses)
        assert np.all(np.isfinite(rows)) and np.all(rows[0] > 0), cid
        if oope in pc.PIECEWISE_CONSTANT:
            bad = pc.ill_conditioned(rows)
            assert bad.mean() <= pc.MAX_LEFT_OUT, "%s: %d of %d poses" % (cid, bad.sum(), bad.size)
            if st == "O":
                assert not bad.any(), cid  # (an ulp of a few metres moves nothing near the origin)
            lines.append("%-40s left out %d of %d" % (cid, bad.sum(), bad.size))
        else:
            rtol, rel = pc.allowance(rows, oope)
            assert rel < 1e-6, cid  # (a probe that moved a score this much would mean a broken scene, not rounding)
            lines.append("%-40s probe %.3g -> rtol %.3g" % (cid, rel, rtol))
    print("\n" + "\n".join(lines))
