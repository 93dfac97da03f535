"""CPU suite: the map-update restatement (oracle/map_update_oracle.c) on a window that is NO square and is touched far
from its middle, against the compiled reference (tests/golden/map_update_oblong.npz,
tests/golden/make_golden_mapupdate_oblong.py): 203 x 131 cells, origin (101, 65), robot near (+4.3, -2.1) m.

Every other map-update golden is symmetric in x and y (square window, equal origin components, robot at the world
origin), so an exchange of width and height or of the origin's components passes them all.  Here
  * the oracle equals the reference bit for bit, all five rules, both estimators, payload and counters after every step
    (the bar of test_oracle_mapupdate.py);
  * the same on the crop box bound as a map of its own: its origin is (-13, 42) in a window 60 x 40 -- negative in x,
    beyond the extent in y, the world origin outside the window -- and the results are the same bytes;
  * the input can tell: with the geometry transposed (or the origin's components alone exchanged) the result differs
    from the golden in more than 1 000 cells for every rule.  An input for which this fails detects no swap."""
import numpy as np
import pytest
from mapupdate_oblong_cases import (MODELS, RUN_IDS, RUNS, crop_of, fresh_map, geometry, golden, oracle_step,
                                    outside_crop, tag)


def test_the_golden_is_oblong_and_off_centre():
    g = golden()
    x0, y0, x1, y1 = [int(v) for v in g["crop"]]
    for name in MODELS:
        w, h, (ox, oy) = geometry(g, name)
        assert (w, h) == (203, 131) and ox != oy and w % 16 and h % 16
        cw, ch, (cox, coy) = geometry(g, name, "crop")
        assert cw != ch and cw % 16 and cox != coy
        assert cox < 0 and coy >= ch  # the world origin lies outside the re-based window, one sign per axis
    for name, est in RUNS:
        n_touched, n_shared = g["%s_est%d_touched_shared" % (name, est)]
        assert n_touched > 1500 and 2 * n_shared < n_touched  # (recorded by the generator)
    for k in range(int(g["n_steps"])):
        rx, ry = np.floor(g["step%d_pose" % k][:2] / float(g["scale"])) + g["mean_origin"]
        assert abs(rx - ry) > 50 and x0 <= rx < x1 and y0 <= ry < y1  # the robot cell's internal x and y differ


@pytest.mark.parametrize("name,est", RUNS, ids=RUN_IDS)
def test_append_scan_oblong_vs_reference(oracle, name, est):
    g = golden()
    m, aux, rule = fresh_map(g, name)
    for k in range(int(g["n_steps"])):
        assert oracle_step(oracle, g, name, est, k, m, aux, rule) > 1000
        np.testing.assert_array_equal(crop_of(g, m.payload), g[tag(name, est, k) + "payload"], err_msg="step %d" % k)
        if aux is not None:
            np.testing.assert_array_equal(crop_of(g, aux), g[tag(name, est, k) + "aux"], err_msg="step %d" % k)
    assert (outside_crop(g, m.payload) == m.unknown[:m.payload.shape[2]]).all()  # as the generator asserted
    if aux is not None:
        assert not outside_crop(g, aux).any()


@pytest.mark.parametrize("name,est", RUNS, ids=RUN_IDS)
def test_append_scan_on_a_window_without_the_world_origin_vs_reference(oracle, name, est):
    """The crop box as its own map, origin - (x0, y0): nothing may depend on where in a window a cell lies."""
    g = golden()
    m, aux, rule = fresh_map(g, name, "crop")
    full, full_aux, _ = fresh_map(g, name)
    for k in range(int(g["n_steps"])):
        n_upd = oracle_step(oracle, g, name, est, k, m, aux, rule)
        assert n_upd == oracle_step(oracle, g, name, est, k, full, full_aux, rule)
        np.testing.assert_array_equal(m.payload, g[tag(name, est, k) + "payload"], err_msg="step %d" % k)
        assert m.payload.tobytes() == g[tag(name, est, k) + "payload"].tobytes()
        if aux is not None:
            np.testing.assert_array_equal(aux, g[tag(name, est, k) + "aux"], err_msg="step %d" % k)
            assert aux.tobytes() == g[tag(name, est, k) + "aux"].tobytes()


def _in_internal_cells(a, unknown, side):
    """`a` laid into a side x side array of internal cells; what lies outside its window holds the prototype."""
    out = np.tile(np.asarray(unknown, dtype=np.float64), (side, side, 1))
    out[:a.shape[0], :a.shape[1]] = a
    return out


@pytest.mark.parametrize("swap", ["transposed", "origin_swapped"])
@pytest.mark.parametrize("name,est", RUNS, ids=RUN_IDS)
def test_a_transposed_geometry_is_noticed(oracle, name, est, swap):
    """Discriminating power without a GPU.  width <-> height and origin_x <-> origin_y, same scans: cell by internal
    coordinate (a cell outside either window counts as never touched) the result differs from the golden in more than
    1 000 cells.  In the transposed window some beams leave it and the oracle stops there (ValueError) -- whatever it
    wrote until then is compared; with the origin's components alone exchanged every beam stays inside."""
    g = golden()
    k_last = int(g["n_steps"]) - 1
    want, _, _ = fresh_map(g, name)
    crop_of(g, want.payload)[:] = g[tag(name, est, k_last) + "payload"]
    m, aux, rule = fresh_map(g, name, swap)
    left = False
    for k in range(k_last + 1):
        try:
            oracle_step(oracle, g, name, est, k, m, aux, rule)
        except ValueError:
            left = True
    assert left == (swap == "transposed")
    st = m.payload.shape[2]
    a = _in_internal_cells(want.payload, m.unknown[:st], 203)
    b = _in_internal_cells(m.payload, m.unknown[:st], 203)
    assert np.count_nonzero((a != b).any(axis=2)) > 1000
