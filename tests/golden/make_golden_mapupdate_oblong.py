#!/usr/bin/env python3
"""G6c: golden vectors of the map update on a window that is NO square, touched far from its middle, captured from the
compiled reference.  Writes tests/golden/map_update_oblong.npz.

Every other map-update golden binds a square window with equal origin components and a robot next to the world origin:
an exchange of x and y in the geometry (width / height, origin_x / origin_y, the robot cell's two internal coordinates)
leaves them all unchanged.  Here:
  * the reference map is 203 x 131 cells of 0.1 m -- both odd, neither a multiple of 16 (device pitch != width), the
    origin the reference reports has origin_x != origin_y (asserted);
  * three poses near (+4.3, -2.1) m: the robot cell's internal x and y differ by about a hundred cells, and everything
    touched lies in the quadrant x > 0, y < 0 of the world, off the window's middle in both axes;
  * 360 beams over 270 degrees into a room of 5 x 3 m around the robot: ranges of 1.1 ... 3.4 m, every ray-traced beam
    <= 4 m (the cap MAX_RAY never bites from these poses); 8 % of the beams are max-range readings -- no obstacle at
    their end, as in map_update.npz -- and in the step that has a range gate half of those are 9 m long and gated away;
  * all five cell rules with the const estimator, mean / tbm / gmapping also with the area estimator (Shift_Amount
    pinned as in make_golden_area.py, which this script repeats: run it in a fresh process);
  * payload (+ update counters) after each of the three steps, cropped to an oblong box around the touched cells that
    lies wholly at x > 0, y < 0: bound as a map of its own, its origin is negative in x and beyond the extent in y.
The script asserts that the window never grows, that nothing outside the crop box was touched, and that the touched
cells are no fixed set of a transposition: {(ix, iy)} and {(iy, ix)} share less than half their members.
Run where oracle/_ref/libslamref.so exists:  python tests/golden/make_golden_mapupdate_oblong.py"""
import os
import sys

import numpy as np

GOLDEN_DIR = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(GOLDEN_DIR))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import pyoracle as po  # noqa: E402

WIDTH, HEIGHT, SCALE = 203, 131, 0.1
ROOM = (1.8, 6.8, -3.7, -0.7)  # x_min, x_max, y_min, y_max of the walls, world metres
MAX_RAY = 4.0
MARGIN = 4


def room_ranges(pose, angles):
    """Distance from `pose` to the walls of ROOM along every beam (the robot stands inside)."""
    x, y, th = pose
    c, s = np.cos(th + angles), np.sin(th + angles)
    with np.errstate(divide="ignore"):
        tx = np.where(c > 0, (ROOM[1] - x) / c, np.where(c < 0, (ROOM[0] - x) / c, np.inf))
        ty = np.where(s > 0, (ROOM[3] - y) / s, np.where(s < 0, (ROOM[2] - y) / s, np.inf))
    return np.minimum(tx, ty)


def main():
    if not po.ref_available():
        sys.exit("oracle/_ref/libslamref.so missing")
    R = po.Ref()
    # pin the area estimator's static Shift_Amount to 0.01 * scale (make_golden_area.py, Q27)
    pin = R.map_create(po.REF_CELL_MEAN, po.MAP_UNBOUNDED_PLAIN, 20, 20, SCALE)
    R.append_scan(pin, R.scan_create([0.01], [0.0]), (0.05, 0.05, 0.0), occ_est=1)
    poses = [(4.3, -2.1, np.deg2rad(100)), (4.62, -1.87, np.deg2rad(-35)), (3.97, -2.38, np.deg2rad(215))]
    steps = [dict(quality=1.0, blur=0.0, max_range=np.inf), dict(quality=0.9, blur=0.3, max_range=np.inf),
             dict(quality=0.7, blur=0.1, max_range=8.0)]
    out = dict(scale=np.array(SCALE), n_steps=np.array(len(steps)), shift_amount=np.array(0.01 * SCALE))
    rs = np.random.RandomState(12)
    angles = np.deg2rad(np.linspace(-135.0, 135.0, 360))
    scans = []
    for k, p in enumerate(poses):
        r = room_ranges(p, angles) + rs.randn(angles.size) * 0.005
        o = np.ones(angles.size, np.int32)
        miss = (rs.rand(r.size) < 0.08) | (r > MAX_RAY)  # max-range readings: no obstacle at the end of the beam
        o[miss] = 0
        r = np.minimum(r, MAX_RAY)  # (a sprinkled miss keeps its length: nothing is touched behind the walls)
        if np.isfinite(steps[k]["max_range"]):
            far = miss & (rs.rand(r.size) < 0.5)  # ... beyond the range gate: dropped, the map never sees them
            r = np.where(far, 9.0, r)
            assert far.any() and 9.0 > steps[k]["max_range"]
        assert r.max() <= (MAX_RAY if k < 2 else 9.0) and (r <= MAX_RAY).sum() >= 300 and miss.sum() > 20
        scans.append((r, angles, o))
        out["step%d_pose" % k] = np.array(p)
        out["step%d_range" % k], out["step%d_angle" % k], out["step%d_occ" % k] = r, angles, o
        out["step%d_params" % k] = np.array([steps[k]["quality"], steps[k]["blur"], steps[k]["max_range"]])
    base_plain, base_tbm = (0.95, 1.0, 0.01, 1.0), (0.95, 0.04, 0.01, 0.003)
    models = {"mean": (po.REF_CELL_MEAN, base_plain), "affine": (po.REF_CELL_AFFINE, base_plain),
              "tbm": (po.REF_CELL_TBM, base_tbm), "gmapping": (po.REF_CELL_GMAPPING, base_plain),
              "last": (po.REF_CELL_MOCK, base_plain)}
    runs = [(name, 0) for name in models] + [(name, 1) for name in ("mean", "tbm", "gmapping")]
    results, touched_all = {}, None
    for name, est in runs:
        cell, base = models[name]
        mtype = po.MAP_UNBOUNDED_LAZY_TILED if cell == po.REF_CELL_GMAPPING else po.MAP_UNBOUNDED_PLAIN
        m = R.map_create(cell, mtype, WIDTH, HEIGHT, SCALE, 0.5)
        g0 = m.geometry()
        assert (g0["width"], g0["height"]) == (WIDTH, HEIGHT), g0
        assert g0["origin"][0] != g0["origin"][1], "the origin must tell x from y"
        unknown = m.to_data().unknown
        if est == 0:
            out[name + "_base"] = np.array(base)
            out[name + "_origin"] = np.array(g0["origin"])
            out[name + "_size"] = np.array([g0["width"], g0["height"]])
            out[name + "_unknown"] = unknown
        else:
            assert tuple(out[name + "_origin"]) == tuple(g0["origin"])
        for k, p in enumerate(poses):
            r, a, o = scans[k]
            R.append_scan(m, R.scan_create(r, a, o), p, quality=steps[k]["quality"], occ_est=est, base=base,
                          blur=steps[k]["blur"], max_range=steps[k]["max_range"])
            assert m.geometry() == g0, "the window must not grow in this fixture"
            md = m.to_data()
            results[(name, est, k)] = (md.payload.copy(), m.aux())
            st = md.payload.shape[2]
            touched = (md.payload != unknown[:st]).any(axis=2)
            touched_all = touched if touched_all is None else (touched_all | touched)
        # discriminating power: the touched cells against their own transposition
        ys, xs = np.nonzero(touched)
        cells = set(zip(xs.tolist(), ys.tolist()))
        shared = len(cells & set(zip(ys.tolist(), xs.tolist())))
        assert len(cells) > 1500 and 2 * shared < len(cells), (name, est, len(cells), shared)
        out["%s_est%d_touched_shared" % (name, est)] = np.array([len(cells), shared])
    # the crop: an oblong box around everything any run touched, wholly at x > 0 and y < 0 of the world
    ys, xs = np.nonzero(touched_all)
    x0, x1, y0, y1 = xs.min() - MARGIN, xs.max() + 1 + MARGIN, ys.min() - MARGIN, ys.max() + 1 + MARGIN
    ox, oy = [int(v) for v in out["mean_origin"]]
    assert 0 <= x0 and x1 <= WIDTH and 0 <= y0 and y1 <= HEIGHT, (x0, y0, x1, y1, ox, oy)
    assert x1 - x0 != y1 - y0 and (x1 - x0) % 16 != 0
    assert ox - x0 < 0 and oy - y0 >= y1 - y0, "re-based, the crop box must not hold the world origin"
    out["crop"] = np.array([x0, y0, x1, y1])
    for (name, est, k), (payload, aux) in results.items():
        tag = "%s%s_step%d_" % (name, "_area" if est else "", k)
        out[tag + "payload"] = payload[y0:y1, x0:x1].copy()
        outside = np.ones(payload.shape[:2], bool)
        outside[y0:y1, x0:x1] = False
        st = payload.shape[2]
        assert (payload[outside] == out[name + "_unknown"][:st]).all(), "touched cells outside the crop"
        if aux is not None:
            out[tag + "aux"] = aux[y0:y1, x0:x1].copy()
            assert not aux[outside].any(), "update counters outside the crop"
    path = os.path.join(GOLDEN_DIR, "map_update_oblong.npz")
    np.savez_compressed(path, **out)
    print("wrote map_update_oblong.npz", os.path.getsize(path) // 1024, "KiB, crop", out["crop"], "origin", (ox, oy))


if __name__ == "__main__":
    main()
