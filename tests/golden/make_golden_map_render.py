#!/usr/bin/env python3
"""Generate tests/golden/map_render.npz from the COMPILED REFERENCE: maps of every cell class the device path holds, read
the way the reference's two map consumers read them.

Runs only where the reference tree is present.  tests/golden/map_render_harness.cpp (ours; it includes the unmodified
reference headers) is compiled with the reference's own flags, as oracle/Makefile does, into oracle/_ref/ (git-ignored);
the binary is never committed.  The fixture is data only: the inputs made here and what the reference computed.

    python tests/golden/make_golden_map_render.py [path/to/reference]

The PGM bytes are written by GridMapToPgmDumber::dump_map itself (src/utils/map_dumpers.h:65-89).  The int8 row of
OccupancyGridPublisher::on_map_update (src/ros/occupancy_grid_publisher.h:37-46) is computed IN THE HARNESS by the
publisher's three lines restated (`double value = (double)map[pnt]; int cell_value = value == -1 ? -1 : value * 100;`
pushed into an int8 vector), because that header includes ROS and cannot be compiled here.

Contents of map_render.npz, per cell class <c> in CLASSES (names below)
  maps    <c>_payload [29, 37, stride]  the cells in the device library's host stride after seeded random
          GridMap::update calls (about a third of the cells never observed), <c>_value [29, 37] = (double)map[c],
          <c>_occgrid [29, 37] int8 (rows bottom-up), <c>_pgm [29, 37] uint8 (rows top-down, as in the file);
          map_origin, map_scale, obs (the observations: x, y, is_occ, prob, est_quality, quality, obst_x, obst_y)
  edges   <c>_edge_payload [n, stride], <c>_edge_value [n], <c>_edge_occgrid [n] int8, <c>_edge_occgrid_ok [n] bool (False
          where the reference's own value is NaN / infinite or its hundredfold leaves int: its conversion is undefined
          there and the cell has no OCCGRID golden), <c>_edge_pgm [n] uint8: hand-made cells -- occupancy exactly 0 and
          1, k / 100 for k = 0..100, values at and one ulp either side of the 1/255 steps, values outside [0, 1], -1,
          denormals; for the belief classes the same occupancies as (u, e, o, c) = (0, 1 - v, v, 0), pure masses,
          masses near 1e-300, the vacuous belief (kept as the fresh cell: TbmBaseCell reports its prototype's occupancy
          until its first update)
  <c>_model, <c>_occ_kind  the SLAMHIP_CELL_* model and SLAMHIP_OCC_TBM_* kind the class maps to
"""
import os
import subprocess
import sys

import numpy as np

GOLDEN_DIR = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(GOLDEN_DIR))
REFERENCE = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("REFERENCE", "/root/reference")
OUT_DIR = os.path.join(ROOT, "oracle", "_ref")

# name, harness class id, SLAMHIP_CELL_* model, occ_kind, host stride
CLASSES = [("affine", 0, 0, 0, 1), ("mean", 1, 0, 0, 1), ("tbm_consistent", 2, 1, 0, 4), ("tbm_unknown_even", 3, 1, 1, 4),
           ("gmapping", 4, 2, 0, 3), ("credibilist", 5, 3, 0, 4)]
MAP_W, MAP_H, SCALE = 37, 29, 0.1
ORIGIN = (11, 20)  # off centre


def build():
    os.makedirs(OUT_DIR, exist_ok=True)
    exe = os.path.join(OUT_DIR, "map_render_harness")
    subprocess.check_call(["g++", "-std=c++14", "-O3", "-w", "-I" + os.path.join(REFERENCE, "src"), "-o", exe,
                           os.path.join(GOLDEN_DIR, "map_render_harness.cpp")])
    return exe


def observations(rs):
    """seeded random observations over about two thirds of the cells, one to four each"""
    obs = []
    for y in range(MAP_H):
        for x in range(MAP_W):
            if rs.rand() < 1.0 / 3.0:
                continue
            ex, ey = x - ORIGIN[0], y - ORIGIN[1]
            for _ in range(rs.randint(1, 5)):
                prob = rs.choice([0.95, 0.01, 0.5, 0.0, 1.0, rs.rand()], p=[0.25, 0.3, 0.05, 0.05, 0.05, 0.3])
                est_q = rs.choice([1.0, 0.7, 0.3, 0.05])
                qual = rs.choice([0.9, 0.6, 0.3])  # est_q * qual < 1: no observation is a certainty
                obs.append([ex, ey, float(prob > 0.5), prob, est_q, qual, (ex + rs.rand()) * SCALE, (ey + rs.rand()) * SCALE])
    order = rs.permutation(len(obs))  # cells are visited in no particular order
    return np.asarray(obs, dtype=np.float64)[order]


def edge_values():
    v = [0.0, 1.0, -1.0, 0.5, -0.0, 1.5, -0.25, 2.0, 1e-300, 5e-324, 1.0 - 2.0 ** -53, 2.0 ** -52]
    v += [k / 100 for k in range(101)]
    for j in range(256):
        s = 1.0 - j / 255.0
        v += [s, np.nextafter(s, 0.0), np.nextafter(s, 1.0)]
    return v


def edges_for(stride):
    vals = edge_values()
    if stride != 4:
        # a one-value cell can hold anything: the values the publisher's conversion is undefined for come last
        vals = vals + [21474836.0, -21474836.0, 1e300, -1e300, np.inf, -np.inf, np.nan]
        e = np.zeros((len(vals), 4))
        e[:, 0] = vals
        return e
    t = 1e-300
    b = [[0.0, 1.0 - v, v, 0.0] for v in vals if 0.0 <= v <= 1.0]
    b += [[1, 0, 0, 0], [0, 0, 1, 0], [0, 1, 0, 0], [0, 0, 0, 1], [0, 0, 0, 0],
          [t, 0, 0, 0], [0, t, 0, 0], [0, 0, t, 0], [0, 0, 0, t], [t, t, t, t], [t, 0, t, 0], [0, t, t, 0], [3 * t, t, 2 * t, 0],
          [1, 0, t, 0], [t, 0, 1, 0], [1, t, 0, 0], [0.5, 0, 0.5, 0], [0.5, 0.5, 0, 0], [0.25, 0.25, 0.25, 0.25],
          [5e-324, 0, 5e-324, 0], [5e-324, 5e-324, 5e-324, 0], [0.1, 0.2, 0.3, 0.4], [0.3, 0.0, 0.7, 0.0], [0.98, 0.01, 0.01, 0.0]]
    b += [[1.0 - k / 100, 0.0, k / 100, 0.0] for k in range(0, 101, 7)]  # o + 0.5 u off the k / 100 grid
    return np.asarray(b, dtype=np.float64)


def main():
    if not os.path.isfile(os.path.join(REFERENCE, "src", "utils", "map_dumpers.h")):
        sys.exit("reference tree not found at %s" % REFERENCE)
    exe = build()
    rs = np.random.RandomState(20261019)
    obs = observations(rs)
    inp = [len(CLASSES)]
    edges = {}
    for name, cid, _model, _kind, stride in CLASSES:
        edges[name] = edges_for(stride)
        inp += [cid, MAP_W, MAP_H, SCALE, ORIGIN[0], ORIGIN[1], len(obs), *obs.ravel(), len(edges[name]), *edges[name].ravel()]
    f_in, f_out = os.path.join(OUT_DIR, "map_render_in.bin"), os.path.join(OUT_DIR, "map_render_out.bin")
    np.asarray(inp, dtype=np.float64).tofile(f_in)
    subprocess.check_call([exe, f_in, f_out, os.path.join(OUT_DIR, "map_render_scratch.pgm")])
    o = np.fromfile(f_out, dtype=np.float64)
    pos = [0]

    def take(n, shape=None):
        v = o[pos[0]:pos[0] + n]
        assert v.size == n
        pos[0] += n
        return v.reshape(shape) if shape else v

    def take_map(stride, w, h):
        geom = [int(v) for v in take(4)]
        assert geom[:2] == [w, h], "the map grew: keep the observations inside the window"
        payload = take(w * h * stride, (h, w, stride)).copy()
        value = take(w * h, (h, w)).copy()
        occ = take(w * h, (h, w)).copy()
        pgm = take(w * h, (h, w)).astype(np.uint8)
        return geom[2:], payload, value, occ, pgm

    out = dict(map_origin=np.array(ORIGIN), map_scale=np.array(SCALE), obs=obs)
    for name, _cid, model, kind, stride in CLASSES:
        origin, payload, value, occ, pgm = take_map(stride, MAP_W, MAP_H)
        assert tuple(origin) == ORIGIN
        # none of the random cells makes the reference's own conversion undefined
        assert np.all(np.isfinite(value)) and not np.any(occ == 9999), name
        out.update({name + "_model": np.array(model), name + "_occ_kind": np.array(kind), name + "_payload": payload,
                    name + "_value": value, name + "_occgrid": occ.astype(np.int8), name + "_pgm": pgm})
        n = len(edges[name])
        _, epay, eval_, eocc, epgm = take_map(stride, n, 1)
        ok = eocc[0] != 9999
        out.update({name + "_edge_payload": epay[0], name + "_edge_value": eval_[0], name + "_edge_occgrid_ok": ok,
                    name + "_edge_occgrid": np.where(ok, eocc[0], 0).astype(np.int8), name + "_edge_pgm": epgm[0]})
        print("%-17s map: %4d distinct occgrid bytes, %3d distinct pgm bytes; edges: %d (%d without an OCCGRID golden)"
              % (name, len(np.unique(occ)), len(np.unique(pgm)), n, int((~ok).sum())))
    assert pos[0] == o.size
    observed = np.zeros((MAP_H, MAP_W), bool)
    observed[(obs[:, 1] + ORIGIN[1]).astype(int), (obs[:, 0] + ORIGIN[0]).astype(int)] = True
    print("never observed: %d of %d cells" % (int((~observed).sum()), observed.size))
    # the truncation the k / 100 edges are there for
    a = out["affine_edge_value"]
    for v, want in ((0.29, 28), (0.57, 56)):
        assert out["affine_edge_occgrid"][np.flatnonzero(a == v)[0]] == want
    path = os.path.join(GOLDEN_DIR, "map_render.npz")
    np.savez_compressed(path, **out)
    print("wrote map_render.npz", os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
