#!/usr/bin/env python3
"""Generate tests/golden/window_oope.npz from the COMPILED REFERENCE (oracle/_ref/libslamref.so, `make -C oracle ref`):
the window observation-probability estimators -- Max / Mean / OverlapWeighted OccupancyObservationPE
(src/core/scan_matchers/occupancy_observation_probability.h:29-99) -- on analysis areas that are NOT squares around the
point: oblong, off-centre, lines, the point, one cell, sub-cell, an area that underflows to 0, 30 x 21 cells.

    python tests/golden/make_golden_window_oope.py

Maps (23 x 17 cells, origin (11, 8), every cell a distinct value written through GridMap::update):
  occ10   MeanProbabilityCell at scale 0.1
  occ07   the same values at scale 0.07 (not representable)
  tbm10   TBM cells at 0.1, a few random updates per cell
Per map: <map>_areas [12, 4] (bot, top, left, right; some depend on the scale), <map>_points [n, 2] -- n_generic random
points (GENERIC), then the BOUNDARY set: cell corners, centres and edge midpoints around the external origin, the window's
corners, points half a cell inside and outside each rim, one point far outside -- and
<map>_prob_d [12, 3, n] = OOPE::probability under the discrepancy OIE, <map>_prob_o the same under the occupancy OIE
(GridCell maps).  The reference re-centres the area itself (LightWeightRectangle::move_center), so it is handed the
un-centred one.
Scan level: scans of 1 / 65 / 257 beams (VinySlamSPW weights, some factors != 1) behind the raw and the cached trig
provider, 16 poses (two with every end point outside the window), scan<n>_<map>_<trig> [3 areas, 3 OOPEs, 16] =
estimate_scan_probability over the wide, the off-centre and the zero-height area.

The reference is compiled with its assertions in (no NDEBUG; checked below): one that fired would have ended this
script, so reaching the end means none did.  Seeds are chosen such that no GENERIC point, no scan end point and no edge
of an area around one lies within 1e-9 cells of a cell boundary (asserted here and in tests/test_window_oope_golden.py).  A BOUNDARY point at which a for some area -- an edge of the area on a cell boundary can make intersect_internal build a rectangle with
left > right -- is probed in a forked child first, left out and listed in <map>_dropped."""
import os
import subprocess
import sys

import numpy as np

GOLDEN_DIR = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(GOLDEN_DIR))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from pyoracle import *  # noqa: E402,F401,F403
from window_oope_cases import (MAPS, MARGIN_CELLS, OOPES, SCAN_MAPS, SCAN_SIZES, TRIGS, area_margin,  # noqa: E402
                               end_points)
from make_golden import map_fields  # noqa: E402

W, H = 23, 17
AREA_NAMES = ("wide", "tall", "off_centre", "zero_width", "zero_height", "point", "one_cell", "two_by_one", "half_by_1p5",
              "tiny", "underflow", "cells_30x21")
SCAN_AREAS = ("wide", "off_centre", "zero_height")
N_GENERIC = 40
N_POSES = 16


def areas_of(S):
    return np.array([(-0.03, 0.03, -0.17, 0.17), (-0.17, 0.17, -0.03, 0.03), (-0.02, 0.10, -0.07, 0.01),
                     (-0.12, 0.12, 0.0, 0.0), (0.0, 0.0, -0.12, 0.12), (0.0, 0.0, 0.0, 0.0), (0.0, S, 0.0, S),
                     (0.0, 2 * S, 0.0, S), (0.0, S / 2, 0.0, 1.5 * S), (0.0, 1e-9, 0.0, 1e-8), (0.0, 1e-170, 0.0, 1e-170),
                     (0.0, 3.05, 0.0, 2.1)])


def boundary_points(S, origin):
    ox, oy = origin
    pts = [(i * S, j * S) for i in range(-2, 3) for j in range(-2, 3)]                    # cell corners
    pts += [((i + 0.5) * S, (j + 0.5) * S) for i in range(-2, 2) for j in range(-2, 2)]  # centres
    pts += [((i + 0.5) * S, j * S) for i in (-1, 0) for j in (-1, 0, 1)]                 # edge midpoints
    pts += [(i * S, (j + 0.5) * S) for i in (-1, 0, 1) for j in (-1, 0)]
    x0, x1, y0, y1 = -ox * S, (W - ox) * S, -oy * S, (H - oy) * S                         # the window's rim
    pts += [(x0, y0), (x1, y0), (x0, y1), (x1, y1)]
    pts += [(x0 + S / 2, S / 2), (x0 - S / 2, S / 2), (x1 - S / 2, -S / 2), (x1 + S / 2, -S / 2),
            (S / 2, y0 + S / 2), (S / 2, y0 - S / 2), (-S / 2, y1 - S / 2), (-S / 2, y1 + S / 2)]
    pts.append((40.0, -35.5))
    return np.array(pts, dtype=np.float64)


def generic_points(S, areas, seed):
    """N_GENERIC random points over the window and half a cell beyond, the first seed at which the margin holds"""
    while True:
        rs = np.random.RandomState(seed)
        pts = np.stack([rs.uniform(-12.5 * S, 13.5 * S, N_GENERIC), rs.uniform(-9.5 * S, 10.5 * S, N_GENERIC)], axis=1)
        if min(area_margin(pts, a, S) for a in areas) > MARGIN_CELLS:
            return pts, seed
        seed += 1


def oies_of(md):
    return (("d", OIE_DISCREPANCY),) + ((("o", OIE_OCCUPANCY),) if md.cell_model == CELL_OCC else ())


def survives(R, m, areas, oies, p):
    """whether the reference evaluates every (area, OOPE, OIE) case at point p without one of its assertions: tried in a
    forked child, which an assertion ends.  On a BOUNDARY point an edge of an area can fall on a cell boundary, where
    LightWeightRectangle::intersect_internal can put together a rectangle with left > right (geometry_primitives.h:173)."""
    sys.stdout.flush()
    pid = os.fork()
    if pid == 0:
        os.dup2(os.open(os.devnull, os.O_WRONLY), 2)
        for area in areas:
            for _n, kind in OOPES:
                for _o, oie in oies:
                    R.oope_probability(kind, oie, m, p[0], p[1], area)
        os._exit(0)
    return os.waitpid(pid, 0)[1] == 0


def build_maps(R):
    rs = np.random.RandomState(20261018)
    occ_vals = rs.permutation(W * H) / float(W * H - 1) * 0.98 + 0.01
    maps = {}
    for name, scale in (("occ10", 0.1), ("occ07", 0.07)):
        m = R.map_create(REF_CELL_MEAN, MAP_UNBOUNDED_PLAIN, W, H, scale)
        for k, v in enumerate(occ_vals):
            m.update(k % W - W // 2, k // W - H // 2, v, 0.9)
        maps[name] = m
    m = R.map_create(REF_CELL_TBM, MAP_UNBOUNDED_PLAIN, W, H, 0.1)
    for k in range(W * H):
        for _ in range(rs.randint(2, 5)):
            m.update(k % W - W // 2, k // W - H // 2, rs.uniform(0.05, 0.95), rs.uniform(0.2, 0.9), is_occ=rs.rand() < 0.5)
    maps["tbm10"] = m
    for name, m in maps.items():
        md = m.to_data()
        assert (md.width, md.height, md.origin) == (W, H, (W // 2, H // 2)), name
        cells = md.payload.reshape(W * H, -1)
        assert len(np.unique(cells, axis=0)) == W * H, name  # every cell a distinct value
    return maps


def make_scan(R, rs, n, trig):
    a_min, inc = -2.2, 4.4 / max(n, 2)
    ang = np.zeros(n)
    a = a_min
    for k in range(n):  # accumulated, as CachedTrigonometryProvider::update builds its table
        ang[k] = a
        a += inc
    rng = rs.uniform(0.05, 0.9, n)
    a_max_passed = ang[-1] + 2 * inc
    return R.scan_create(rng, ang, None, trig, a_min, a_max_passed, inc), rng, ang, a_min, inc, a_max_passed


def scan_level(R, maps, areas, out):
    seed = 77
    while True:  # the first seed at which the margin holds for every (pose, beam) end point
        rs = np.random.RandomState(seed)
        poses = np.stack([rs.uniform(-0.4, 0.6, N_POSES), rs.uniform(-0.3, 0.4, N_POSES), rs.uniform(-np.pi, np.pi, N_POSES)], axis=1)
        poses[2] = [40.0, 40.0, 0.3]      # every end point outside the window: the prototype cell
        poses[9] = [-35.5, 12.25, -2.0]
        scans, ok = {}, True
        for n in SCAN_SIZES:
            raw = make_scan(R, np.random.RandomState(seed + n), n, TRIG_RAW)
            scans[n] = raw
            pts = end_points(ScanData(raw[1], raw[2]), poses)
            ok &= all(area_margin(pts, areas[AREA_NAMES.index(nm)], 0.1) > MARGIN_CELLS for nm in SCAN_AREAS)
        if ok:
            break
        seed += 1
    out["scan_poses"], out["scan_seed"] = poses, np.array(seed)
    out["scan_area_idx"] = np.array([AREA_NAMES.index(nm) for nm in SCAN_AREAS])
    n_cases = 0
    for n in SCAN_SIZES:
        _h, rng, ang, a_min, inc, a_max_passed = scans[n]
        pre = "scan%d_" % n
        frs = np.random.RandomState(1000 + n)
        factor = np.where(frs.rand(n) < 0.3, frs.uniform(0.1, 0.9, n), 1.0)
        factor[0] = 0.75
        for tname, trig in TRIGS:
            scan = R.scan_create(rng, ang, None, trig, a_min, a_max_passed, inc)
            for mname in SCAN_MAPS:
                sc = np.zeros((len(SCAN_AREAS), len(OOPES), N_POSES))
                for oi, (_oname, kind) in enumerate(OOPES):
                    spe = R.spe_create(kind, OIE_DISCREPANCY, 1)  # VinySlamSPW: unequal weights
                    fs = R.filter_scan(spe, scan, (0.0, 0.0, 0.0), maps[mname])
                    assert fs.size() == n  # unbounded map, every point occupied: nothing is filtered
                    for b in range(n):
                        fs.ref.lib.ref_scan_set_factor(fs.h, b, float(factor[b]))
                    fr, fa, _fo, ff = fs.get()
                    assert np.array_equal(fr, rng) and np.array_equal(fa, ang) and np.array_equal(ff, factor)
                    out[pre + "weight"] = R.scan_weights(spe, fs)
                    for ai, nm in enumerate(SCAN_AREAS):
                        sc[ai, oi] = R.score(spe, fs, maps[mname], poses, areas[AREA_NAMES.index(nm)])
                        n_cases += N_POSES
                assert np.all(np.isfinite(sc))
                out["%s%s_%s" % (pre, mname, tname)] = sc
            if trig == TRIG_CACHED:
                out[pre + "tab_sin"], out[pre + "tab_cos"] = scan.trig_table()
        assert n == 1 or len(np.unique(out[pre + "weight"])) > n // 2  # unequal weights
        out.update({pre + "range": rng, pre + "angle": ang, pre + "factor": factor, pre + "a_min": np.array(a_min),
                    pre + "a_inc": np.array(inc), pre + "a_max_passed": np.array(a_max_passed)})
    return n_cases


def main():
    if not ref_available():
        sys.exit("oracle/_ref/libslamref.so missing: run `make -C oracle ref` where the reference tree exists")
    so = os.path.join(ROOT, "oracle", "_ref", "libslamref.so")
    assert "__assert_fail" in subprocess.check_output(["nm", "-D", "--undefined-only", so]).decode(), \
        "the reference was compiled without its assertions"
    R = Ref()
    maps = build_maps(R)
    out = dict(area_names=np.array(AREA_NAMES), n_generic=np.array(N_GENERIC))
    n_cases = 0
    for mi, name in enumerate(MAPS):
        md = maps[name].to_data()
        S = md.scale
        areas = areas_of(S)
        generic, seed = generic_points(S, areas, 100 * (mi + 1))
        boundary = boundary_points(S, md.origin)
        keep = np.array([survives(R, maps[name], areas, oies_of(md), p) for p in boundary])
        assert all(survives(R, maps[name], areas, oies_of(md), p) for p in generic)
        out[name + "_dropped"] = boundary[~keep].reshape(-1, 2)
        for p in boundary[~keep]:
            print("%s: BOUNDARY point (%r, %r) left out, a reference assertion fires there" % (name, p[0], p[1]))
        pts = np.concatenate([generic, boundary[keep]])
        out.update(map_fields(md, name + "_map_"))
        out[name + "_areas"], out[name + "_points"], out[name + "_seed"] = areas, pts, np.array(seed)
        for oname, oie in oies_of(md):
            prob = np.zeros((len(areas), len(OOPES), len(pts)))
            for ai, area in enumerate(areas):
                for oi, (_n, kind) in enumerate(OOPES):
                    for pi, (x, y) in enumerate(pts):
                        prob[ai, oi, pi] = R.oope_probability(kind, oie, maps[name], x, y, area)
            assert np.all(np.isfinite(prob))
            out["%s_prob_%s" % (name, oname)] = prob
            n_cases += prob.size
    n_scan = scan_level(R, maps, areas_of(0.1), out)
    path = os.path.join(GOLDEN_DIR, "window_oope.npz")
    np.savez_compressed(path, **out)
    print("wrote window_oope.npz %d KiB: %d point cases (%s points per map, %d of them GENERIC) + %d scan-level scores, "
          "no reference assertion fired" % (os.path.getsize(path) // 1024, n_cases,
                                            " / ".join(str(len(out[nm + "_points"])) for nm in MAPS), N_GENERIC, n_scan))


if __name__ == "__main__":
    main()
