#!/usr/bin/env python3
"""Time scan generation from per-particle maps: K particles x the evaluator's to_lsp(100, 270, 1000) (1001 beams) at the
particle-map bench scene's scale (0.05 m), ms per call, two routes that compute the same arrays:

  tiled   GmappingFilter.generate_particle_scans -- one launch over the tile pool for all K particles
  detour  what it replaces: per particle particle_map (the 40-byte-per-cell download of the window) -> upload_map under a
          spare map id -> Context.generate_scans

    python tools/particle_scan_generate_ms.py [--particles 1 8 64] [--blocks 20] [--side 768] [--out FILE]

Per K: both routes once as a warm-up, then `blocks` blocks of (tiled, detour) alternating, each call timed by the host
clock (both end in a stream synchronise) and its arrays compared bit for bit with the other route's on EVERY call.  Prints
(and writes to --out) one JSON record: per K and route the median, minimum and maximum of the blocks, and a speed-up only
where the slower route's fastest block is still slower than the faster route's slowest block -- otherwise "no claim".
Needs a GPU; there is no fall-back."""
import argparse
import json
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

SCALE = 0.05
THRESHOLD = 0.5


def room(side):
    """a GMAPPING map: observed free space, a wall around the window, a few pillars inside"""
    p = np.zeros((side, side, 3))
    p[:2, :, 0], p[-2:, :, 0], p[:, :2, 0], p[:, -2:, 0] = 1.0, 1.0, 1.0, 1.0
    rs = np.random.RandomState(5)
    for _ in range(12):
        x, y = rs.randint(20, side - 24, 2)
        p[y:y + 4, x:x + 4, 0] = 1.0
    half = side // 2
    p[half - 12:half + 12, half - 12:half + 12, 0] = 0.0  # room for the robot
    return types.SimpleNamespace(cell_model=2, payload=p, origin=(half, half), scale=SCALE, unknown=np.array([-1.0, 0.0, 0.0]),
                                 width=side, height=side)


def poses_for(k, seed=0):
    rs = np.random.RandomState(seed + k)
    return np.column_stack([0.013 + 0.4 * (rs.rand(k) - 0.5), 0.017 + 0.4 * (rs.rand(k) - 0.5), rs.rand(k) * 6.28 - 3.14])


def stats(ms):
    return dict(median_ms=float(np.median(ms)), min_ms=float(np.min(ms)), max_ms=float(np.max(ms)), blocks=len(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--blocks", type=int, default=20)
    ap.add_argument("--side", type=int, default=768, help="cells a side of the room: a multiple of 256")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.side % 256 == 0
    pkg = ge.load_package()
    m = room(a.side)
    half = a.side // 2
    max_dist, inc, hs = pkg.to_lsp(100, 270, 1000)
    angles = pkg.scan_gen_angles(hs, inc)
    variant = pkg.scan_gen_libm_variant()
    out = dict(tool="particle_scan_generate_ms", side=a.side, scale=SCALE, beams=int(angles.size), max_dist=max_dist,
               occ_threshold=THRESHOLD, sincos_variant=variant, window_bytes_per_particle=40 * a.side * a.side, results={})
    ctx = pkg.Context(0)
    ctx.upload_map(0, m)
    ring_r, ring_a = np.full(180, 3.0), np.linspace(-np.pi, np.pi, 180, endpoint=False)
    for k in a.particles:
        pf = pkg.GmappingFilter(ctx, pkg.gmapping_params(), k, np.arange(100, 100 + k, dtype=np.uint32))
        pf.enable_particle_maps(0, extent_tiles=a.side // 128, pool_tiles=(a.side // 128) ** 2 + 9 * k + 8)
        particles = np.arange(k, dtype=np.int32)
        poses = poses_for(k)
        # the maps diverge: every particle appends its own ring of obstacles 3 m around a pose of its own
        pf.particle_maps_append(particles, poses_for(k, seed=1000), ring_r, ring_a)

        def tiled():
            return pf.generate_particle_scans(particles, angles, max_dist, poses=poses, occ_threshold=THRESHOLD, variant=variant)

        def detour():
            rng, st = np.zeros((k, angles.size)), np.zeros((k, angles.size), np.uint8)
            for i in range(k):
                payload, _ = pf.particle_map(i, -half, -half, a.side, a.side)
                ctx.upload_map(1, types.SimpleNamespace(cell_model=2, payload=payload, origin=(half, half), scale=SCALE,
                                                        unknown=m.unknown, width=a.side, height=a.side))
                r, s = ctx.generate_scans(1, poses[i:i + 1], angles, max_dist, THRESHOLD, 0, variant)
                ctx.map_release(1)  # (binding over a bound id would copy the old window first)
                rng[i], st[i] = r[0], s[0]
            return rng, st

        want = tiled()  # warm-up of both routes, and the first check
        got = detour()
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0]), "the routes differ (warm-up, K = %d)" % k
        t_tiled, t_detour = [], []
        for _ in range(a.blocks):
            t0 = time.perf_counter()
            x = tiled()
            t1 = time.perf_counter()
            y = detour()
            t2 = time.perf_counter()
            t_tiled.append(1e3 * (t1 - t0))
            t_detour.append(1e3 * (t2 - t1))
            assert np.array_equal(x[1], y[1]) and np.array_equal(x[0], y[0]), "the routes differ (K = %d)" % k
            assert np.array_equal(x[1], want[1]) and np.array_equal(x[0], want[0]), "a route changed its result (K = %d)" % k
        res = dict(tiled=stats(t_tiled), detour=stats(t_detour), hits=int(np.count_nonzero(want[1] == 1)),
                   assert_beams=int(np.count_nonzero(want[1] == 2)))
        if res["tiled"]["max_ms"] < res["detour"]["min_ms"]:
            res["speedup_of_medians"] = res["detour"]["median_ms"] / res["tiled"]["median_ms"]
        elif res["detour"]["max_ms"] < res["tiled"]["min_ms"]:
            res["speedup_of_medians"] = res["detour"]["median_ms"] / res["tiled"]["median_ms"]  # (below 1: the detour is faster)
        else:
            res["speedup_of_medians"] = "no claim"
        out["results"]["k%d" % k] = res
        pf.close()
    ctx.close()
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
