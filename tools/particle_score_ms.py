#!/usr/bin/env python3
"""Time pose scoring over per-particle maps: K particles x P poses each under one scan of 1001 points, at the
particle-map bench scene's scale (0.05 m) and window (768 cells a side), ms per call, two routes that compute the same
scores:

  tiled   GmappingFilter.score_particle_poses -- one scoring launch and one carry launch over the tile pool for all K jobs
  detour  what it replaces: per particle particle_map (the 40-byte-per-cell download of the window) -> upload_map under a
          spare map id -> gm_cache_reset -> scan_select -> Context.score_poses

    python tools/particle_score_ms.py [--particles 1 8 64] [--poses 1 6 1332] [--blocks 20] [--side 768] [--out FILE]

Per (K, P): both routes once as a warm-up, then `blocks` blocks of (tiled, detour) alternating, each call timed by the
host clock (both end in a stream synchronise) and its scores compared bit for bit with the other route's on EVERY call.
Prints (and writes to --out) one JSON record: per (K, P) and route the median, minimum and maximum of the blocks, and a
speed-up only where the slower route's fastest block is still slower than the faster route's slowest block -- otherwise
"no claim".  Needs a GPU; there is no fall-back."""
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
SCAN_SLOT = 0


def room(side):
    """tools/particle_scan_generate_ms.py's room -- observed free space, a wall around the window, a few pillars inside --
    with every occupied cell's obstacle mean at the centre of the cell"""
    p = np.zeros((side, side, 3))
    p[:2, :, 0], p[-2:, :, 0], p[:, :2, 0], p[:, -2:, 0] = 1.0, 1.0, 1.0, 1.0
    rs = np.random.RandomState(5)
    for _ in range(12):
        x, y = rs.randint(20, side - 24, 2)
        p[y:y + 4, x:x + 4, 0] = 1.0
    half = side // 2
    p[half - 12:half + 12, half - 12:half + 12, 0] = 0.0  # room for the robot
    ys, xs = np.mgrid[0:side, 0:side]
    occ = p[..., 0] > 0.5
    p[..., 1] = np.where(occ, (xs - half + 0.5) * SCALE, 0.0)
    p[..., 2] = np.where(occ, (ys - half + 0.5) * SCALE, 0.0)
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
    ap.add_argument("--poses", type=int, nargs="+", default=[1, 6, 1332])
    ap.add_argument("--blocks", type=int, default=20)
    ap.add_argument("--side", type=int, default=768, help="cells a side of the room: a multiple of 256")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.side % 256 == 0
    pkg = ge.load_package()
    m = room(a.side)
    half = a.side // 2
    # the scan: what the evaluator's to_lsp(100, 270, 1000) sees from the middle of the room, every beam kept (a beam that
    # hits nothing ends 3 m away), even weights
    max_dist, inc, hs = pkg.to_lsp(100, 270, 1000)
    angles = pkg.scan_gen_angles(hs, inc)
    ctx = pkg.Context(0)
    ctx.upload_map(0, m)
    rng, st = ctx.generate_scans(0, np.array([[0.013, 0.017, 0.3]]), angles, max_dist, 0.5, 0, pkg.scan_gen_libm_variant())
    scan_r = np.where(st[0] == 1, rng[0], 3.0)
    cos_a, sin_a = pkg.beam_trig(angles)
    ctx.scan_store(SCAN_SLOT, scan_r, cos_a, sin_a, np.full(angles.size, 1.0 / angles.size))
    cfg = pkg.spe_cfg(oope=pkg.OOPE_GMAPPING)
    out = dict(tool="particle_score_ms", side=a.side, scale=SCALE, beams=int(angles.size),
               window_bytes_per_particle=40 * a.side * a.side, results={})
    ring_r, ring_a = np.full(180, 3.0), np.linspace(-np.pi, np.pi, 180, endpoint=False)
    for k in a.particles:
        pf = pkg.GmappingFilter(ctx, pkg.gmapping_params(), k, np.arange(100, 100 + k, dtype=np.uint32))
        pf.enable_particle_maps(0, extent_tiles=a.side // 128, pool_tiles=(a.side // 128) ** 2 + 9 * k + 8)
        # the maps diverge: every particle appends its own ring of obstacles 3 m around a pose of its own
        pf.particle_maps_append(np.arange(k, dtype=np.int32), poses_for(k, seed=1000), ring_r, ring_a)
        centres = poses_for(k)
        for n_poses in a.poses:
            rs = np.random.RandomState(7 * k + n_poses)
            spread = np.array([0.6, 0.6, 0.2]) if n_poses > 1 else np.zeros(3)  # (one pose: the particle's own)
            jobs = [dict(particle=i, scan_slot=SCAN_SLOT, poses=centres[i] + (rs.rand(n_poses, 3) - 0.5) * spread) for i in range(k)]

            def tiled():
                return np.concatenate(pf.score_particle_poses(jobs, cfg))

            def detour():
                scores = []
                for i in range(k):
                    payload, _ = pf.particle_map(i, -half, -half, a.side, a.side)
                    ctx.upload_map(1, types.SimpleNamespace(cell_model=2, payload=payload, origin=(half, half), scale=SCALE,
                                                            unknown=m.unknown, width=a.side, height=a.side))
                    ctx.gm_cache_reset()
                    ctx.scan_select(SCAN_SLOT)
                    scores.append(ctx.score_poses(1, cfg, jobs[i]["poses"]))
                    ctx.map_release(1)  # (binding over a bound id would copy the old window first)
                return np.concatenate(scores)

            want = tiled()  # warm-up of both routes, and the first check
            assert np.array_equal(detour(), want, equal_nan=True), "the routes differ (warm-up, K = %d, P = %d)" % (k, n_poses)
            t_tiled, t_detour = [], []
            for _ in range(a.blocks):
                t0 = time.perf_counter()
                x = tiled()
                t1 = time.perf_counter()
                y = detour()
                t2 = time.perf_counter()
                t_tiled.append(1e3 * (t1 - t0))
                t_detour.append(1e3 * (t2 - t1))
                assert np.array_equal(x, y, equal_nan=True), "the routes differ (K = %d, P = %d)" % (k, n_poses)
                assert np.array_equal(x, want, equal_nan=True), "a route changed its result (K = %d, P = %d)" % (k, n_poses)
            res = dict(tiled=stats(t_tiled), detour=stats(t_detour), scores_above_zero=int(np.count_nonzero(want > 0)),
                       poses_carried=pf.particle_score_stats()["poses_carried"])
            if res["tiled"]["max_ms"] < res["detour"]["min_ms"] or res["detour"]["max_ms"] < res["tiled"]["min_ms"]:
                res["speedup_of_medians"] = res["detour"]["median_ms"] / res["tiled"]["median_ms"]  # (below 1: the detour is faster)
            else:
                res["speedup_of_medians"] = "no claim"
            out["results"]["k%d_p%d" % (k, n_poses)] = res
        pf.close()
    ctx.close()
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
