#!/usr/bin/env python3
"""Time scan generation on the evaluator's geometry: to_lsp(100, 270, 1000) (1001 beams of up to ~1400 cells at 0.1 m)
over a walled room, K poses a call.

    python tools/scan_generate_ms.py [--poses 1 16 256] [--reps 20] [--side 400]

Prints one JSON line: per K the median wall time of a whole call (upload of poses and angles, kernel, one copy back) and
the kernel's own time (slamhip_profile_read) for the wave form and for the forced sequential form, the host entry's
time, and -- where the compiled reference (oracle/_ref) is present -- the reference generator's time per pose, measured
BEFORE the GPU is initialised.  All four compute the same scans; the tool checks that before it reports."""
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


def room(side, scale):
    """an occupancy map: a wall around the window, a few pillars inside"""
    p = np.full((side, side, 1), 0.01)
    p[:2], p[-2:], p[:, :2], p[:, -2:] = 1.0, 1.0, 1.0, 1.0
    rs = np.random.RandomState(5)
    for _ in range(12):
        x, y = rs.randint(20, side - 24, 2)
        p[y:y + 4, x:x + 4] = 1.0
    half = side // 2
    p[half - 6:half + 6, half - 6:half + 6] = 0.01  # room for the robot
    return types.SimpleNamespace(cell_model=0, payload=p, origin=(half, half), scale=scale, unknown=np.array([0.5]), width=side,
                                 height=side)


def poses_for(k):
    rs = np.random.RandomState(k)
    return np.column_stack([0.05 + 0.4 * (rs.rand(k) - 0.5), 0.05 + 0.4 * (rs.rand(k) - 0.5) + 0.003, rs.rand(k) * 6.28 - 3.14])


def reference_ms(m, poses, reps):
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import pyoracle as po
    if not po.ref_available():
        return None, None
    R = po.Ref()
    rm = R.map_create(po.REF_CELL_MOCK, po.MAP_UNBOUNDED_PLAIN, m.width, m.height, m.scale, 0.5)
    ys, xs = np.nonzero(m.payload[..., 0] != 0.5)
    for x, y in zip(xs, ys):
        rm.update(int(x) - m.origin[0], int(y) - m.origin[1], float(m.payload[y, x, 0]), qual=1.0, is_occ=True, quality=1.0)
    g = rm.geometry()
    assert (g["width"], g["height"]) == (m.width, m.height) and tuple(g["origin"]) == tuple(m.origin), g
    times, scans = [], []
    for p in poses:
        best = float("inf")
        for _ in range(reps):
            t0 = time.perf_counter()
            sc = R.scan_generate(rm, p, 100, 270, 1000, 1.0)
            best = min(best, time.perf_counter() - t0)
        times.append(best)
        scans.append(sc.get()[:2])
    return 1e3 * float(np.median(times)), scans


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", type=int, nargs="+", default=[1, 16, 256])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--side", type=int, default=400)
    a = ap.parse_args()
    pkg = ge.load_package()
    m = room(a.side, 0.1)
    max_dist, inc, hs = pkg.to_lsp(100, 270, 1000)
    angles = pkg.scan_gen_angles(hs, inc)
    out = dict(tool="scan_generate_ms", side=a.side, beams=int(angles.size), sincos_variant=pkg.scan_gen_libm_variant())
    ref_ms, ref_scans = reference_ms(m, poses_for(4), max(3, a.reps // 4))  # (before the first HIP call)
    out["reference_ms_per_pose"] = ref_ms
    t0 = time.perf_counter()
    host = pkg.generate_scans_host(m, poses_for(4), angles, max_dist, 1.0)
    out["host_entry_ms_per_pose"] = 1e3 * (time.perf_counter() - t0) / 4
    if ref_scans is not None:
        for k, scan in enumerate(pkg.compact_scans(host[0], host[1], angles)):
            assert np.array_equal(scan[0], ref_scans[k][0]) and np.array_equal(scan[1], ref_scans[k][1]), "host != reference"
    ctx = pkg.Context(0)
    ctx.upload_map(0, m)
    for k in a.poses:
        poses = poses_for(k)
        want = pkg.generate_scans_host(m, poses, angles, max_dist, 1.0) if k <= 16 else None
        for name, seq in (("wave", False), ("sequential", True)):
            got = ctx.generate_scans(0, poses, angles, max_dist, 1.0, sequential=seq)  # warm-up, and the check
            if want is not None:
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), name + " != host"
            wall = []
            ctx.profile_enable(True)
            ctx.profile_read()
            for _ in range(a.reps):
                t0 = time.perf_counter()
                ctx.generate_scans(0, poses, angles, max_dist, 1.0, sequential=seq)
                wall.append(time.perf_counter() - t0)
            prof = ctx.profile_read()
            ctx.profile_enable(False)
            out["%s_k%d" % (name, k)] = dict(call_ms_median=1e3 * float(np.median(wall)),
                                             kernel_ms_mean=float(prof[0]) / max(1, a.reps))
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
