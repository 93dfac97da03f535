"""The peaks of a brute-force sweep's score landscape on two routes, timed side by side, K = 1 and 16 robots:

  (device) ONE slamhip_matcher_bf_peaks call (K = 1) or ONE slamhip_matcher_bf_peaks_batch call: the lattice scored and
           reduced to its peaks on the device, only the counts and the written peaks come back;
  (host)   the route it replaces: per robot slamhip_scan_select + slamhip_score_poses of the same poses, the scores
           downloaded, slamhip_bf_peaks_host over them.

Sweeps of 201 x 201 x 1 (the search-space evaluator's) and 41 x 41 x 21 poses, windows of radius (3, 3, 0) and (2, 2, 2),
scores within 3 % of the best, 16 peaks asked for.  1080-beam scans resident in scan slots, a 1000 x 1000 occupancy map at
0.05 m, the 1-cell estimator, default sum order, device pose trig.  The peaks of both routes are compared bit for bit on
EVERY block.  The routes alternate block by block; per route the median over the blocks (the first pair dropped) of the
mean ms per call of a block, with the blocks' min and max.  "no claim" where the two routes' [min, max] ranges overlap.
Writes one JSON document to --out.  Run on the GPU box.  (tools/bf_peaks_kernel_times.py adds the kernels' own times.)"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge  # noqa: E402
from bench_legs.common import rotating_scenes  # noqa: E402
from synth import make_scene  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--ks", default="1,16")
ap.add_argument("--blocks", type=int, default=21, help="timed blocks per route (the first is dropped)")
ap.add_argument("--ms-per-block", type=float, default=40.0, help="the calls of a block are sized to about this much time")
ap.add_argument("--size", type=int, default=1000)
ap.add_argument("--beams", type=int, default=1080)
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert args.blocks >= 21, "medians of at least 20 blocks"

pkg = ge.load_package()
SWEEPS = {"201x201x1": [-1.0, 1.0, 0.01, -1.0, 1.0, 0.01, 0.0, 0.0, 1.0],
          "41x41x21": [-0.2, 0.2, 0.01, -0.2, 0.2, 0.01, -0.1, 0.1, 0.01]}
RADII = [(3, 3, 0), (2, 2, 2)]
RATIO, MAX_PEAKS = 0.97, 16


def offsets(lo, to, step, below):
    """an axis as BruteForcePoseEnumerator accumulates it"""
    out, v = [], lo
    while True:
        if not below and not v <= to:
            return out
        out.append(v)
        if below and not v < to:
            return out
        v += step


def lattice(r9, centre):
    xs, ys, ts = offsets(*r9[0:3], True), offsets(*r9[3:6], True), offsets(*r9[6:9], False)
    poses = np.array([(centre[0] + x, centre[1] + y, centre[2] + t) for t in ts for y in ys for x in xs])
    return (len(xs), len(ys), len(ts)), np.ascontiguousarray(poses)


doc = {"what": "ms per call: the peaks of K sweeps' landscapes in one slamhip_matcher_bf_peaks(_batch) call against K x "
               "(slamhip_scan_select + slamhip_score_poses + slamhip_bf_peaks_host)", "beams": args.beams,
       "map_cells": args.size, "min_ratio": RATIO, "max_peaks": MAX_PEAKS, "blocks": args.blocks - 1, "rows": []}
ctx = pkg.Context(0)
sc = make_scene(cell_model=0, size=args.size, scale=0.05, n_beams=args.beams, seed=100)
scans = rotating_scenes(sc, args.beams, "even")
ctx.upload_map(0, sc["map"])
cfg = pkg.spe_cfg()
for sweep, r9 in SWEEPS.items():
    m = pkg.Matcher(ctx, "BF", pkg.spe_cfg(), r9)
    for K in [int(v) for v in args.ks.split(",")]:
        for k in range(K):
            s = scans[k % len(scans)]
            ctx.scan_store(k, s["range"], *pkg.beam_trig(s["angle"]), s["weight"])
        centres = [np.array(scans[k % len(scans)]["init_pose"], dtype=np.float64) for k in range(K)]
        shape, _ = lattice(r9, centres[0])
        poses = [lattice(r9, c)[1] for c in centres]
        jobs = m.make_batch([dict(map_id=0, scan_slot=k, init_pose=centres[k]) for k in range(K)])
        for radius in RADII:
            res = {}

            def run_device():
                if K == 1:
                    ctx.scan_select(0)
                    res["device"] = [m.bf_peaks(0, centres[0], radius, RATIO, 0.0, MAX_PEAKS)]
                else:
                    res["device"] = m.bf_peaks_batch(jobs, radius, RATIO, 0.0, MAX_PEAKS)

            def run_host():
                out = []
                for k in range(K):
                    ctx.scan_select(k)
                    out.append(pkg.bf_peaks_host(ctx.score_poses(0, cfg, poses[k]), shape, radius, RATIO, 0.0, MAX_PEAKS))
                res["host"] = out

            def same():
                return all(d["n_found"] == h["n_found"] and np.array_equal(d["index"], h["index"]) and
                           np.array_equal(d["scores"].view(np.uint64), h["scores"].view(np.uint64))
                           for d, h in zip(res["device"], res["host"]))

            t_pair = 0.0
            for _ in range(3):  # warm-up, and the same peaks on both routes bit for bit
                t0 = time.perf_counter()
                run_device()
                run_host()
                t_pair = time.perf_counter() - t0
                assert same(), (sweep, K, radius)
            stats = m.bf_peaks_stats()
            calls = int(max(2, min(200, args.ms_per_block / (1e3 * t_pair / 2))))
            ctx.synchronize()
            per = {"device": [], "host": []}
            for _ in range(args.blocks):
                for route, run in (("device", run_device), ("host", run_host)):
                    t0 = time.perf_counter()
                    for _c in range(calls):
                        run()
                    per[route].append(1e3 * (time.perf_counter() - t0) / calls)
                    assert same(), (sweep, K, radius, route)
            row = {"sweep": sweep, "shape": list(shape), "K": K, "radius": list(radius), "launches_device": stats["launches"],
                   "on_shared_launch": stats["on_shared_launch"], "survivors_bound": stats["survivors_bound"],
                   "n_found": [int(d["n_found"]) for d in res["device"]], "calls_per_block": calls}
            for r in per:
                x = np.array(per[r][1:])  # (the first block settles clocks and caches)
                row[r] = dict(ms_per_call_median=float(np.median(x)), ms_per_call_min=float(x.min()), ms_per_call_max=float(x.max()))
            d, h = row["device"], row["host"]
            # (a ratio only where the two ranges do not overlap)
            inside = not (d["ms_per_call_max"] < h["ms_per_call_min"] or h["ms_per_call_max"] < d["ms_per_call_min"])
            row["host_over_device"] = "no claim" if inside else h["ms_per_call_median"] / d["ms_per_call_median"]
            doc["rows"].append(row)
            print("%-9s K %2d radius %s: device %.4f [%.4f - %.4f] ms, host %.4f [%.4f - %.4f] ms, host / device %s"
                  % (sweep, K, radius, d["ms_per_call_median"], d["ms_per_call_min"], d["ms_per_call_max"], h["ms_per_call_median"],
                     h["ms_per_call_min"], h["ms_per_call_max"], row["host_over_device"] if inside else "%.2f" % row["host_over_device"]),
                  flush=True)
    m.close()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(doc, open(args.out, "w"), indent=1)
ctx.close()
