"""The pose sets of K robots scored on two routes, timed side by side, K = 1, 4, 16, 64:

  (batch) ONE slamhip_score_poses_batch call over a job table made once: one copy of the call's arena, one scoring launch;
  (lone)  K x (slamhip_scan_select + slamhip_score_poses), one after another -- code the batch form does not touch: the
          baseline.

Shapes a user runs: 1080-beam scans (the benchmark's rotating scans, one per robot, resident in scan slots), a 2000 x 2000
map at 0.05 m (robot j on map j mod 4: four resident copies), P = 6 poses per robot (one hill-climbing round around its
initial pose) and P = 1332 (the reference's brute-force preset, init_scan_matching.h:152-169: +-0.5 m in 0.1 m steps,
+-5 deg in 1 deg steps, and the initial pose).  Occupancy cells with even weights and TBM cells (through the probability
plane) with viny weights, the 1-cell estimator and the max estimator over a 3 x 3-cell window; default sum order, device
pose trig.  Both routes return with their scores in host memory; the scores are compared bit for bit on EVERY run, timed
or not.  The routes alternate block by block (batch block, lone block, ...); per route the median over the blocks (the
first pair dropped) of the mean ms per call of a block, with the blocks' min and max.  "no claim" where one route's
median lies inside the other's [min, max].  Writes one JSON document to --out.  Run on the GPU box."""
import argparse
import ctypes as C
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
ap.add_argument("--ks", default="1,4,16,64")
ap.add_argument("--ps", default="6,1332")
ap.add_argument("--blocks", type=int, default=21, help="timed blocks per route (the first is dropped)")
ap.add_argument("--ms-per-block", type=float, default=40.0, help="the calls of a block are sized to about this much time")
ap.add_argument("--size", type=int, default=2000)
ap.add_argument("--beams", type=int, default=1080)
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert args.blocks >= 21, "medians of at least 20 blocks"

pkg = ge.load_package()
L = pkg.load()
_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
L.slamhip_score_poses_batch.argtypes = [C.c_void_p, C.POINTER(pkg.SpeCfg), C.c_int, C.POINTER(pkg.ScoreJob), _dp]
N_MAPS = 4
SCALE = 0.05
WINDOW = (-SCALE, SCALE, -SCALE, SCALE)  # the max estimator's analysis area: 3 x 3 cells around the end point


def pose_set(init, p):
    """p poses around `init`: 6 = one hill-climbing round (+- 0.1 m in x, in y, +- 0.1 rad), 1332 = the brute-force preset"""
    if p == 6:
        d = np.array([[0.1, 0, 0], [-0.1, 0, 0], [0, 0.1, 0], [0, -0.1, 0], [0, 0, 0.1], [0, 0, -0.1]])
        return init + d
    if p == 1332:
        xy, th = np.linspace(-0.5, 0.5, 11), np.deg2rad(np.linspace(-5.0, 5.0, 11))
        gx, gy, gt = np.meshgrid(xy, xy, th, indexing="ij")
        return np.vstack([init, init + np.stack([gx.ravel(), gy.ravel(), gt.ravel()], axis=1)])
    rs = np.random.RandomState(p)
    return init + rs.randn(p, 3) * [0.2, 0.2, 0.05]


doc = {"what": "ms per call: the pose sets of K robots in one slamhip_score_poses_batch call against K x (slamhip_scan_select + "
               "slamhip_score_poses)", "beams": args.beams, "map_cells": args.size, "scale": SCALE, "resident_maps": N_MAPS,
       "blocks": args.blocks - 1, "scenes": []}
ctx = pkg.Context(0)
for cell_name, cell, weighting in (("OCC even", 0, "even"), ("TBM viny", 1, "viny")):
    sc = make_scene(cell_model=cell, size=args.size, scale=SCALE, n_beams=args.beams, seed=100, weighting=weighting)
    scans = rotating_scenes(sc, args.beams, weighting)
    for j in range(N_MAPS):
        ctx.upload_map(j, sc["map"])
    for oope_name, oope in (("obstacle", pkg.OOPE_OBSTACLE), ("max", pkg.OOPE_MAX)):
        cfg = pkg.spe_cfg(oope=oope, area=WINDOW)
        entry = {"cells": cell_name, "oope": oope_name, "rows": []}
        for P in [int(v) for v in args.ps.split(",")]:
            for K in [int(v) for v in args.ks.split(",")]:
                for k in range(K):
                    s = scans[k % len(scans)]
                    ctx.scan_store(k, s["range"], *pkg.beam_trig(s["angle"]), s["weight"])
                poses = [np.ascontiguousarray(pose_set(scans[k % len(scans)]["init_pose"], P)) for k in range(K)]
                table = (pkg.ScoreJob * K)()
                for k in range(K):
                    table[k].map_id, table[k].scan_slot, table[k].n_poses = k % N_MAPS, k, P
                    table[k].poses_xyt = poses[k].ctypes.data_as(_dp)
                out_batch, out_lone = np.zeros(K * P), np.zeros(K * P)
                batch_args = (ctx.h, C.byref(cfg), K, table, out_batch.ctypes.data_as(_dp))
                lone_args = [(ctx.h, k % N_MAPS, C.byref(cfg), P, poses[k].ctypes.data_as(_dp),
                              out_lone[k * P:].ctypes.data_as(_dp)) for k in range(K)]

                def run_batch():
                    rc = L.slamhip_score_poses_batch(*batch_args)
                    assert rc == 0, L.slamhip_last_error()

                def run_lone():
                    for k in range(K):
                        rc = L.slamhip_scan_select(ctx.h, k) or L.slamhip_score_poses(*lone_args[k])
                        assert rc == 0, L.slamhip_last_error()

                def same():
                    return np.array_equal(out_batch.view(np.uint64), out_lone.view(np.uint64))

                # ---- warm-up, and the same scores on both routes bit for bit
                t_pair = 0.0
                for _ in range(3):
                    out_batch[:], out_lone[:] = np.nan, -1.0
                    t0 = time.perf_counter()
                    run_batch()
                    run_lone()
                    t_pair = time.perf_counter() - t0
                    assert same(), (cell_name, oope_name, P, K)
                stats = ctx.score_poses_batch_stats()
                calls = int(max(4, min(400, args.ms_per_block / (1e3 * t_pair / 2))))
                # ---- timed: the routes alternate block by block
                ctx.synchronize()
                per = {"batch": [], "lone": []}
                for _ in range(args.blocks):
                    for route, run in (("batch", run_batch), ("lone", run_lone)):
                        t0 = time.perf_counter()
                        for _c in range(calls):
                            run()
                        per[route].append(1e3 * (time.perf_counter() - t0) / calls)
                        assert same(), (cell_name, oope_name, P, K, route)
                row = {"P": P, "K": K, "jobs_in_shared_launches": stats["jobs_shared"], "jobs_lone": stats["jobs_lone"],
                       "scoring_launches_batch": stats["launches"], "scoring_launches_lone": K, "calls_per_block": calls}
                for r in per:
                    x = np.array(per[r][1:])  # (the first block settles clocks and caches)
                    row[r] = dict(ms_per_call_median=float(np.median(x)), ms_per_call_min=float(x.min()), ms_per_call_max=float(x.max()))
                b, lo = row["batch"], row["lone"]
                inside = (lo["ms_per_call_min"] <= b["ms_per_call_median"] <= lo["ms_per_call_max"] or
                          b["ms_per_call_min"] <= lo["ms_per_call_median"] <= b["ms_per_call_max"])
                row["lone_over_batch"] = "no claim" if inside else lo["ms_per_call_median"] / b["ms_per_call_median"]
                entry["rows"].append(row)
                print("%s %-8s P %4d K %2d: batch %.4f [%.4f - %.4f] ms, lone %.4f [%.4f - %.4f] ms, lone / batch %s"
                      % (cell_name, oope_name, P, K, b["ms_per_call_median"], b["ms_per_call_min"], b["ms_per_call_max"],
                         lo["ms_per_call_median"], lo["ms_per_call_min"], lo["ms_per_call_max"],
                         row["lone_over_batch"] if inside else "%.2f" % row["lone_over_batch"]), flush=True)
        doc["scenes"].append(entry)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(doc, open(args.out, "w"), indent=1)
ctx.close()
