"""K brute-force matches of K robots' raw scans, two routes timed side by side, K = 1, 4, 16, 64:

  (batch) ONE slamhip_matcher_process_raw_scan_batch call on a matcher with K enumerator streams
          (slamhip_matcher_set_bf_streams), the argument block made once: the assembly launch + score, scan, decide;
  (lone)  K slamhip_matcher_process_raw_scan calls on K lone matchers, one after another (four launches and a host spin
          each) -- code the batch form does not touch: the baseline.

Two ranges: the reference's brute-force preset (init_scan_matching.h:152-169: +-0.5 m in 0.1 m steps, +-5 deg in 1 deg
steps) and the sweep of p2D_ss_evaluator (pose2D_search_space_evaluator.cpp:163-171: +-1 m at 0.01 m, one heading).
Scene: occupancy cells, even weights, the benchmark's rotating scans.  Both routes see the same scans in the same order,
stream j and lone matcher j latch the same base at their first match, so they compute the same matches: checked bit for
bit on EVERY call, timed or not.  The routes alternate call by call inside every block; per route and K the median over
the blocks (the first one dropped) of the mean ms per call, and the blocks' max - min.  "no claim" where the two routes'
ranges over the blocks overlap.  Writes one JSON document to --out.  Run on the GPU box."""
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
ap.add_argument("--blocks", type=int, default=21, help="timed blocks per K (the first is dropped)")
ap.add_argument("--ms-per-block", type=float, default=150.0, help="the calls of a block are sized to about this much time")
ap.add_argument("--size", type=int, default=1000)
ap.add_argument("--beams", type=int, default=1080)
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert args.blocks >= 21, "medians of at least 20 blocks"

pkg = ge.load_package()
L = pkg.load()
_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
D = np.deg2rad
RANGES = [("reference preset", [-0.5, 0.5, 0.1, -0.5, 0.5, 0.1, -D(5.0), D(5.0), D(1.0)]),
          ("p2D_ss_evaluator", [-1.0, 1.0, 0.01, -1.0, 1.0, 0.01, 0.0, 0.0, 0.1])]
WEIGHTING = "even"

doc = {"what": "ms per call: K raw brute-force matches in one process_raw_scan_batch call (enumerator streams) against K "
               "lone process_raw_scan calls on K lone matchers", "beams": args.beams, "map_cells": args.size,
       "blocks": args.blocks - 1, "ranges": []}
ctx = pkg.Context(0)
sc = make_scene(cell_model=0, size=args.size, scale=0.05, n_beams=args.beams, seed=100, weighting=WEIGHTING)
scans = rotating_scenes(sc, args.beams, WEIGHTING)
ctx.upload_map(0, sc["map"])
for name, r9 in RANGES:
    entry = {"range": name, "range9": r9, "by_K": []}
    for K in [int(v) for v in args.ks.split(",")]:
        groups = [[(g * K + j) % len(scans) for j in range(K)] for g in range(max(1, min(4, len(scans) // K)))]
        mb = pkg.Matcher(ctx, "BF", pkg.spe_cfg(), r9)
        mb.set_bf_streams(K)
        assert L.slamhip_matcher_set_observer(mb.h, None) == 0
        blocks = [mb.make_raw_batch([dict(map_id=0, range=scans[k]["raw_range"], angle=scans[k]["raw_angle"], is_occ=scans[k]["is_occ"],
                                          weighting=WEIGHTING, init_pose=scans[k]["init_pose"]) for k in grp]) for grp in groups]
        fn = L.slamhip_matcher_process_raw_scan_batch
        fn.argtypes = [C.c_void_p, C.c_int, C.POINTER(pkg.RawMatchJob), _dp, _dp, _ip]
        bargs = [(mb.h, b["n"], b["raw_arr"], b["deltas"].ctypes.data_as(_dp), b["probs"].ctypes.data_as(_dp),
                  b["kept"].ctypes.data_as(_ip)) for b in blocks]
        lones = [pkg.Matcher(ctx, "BF", pkg.spe_cfg(), r9) for _ in range(K)]
        lone_fn = [[m.make_raw_process_scan(0, scans[k]["raw_range"], scans[k]["raw_angle"], is_occ=scans[k]["is_occ"],
                                            weighting=WEIGHTING) for m, k in zip(lones, grp)] for grp in groups]
        lone_out = np.zeros((K, 4))

        def run_batch(g):
            rc = fn(*bargs[g])
            assert rc == 0, L.slamhip_last_error()

        def run_lone(g):
            for j, (match, k) in enumerate(zip(lone_fn[g], groups[g])):
                _, prob = match(scans[k]["init_pose"])
                lone_out[j, 0] = prob
                lone_out[j, 1:] = match.delta[:]

        def same(g):
            b = blocks[g]
            return (np.array_equal(b["probs"].view(np.uint64), lone_out[:, 0].copy().view(np.uint64)) and
                    np.array_equal(b["deltas"].view(np.uint64), np.ascontiguousarray(lone_out[:, 1:]).view(np.uint64)))

        # ---- the same matches on both routes, bit for bit (and the warm-up: every group of scans twice)
        on_chain, t_pair = 0, 0.0
        for rep in range(2):
            for g in range(len(groups)):
                t0 = time.perf_counter()
                run_batch(g)
                run_lone(g)
                t_pair = time.perf_counter() - t0
                assert same(g), (name, K, g)
                on_chain = sum(mb.batch_stats(j)["on_device_chain"] for j in range(K))
        launches = mb.chain_stats()["kernels_launched"]
        calls = int(max(4, min(200, args.ms_per_block / (1e3 * t_pair))))
        # ---- timed: the routes alternate call by call (each returns after its matches have reported their results)
        ctx.synchronize()
        per = {"batch": [], "lone": []}
        for _ in range(args.blocks):
            acc = {"batch": 0.0, "lone": 0.0}
            for it in range(calls):
                g = it % len(groups)
                t0 = time.perf_counter()
                run_batch(g)
                t1 = time.perf_counter()
                run_lone(g)
                t2 = time.perf_counter()
                acc["batch"] += t1 - t0
                acc["lone"] += t2 - t1
                assert same(g), (name, K, g)
            for r in acc:
                per[r].append(1e3 * acc[r] / calls)
        row = {"K": K, "poses_per_match": int(mb.batch_stats(0)["scorer_calls"]), "matches_on_shared_launches": on_chain,
               "kernels_launched_batch": int(launches), "kernels_launched_lone": 4 * K, "calls_per_block": calls}
        for r in per:
            x = np.array(per[r][1:])  # (the first block settles clocks and caches)
            row[r] = dict(ms_per_call_median=float(np.median(x)), ms_per_call_spread=float(x.max() - x.min()),
                          ms_per_call_min=float(x.min()), ms_per_call_max=float(x.max()))
        b, lo = row["batch"], row["lone"]
        apart = b["ms_per_call_max"] < lo["ms_per_call_min"] or lo["ms_per_call_max"] < b["ms_per_call_min"]
        row["lone_over_batch"] = lo["ms_per_call_median"] / b["ms_per_call_median"] if apart else "no claim"
        entry["by_K"].append(row)
        print(json.dumps(dict(range=name, **row)), flush=True)
        for m in [mb] + lones:
            m.close()
    doc["ranges"].append(entry)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(doc, open(args.out, "w"), indent=1)
ctx.close()
