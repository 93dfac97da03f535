"""K Monte-Carlo matches of K robots' raw scans, two routes timed side by side at the reference's own preset (failed
attempts 20, attempts 100: common/monte_carlo_scan_matching.properties), K = 1, 4, 8, 16, 64:

  (batch) ONE slamhip_matcher_process_raw_scan_batch call on a matcher with K engine streams
          (slamhip_matcher_set_mc_streams), the argument block made once;
  (lone)  K slamhip_matcher_process_raw_scan calls on K lone matchers seeded like the streams, one after another -- code
          the batch form does not touch: the baseline.

Scenes: the tinySLAM preset (occupancy cells, even weights) and the vinySLAM preset (TBM cells, viny weights), 1080 beams,
2000 x 2000 cells @ 0.05 m, the benchmark's rotating scans.  Both routes see the same scans in the same order on the
same seeds, so they compute the same matches: checked bit for bit before anything is timed and after the timed calls.
The routes alternate call by call inside every block; per route and K the median over the blocks (the first one dropped)
of the mean ms per call, and the blocks' max - min.  From a second pass with slamhip_profile_enable: kernels launched
per call and the kernels' own time.  Beside it: super-steps per match and the candidates per job and super-step.
Writes one JSON document to --out.  Run on the GPU box."""
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
ap.add_argument("--ks", default="1,4,8,16,64")
ap.add_argument("--blocks", type=int, default=21, help="timed blocks per K (the first is dropped)")
ap.add_argument("--calls", type=int, default=160, help="calls per route and block")
ap.add_argument("--size", type=int, default=2000)
ap.add_argument("--beams", type=int, default=1080)
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert args.blocks >= 21, "medians of at least 20 blocks"

pkg = ge.load_package()
L = pkg.load()
_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
PRESETS = [("tinySLAM", 0, "even", "occupancy cells, even weights"), ("vinySLAM", 1, "viny", "TBM cells, viny weights")]
TD, RD, LIMITS = 0.2, 0.1, (20, 100)


def seeds_of(k):
    return [666666 + 7919 * j for j in range(k)]


doc = {"what": "ms per call: K raw Monte-Carlo matches in one process_raw_scan_batch call (engine streams) against K lone "
               "process_raw_scan calls on K lone matchers", "limits": {"failed_attempts": LIMITS[0], "attempts": LIMITS[1]},
       "dispersion": [TD, RD], "beams": args.beams, "map_cells": args.size, "blocks": args.blocks - 1,
       "calls_per_block": args.calls, "scenes": []}
ctx = pkg.Context(0)
for name, cell, weighting, text in PRESETS:
    sc = make_scene(cell_model=cell, size=args.size, scale=0.05, n_beams=args.beams, seed=100, weighting=weighting)
    scans = rotating_scenes(sc, args.beams, weighting)
    ctx.upload_map(0, sc["map"])
    entry = {"preset": name, "scene": text, "by_K": []}
    for K in [int(v) for v in args.ks.split(",")]:
        seeds = seeds_of(K)
        # (groups of K scans; with more robots than scans a scan serves several robots -- their engines differ)
        groups = [[(g * K + j) % len(scans) for j in range(K)] for g in range(max(1, len(scans) // K))]
        mb = pkg.Matcher(ctx, "MC", pkg.spe_cfg(), [1, TD, RD, LIMITS[0], LIMITS[1]])
        mb.set_mc_streams(seeds)
        assert L.slamhip_matcher_set_observer(mb.h, None) == 0
        blocks = [mb.make_raw_batch([dict(map_id=0, range=scans[k]["raw_range"], angle=scans[k]["raw_angle"], is_occ=scans[k]["is_occ"],
                                          weighting=weighting, init_pose=scans[k]["init_pose"]) for k in grp]) for grp in groups]
        fn = L.slamhip_matcher_process_raw_scan_batch
        fn.argtypes = [C.c_void_p, C.c_int, C.POINTER(pkg.RawMatchJob), _dp, _dp, _ip]
        bargs = [(mb.h, b["n"], b["raw_arr"], b["deltas"].ctypes.data_as(_dp), b["probs"].ctypes.data_as(_dp),
                  b["kept"].ctypes.data_as(_ip)) for b in blocks]
        lones = [pkg.Matcher(ctx, "MC", pkg.spe_cfg(), [s, TD, RD, LIMITS[0], LIMITS[1]]) for s in seeds]
        lone_fn = [[m.make_raw_process_scan(0, scans[k]["raw_range"], scans[k]["raw_angle"], is_occ=scans[k]["is_occ"],
                                            weighting=weighting) for m, k in zip(lones, grp)] for grp in groups]
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
        steps, on_chain = [], 0
        for _ in range(2):
            for g in range(len(groups)):
                run_batch(g)
                run_lone(g)
                assert same(g), (name, K, g)
                steps += [mb.batch_stats(j)["super_steps"] for j in range(K)]
                on_chain = sum(mb.batch_stats(j)["on_device_chain"] for j in range(K))
        # ---- timed: the routes alternate call by call (each returns after its matches have reported their results)
        ctx.synchronize()
        per = {"batch": [], "lone": []}
        for _ in range(args.blocks):
            acc = {"batch": 0.0, "lone": 0.0}
            for it in range(args.calls):
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
                per[r].append(1e3 * acc[r] / args.calls)
        # ---- the kernels' own time: a pass of its own with events on every dispatch
        kern = {}
        for r, run in (("batch", run_batch), ("lone", run_lone)):
            ctx.profile_enable(True)
            ctx.profile_read(reset=True)
            for it in range(args.calls):
                run(it % len(groups))
            ctx.synchronize()
            ctx.profile_enable(False)
            k_ms, k_launches, _ = ctx.profile_read(reset=True)
            kern[r] = dict(kernel_ms_per_call=k_ms / args.calls, launches_per_call=k_launches / args.calls,
                           us_per_kernel=1e3 * k_ms / max(k_launches, 1))
        row = {"K": K, "matches_on_shared_launches": on_chain, "super_steps_per_match_mean": float(np.mean(steps)),
               "super_steps_per_match_max": int(np.max(steps)),
               "candidates_per_job_and_super_step": min(511, LIMITS[0], LIMITS[1], max(1, 2048 // K - 1))}
        for r in per:
            x = np.array(per[r][1:])  # (the first block settles clocks and caches)
            row[r] = dict(ms_per_call_median=float(np.median(x)), ms_per_call_spread=float(x.max() - x.min()),
                          ms_per_call_min=float(x.min()), ms_per_call_max=float(x.max()), **kern[r])
        b, lo = row["batch"], row["lone"]
        # "no claim" where the batch's median lies inside the lone route's own spread (or the other way round)
        apart = b["ms_per_call_max"] < lo["ms_per_call_min"] or lo["ms_per_call_max"] < b["ms_per_call_min"]
        row["lone_over_batch"] = lo["ms_per_call_median"] / b["ms_per_call_median"] if apart else "no claim"
        entry["by_K"].append(row)
        print(json.dumps(dict(preset=name, **row)))
        for m in [mb] + lones:
            m.close()
    doc["scenes"].append(entry)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(doc, open(args.out, "w"), indent=1)
ctx.close()
