"""K raw scans to K matches, two routes timed side by side on the cfg2 scene (the headline's matcher and map, its 16
rotating scans, K = 1, 8, 16, 64):

  (a) what a caller of slamhip_matcher_process_scan_batch does with K RAW scans: per scan slamhip_filter_scan,
      slamhip_scan_weights and slamhip_beam_trig_raw on the kept points (as host/slamhip_reference_adapter.h prepares a
      filtered scan), then the batch call with the five arrays per job.  The C functions are called through ctypes on
      buffers made once; the gathers through the kept list are numpy's.
  (b) slamhip_matcher_process_raw_scan_batch on an argument block made once.
  (c) the chains alone: slamhip_matcher_process_scan_batch on scans stored in slots (no scan comes in at all) -- what
      b - c and a - c are measured against.

The routes alternate call by call inside every block; per route and K the median over the blocks of the mean ms per
call, the blocks' max - min, and -- from a second pass with slamhip_profile_enable -- the kernels' own time per call
(chains; for (b) the assembly launch as well, so kernels(b) - kernels(c) is that launch's share).  Results of (a) and
(b) are compared bit for bit before anything is timed.  --lib PATH: another build of libslamhip.so (the parent commit's)
for routes a and c.  Writes one JSON document to --out.  Run on the GPU box."""
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
from bench_legs.common import WORKLOADS, rotating_scenes  # noqa: E402
from synth import make_scene  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--ks", default="1,8,16,64")
ap.add_argument("--blocks", type=int, default=9)
ap.add_argument("--calls", type=int, default=24, help="calls per route and block")
ap.add_argument("--routes", default="a,b,c")
ap.add_argument("--lib", default=None)
ap.add_argument("--out", default=None)
args = ap.parse_args()
routes = args.routes.split(",")

pkg = ge.load_package()
if args.lib:
    pkg.LIB_PATH = os.path.abspath(args.lib)
L = pkg.load()
_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
cell, weighting, kind, params = WORKLOADS["hc"][:4]
sc = make_scene(cell_model=cell, size=2000, scale=0.05, n_beams=1080, seed=100, weighting=weighting)
scenes = rotating_scenes(sc, 1080, weighting)
ctx = pkg.Context(0)
ctx.upload_map(0, sc["map"])
for k, s in enumerate(scenes):
    c_, s_ = pkg.beam_trig(s["angle"])
    ctx.scan_store(k, s["range"], c_, s_, s["weight"])
W = {"even": 0, "viny": 1, "ahr": 2}[weighting]
mp = sc["map"]


class RouteA:
    """K raw scans through the public host functions and slamhip_matcher_process_scan_batch with arrays"""

    def __init__(self, m, idx):
        self.m, self.idx, self.K = m, idx, len(idx)
        n = 1080
        self.buf = [dict(kept=np.zeros(n, np.int32), r=np.zeros(n), a=np.zeros(n), w=np.zeros(n), c=np.zeros(n), s=np.zeros(n),
                         occ=np.ascontiguousarray(scenes[k]["is_occ"], dtype=np.int32), rng=np.ascontiguousarray(scenes[k]["raw_range"]),
                         ang=np.ascontiguousarray(scenes[k]["raw_angle"]), pose=np.ascontiguousarray(scenes[k]["init_pose"], dtype=np.float64),
                         nk=C.c_int(0)) for k in idx]
        self.arr = (pkg.MatchJob * self.K)()
        for j, (k, b) in enumerate(zip(idx, self.buf)):
            a = self.arr[j]
            a.map_id, a.scan_slot = 0, -1
            a.range, a.cos_a, a.sin_a, a.weight = (b[x].ctypes.data_as(_dp) for x in ("r", "c", "s", "w"))
            a.factor = None
            for q in range(3):
                a.init_pose[q] = float(scenes[k]["init_pose"][q])
        self.deltas, self.probs = np.zeros((self.K, 3)), np.zeros(self.K)
        self.prep_s = 0.0

    def __call__(self):
        t0 = time.perf_counter()
        for j, b in enumerate(self.buf):
            rc = L.slamhip_filter_scan(1080, b["rng"].ctypes.data_as(_dp), b["ang"].ctypes.data_as(_dp), b["occ"].ctypes.data_as(_ip),
                                       pkg.TRIG_RAW, 0.0, 1.0, 0, None, None, b["pose"].ctypes.data_as(_dp), 0, -1.0, 0, mp.width,
                                       mp.height, mp.origin[0], mp.origin[1], mp.scale, b["kept"].ctypes.data_as(_ip), C.byref(b["nk"]))
            nk = b["nk"].value
            kept = b["kept"][:nk]
            np.take(b["rng"], kept, out=b["r"][:nk])
            np.take(b["ang"], kept, out=b["a"][:nk])
            rc |= L.slamhip_scan_weights(W, nk, b["r"].ctypes.data_as(_dp), b["a"].ctypes.data_as(_dp), b["w"].ctypes.data_as(_dp))
            rc |= L.slamhip_beam_trig_raw(nk, b["a"].ctypes.data_as(_dp), b["c"].ctypes.data_as(_dp), b["s"].ctypes.data_as(_dp))
            assert rc == 0
            self.arr[j].n = nk
        self.prep_s += time.perf_counter() - t0
        rc = L.slamhip_matcher_process_scan_batch(self.m.h, self.K, self.arr, self.deltas.ctypes.data_as(_dp),
                                                  self.probs.ctypes.data_as(_dp))
        assert rc == 0, L.slamhip_last_error()


class RouteB:
    def __init__(self, m, idx):
        self.m = m
        self.blk = m.make_raw_batch([dict(map_id=0, range=scenes[k]["raw_range"], angle=scenes[k]["raw_angle"], is_occ=scenes[k]["is_occ"],
                                          weighting=weighting, init_pose=scenes[k]["init_pose"]) for k in idx])
        self.fn = L.slamhip_matcher_process_raw_scan_batch
        self.fn.argtypes = [C.c_void_p, C.c_int, C.POINTER(pkg.RawMatchJob), _dp, _dp, _ip]
        self.deltas, self.probs = self.blk["deltas"], self.blk["probs"]
        self.args = (m.h, self.blk["n"], self.blk["raw_arr"], self.deltas.ctypes.data_as(_dp), self.probs.ctypes.data_as(_dp),
                     self.blk["kept"].ctypes.data_as(_ip))

    def __call__(self):
        rc = self.fn(*self.args)
        assert rc == 0, L.slamhip_last_error()


class RouteC:
    def __init__(self, m, idx):
        self.m = m
        self.blk = m.make_batch([dict(map_id=0, scan_slot=k, init_pose=scenes[k]["init_pose"]) for k in idx])
        self.deltas, self.probs = self.blk["deltas"], self.blk["probs"]

    def __call__(self):
        rc = L.slamhip_matcher_process_scan_batch(self.m.h, self.blk["n"], self.blk["arr"], self.deltas.ctypes.data_as(_dp),
                                                  self.probs.ctypes.data_as(_dp))
        assert rc == 0, L.slamhip_last_error()


MAKE = {"a": RouteA, "b": RouteB, "c": RouteC}
doc = {"scene": WORKLOADS["hc"][5], "lib": args.lib or "the tree's", "blocks": args.blocks, "calls_per_block": args.calls,
       "routes": {"a": "filter_scan + scan_weights + beam_trig per scan on the host, process_scan_batch with arrays",
                  "b": "process_raw_scan_batch", "c": "process_scan_batch on stored scans (the chains alone)"}, "by_K": []}
for K in [int(v) for v in args.ks.split(",")]:
    groups = [[(g * K + j) % len(scenes) for j in range(K)] for g in range(max(1, len(scenes) // K))]
    ms = {r: pkg.Matcher(ctx, kind, pkg.spe_cfg(), params) for r in routes}
    for m in ms.values():
        assert m.L.slamhip_matcher_set_observer(m.h, None) == 0
    run = {r: [MAKE[r](ms[r], grp) for grp in groups] for r in routes}
    # ---- the same results on every route, bit for bit (and the warm-up: every block of scans twice)
    for _ in range(2):
        for g in range(len(groups)):
            for r in routes:
                run[r][g]()
            first = run[routes[0]][g]
            for r in routes[1:]:
                assert np.array_equal(first.probs.view(np.uint64), run[r][g].probs.view(np.uint64)), (K, r)
                assert np.array_equal(first.deltas.view(np.uint64), run[r][g].deltas.view(np.uint64)), (K, r)
    on_chain = {r: sum(ms[r].batch_stats(j)["on_device_chain"] for j in range(K)) for r in routes}
    if "a" in routes:
        for x in run["a"]:
            x.prep_s = 0.0
    # ---- timed: the routes alternate call by call
    ctx.synchronize()
    per = {r: [] for r in routes}
    for _ in range(args.blocks):
        acc = {r: 0.0 for r in routes}
        for it in range(args.calls):
            g = it % len(groups)
            for r in routes:
                t0 = time.perf_counter()
                run[r][g]()  # (returns after its chains have reported their results)
                acc[r] += time.perf_counter() - t0
        for r in routes:
            per[r].append(1e3 * acc[r] / args.calls)
    prep_ms = 1e3 * sum(x.prep_s for x in run["a"]) / (args.blocks * args.calls) if "a" in routes else None
    # ---- the kernels' own time: a pass of its own with events on every dispatch
    kern = {}
    for r in routes:
        ctx.profile_enable(True)
        ctx.profile_read(reset=True)
        for it in range(args.calls):
            run[r][it % len(groups)]()
        ctx.synchronize()
        ctx.profile_enable(False)
        k_ms, k_launches, _ = ctx.profile_read(reset=True)
        kern[r] = dict(kernel_ms_per_call=k_ms / args.calls, launches_per_call=k_launches / args.calls)
    row = {"K": K, "matches_on_shared_launches": on_chain}
    for r in routes:
        x = np.array(per[r][1:])  # (the first block settles clocks and caches)
        row[r] = dict(ms_per_call_median=float(np.median(x)), ms_per_call_spread=float(x.max() - x.min()),
                      ms_per_call_blocks=[float(v) for v in x], **kern[r])
    if "a" in routes:
        row["a"]["host_prep_ms_per_call"] = prep_ms  # (filter + weights + trig + gathers, over all timed blocks)
    if "b" in routes and "c" in routes:
        asm = row["b"]["kernel_ms_per_call"] - row["c"]["kernel_ms_per_call"]
        row["b_split"] = {"chains_ms": row["c"]["ms_per_call_median"], "assemble_kernel_ms": asm,
                          "host_filter_staging_and_launch_ms": row["b"]["ms_per_call_median"] - row["c"]["ms_per_call_median"] - asm}
    if "a" in routes and "b" in routes:
        row["b_minus_a_ms"] = row["b"]["ms_per_call_median"] - row["a"]["ms_per_call_median"]
    doc["by_K"].append(row)
    print(json.dumps(row))
    for m in ms.values():
        m.close()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(doc, open(args.out, "w"), indent=1)
ctx.close()
