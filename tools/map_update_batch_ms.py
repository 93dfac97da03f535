"""K scans into K resident maps, three routes timed side by side (K = 1, 4, 8, 16, 64 maps of 1000 x 1000 cells at 0.1 m;
the tinySLAM preset -- MeanProbabilityCell, blur 0.5 -- and the vinySLAM preset -- TbmBaseCell, blur 0.3; 1080-beam raw
scans of synth.make_scene, robot k of call i at pose and scan (i + k) mod 16 of bench_legs.common.rotating_scenes):

  batch     slamhip_map_append_scan_batch on an argument block made once
  deferred  the fastest lone route: K slamhip_map_append_scan_q calls queued (slamhip_map_set_deferred) and closed by one
            slamhip_map_drain
  awaited   K awaited slamhip_map_append_scan_q calls, for the record

The routes alternate call by call inside every block, each on its own set of K maps; per route and K the median over the
blocks of the mean ms per call and the blocks' max - min (the first block settles clocks and caches and is dropped).
At the end of a K the maps of all routes are compared bit for bit.  --lib PATH: another build of libslamhip.so (the
parent commit's, which has no batch: --routes deferred,awaited).  --with-match: one fleet step at K = 16 on the
tinySLAM preset, slamhip_matcher_process_raw_scan_batch followed by the batch update, against the same batched match
followed by K deferred lone updates and the drain.  Writes one JSON document to --out.  Run on the GPU box."""
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
ap.add_argument("--ks", default="1,4,8,16,64")
ap.add_argument("--blocks", type=int, default=21, help="blocks per K (the first one is dropped)")
ap.add_argument("--calls", type=int, default=16, help="calls per route and block")
ap.add_argument("--routes", default="batch,deferred,awaited")
ap.add_argument("--presets", default="tiny,viny")
ap.add_argument("--with-match", action="store_true")
ap.add_argument("--lib", default=None)
ap.add_argument("--out", default=None)
args = ap.parse_args()
routes = args.routes.split(",")

pkg = ge.load_package()
if args.lib:
    pkg.LIB_PATH = os.path.abspath(args.lib)
L = pkg.load()
_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
SIZE, SCALE, BEAMS, N_SCENES = 1000, 0.1, 1080, 16
PRESETS = {"tiny": dict(cell=0, rule=pkg.RULE_MEAN, blur=0.5, unknown=[0.5], stride=1, aux=1),
           "viny": dict(cell=1, rule=pkg.RULE_TBM, blur=0.3, unknown=[1.0, 0.0, 0.0, 0.0], stride=4, aux=0)}


class JobStruct(C.Structure):  # slamhip_map_update_job
    _fields_ = [("map_id", C.c_int), ("pose", C.c_double * 3), ("scan_quality", C.c_double), ("n", C.c_int),
                ("range", _dp), ("cos_a", _dp), ("sin_a", _dp), ("angle", _dp), ("is_occ", _ip), ("quality", _dp),
                ("cfg", C.c_void_p)]


def scans_of(sc):
    out = []
    for s in rotating_scenes(sc, BEAMS, "even", N_SCENES):
        c_, s_ = pkg.beam_trig(s["raw_angle"])
        out.append(dict(range=np.ascontiguousarray(s["raw_range"], dtype=np.float64), cos=c_, sin=s_,
                        occ=np.ascontiguousarray(s["is_occ"], dtype=np.int32), pose=np.ascontiguousarray(s["true_pose"], dtype=np.float64),
                        raw=s))
    return out


class Batch:
    def __init__(self, ctx, p, scans, K, first_map):
        self.ctx, self.K = ctx, K
        self.cfg = pkg.ScanAdderCfg(p["rule"], 1.0, 0.95, 1.0, 0.01, 1.0, p["blur"], float("inf"), 0, 0.0)
        self.blocks = []
        for g in range(N_SCENES):
            arr = (JobStruct * K)()
            for k in range(K):
                s = scans[(g + k) % N_SCENES]
                a = arr[k]
                a.map_id, a.scan_quality, a.n = first_map + k, 0.9, s["range"].size
                a.pose[:] = list(s["pose"])
                a.range, a.cos_a, a.sin_a = (s[x].ctypes.data_as(_dp) for x in ("range", "cos", "sin"))
                a.is_occ = s["occ"].ctypes.data_as(_ip)
            self.blocks.append(arr)
        self.nu = np.zeros(K, np.int64)
        self.fn = L.slamhip_map_append_scan_batch
        self.fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]

    def __call__(self, g):
        rc = self.fn(self.ctx.h, C.byref(self.cfg), self.K, C.byref(self.blocks[g]), self.nu.ctypes.data, None)
        assert rc == 0, L.slamhip_last_error()
        return int(self.nu.sum())


class Lone:
    def __init__(self, ctx, p, scans, K, first_map, deferred):
        self.ctx, self.K, self.deferred = ctx, K, deferred
        self.append = [[ctx.make_map_append_scan(first_map + k, p["rule"], s["range"], s["cos"], s["sin"], s["occ"], quality=0.9,
                                                 blur=p["blur"]) for s in scans] for k in range(K)]
        self.poses = [s["pose"] for s in scans]

    def __call__(self, g):
        self.ctx.map_set_deferred(self.deferred)
        total = 0
        for k in range(self.K):
            j = (g + k) % N_SCENES
            total += self.append[k][j](self.poses[j])
        if self.deferred:
            total = self.ctx.map_drain()
        return total


def measure(ctx, run, K, calls, blocks):
    names = list(run)
    for g in range(2):  # warm-up, and the same update counts on every route
        got = {r: run[r](g) for r in names}
        assert len(set(got.values())) == 1 and got[names[0]] > 0, got
    ctx.synchronize()
    per = {r: [] for r in names}
    for _ in range(blocks):
        acc = {r: 0.0 for r in names}
        for it in range(calls):
            for r in names:
                t0 = time.perf_counter()
                run[r](it % N_SCENES)  # (returns after the maps are updated: awaited, or drained)
                acc[r] += time.perf_counter() - t0
        for r in names:
            per[r].append(1e3 * acc[r] / calls)
    row = {"K": K}
    for r in names:
        x = np.array(per[r][1:])
        row[r] = dict(ms_per_call_median=float(np.median(x)), ms_per_call_spread=float(x.max() - x.min()),
                      ms_per_call_blocks=[float(v) for v in x])
    return row


doc = {"lib": args.lib or "the tree's", "blocks": args.blocks - 1, "calls_per_block": args.calls,
       "maps": "%d x %d cells at %g m, %d-beam raw scans, %d rotating poses" % (SIZE, SIZE, SCALE, BEAMS, N_SCENES),
       "routes": {"batch": "slamhip_map_append_scan_batch", "deferred": "K queued slamhip_map_append_scan_q + slamhip_map_drain",
                  "awaited": "K awaited slamhip_map_append_scan_q"}, "presets": {}}
for preset in args.presets.split(","):
    p = PRESETS[preset]
    sc = make_scene(cell_model=p["cell"], size=SIZE, scale=SCALE, n_beams=BEAMS, seed=100)
    scans = scans_of(sc)
    rows = []
    for K in [int(v) for v in args.ks.split(",")]:
        ctx = pkg.Context(0)
        first = {r: 100 * i for i, r in enumerate(routes)}
        for r in routes:
            for k in range(K):
                ctx.map_bind(first[r] + k, p["cell"], SIZE, SIZE, (SIZE // 2, SIZE // 2), SCALE, p["unknown"])
        run = {}
        for r in routes:
            run[r] = Batch(ctx, p, scans, K, first[r]) if r == "batch" else Lone(ctx, p, scans, K, first[r], r == "deferred")
        row = measure(ctx, run, K, args.calls, args.blocks)
        ctx.map_set_deferred(False)
        if "batch" in routes:
            st = ctx.map_update_batch_stats()
            row["batch"]["jobs_in_shared_launches"], row["batch"]["rounds"] = st["jobs_shared"], st["rounds"]
        # every route saw the same scans in the same order: the same maps, bit for bit
        for k in range(K):
            ref = ctx.map_download_window(first[routes[0]] + k, 0, 0, SIZE, SIZE, p["stride"])
            for r in routes[1:]:
                assert np.array_equal(ref.view(np.uint64), ctx.map_download_window(first[r] + k, 0, 0, SIZE, SIZE, p["stride"]).view(np.uint64)), (K, k, r)
                if p["aux"]:
                    assert np.array_equal(ctx.map_download_aux(first[routes[0]] + k, 0, 0, SIZE, SIZE, p["aux"]),
                                          ctx.map_download_aux(first[r] + k, 0, 0, SIZE, SIZE, p["aux"])), (K, k, r)
        row["maps_equal_on_all_routes"] = True
        rows.append(row)
        print(preset, json.dumps({k: (v if not isinstance(v, dict) else {a: b for a, b in v.items() if a != "ms_per_call_blocks"})
                                  for k, v in row.items()}), flush=True)
        ctx.close()
    doc["presets"][preset] = rows

if args.with_match:
    # one fleet step, K = 16, tinySLAM preset: the batched raw-scan match, then the updates at the matched poses' place
    # (the update's poses are the scans' own: both routes update the same cells whatever the match returns)
    K, p = 16, PRESETS["tiny"]
    cell, weighting, kind, params = WORKLOADS["hc"][:4]
    sc = make_scene(cell_model=cell, size=SIZE, scale=SCALE, n_beams=BEAMS, seed=100, weighting=weighting)
    scans = scans_of(sc)
    ctx = pkg.Context(0)
    first = {"batch": 0, "deferred": 100}
    for r in first:
        for k in range(K):
            ctx.upload_map(first[r] + k, sc["map"])
    upd = {"batch": Batch(ctx, p, scans, K, first["batch"]), "deferred": Lone(ctx, p, scans, K, first["deferred"], True)}
    m = {r: pkg.Matcher(ctx, kind, pkg.spe_cfg(), params) for r in first}
    fn = L.slamhip_matcher_process_raw_scan_batch
    fn.argtypes = [C.c_void_p, C.c_int, C.POINTER(pkg.RawMatchJob), _dp, _dp, _ip]
    blk = {r: [m[r].make_raw_batch([dict(map_id=first[r] + k, range=scans[(g + k) % N_SCENES]["raw"]["raw_range"],
                                         angle=scans[(g + k) % N_SCENES]["raw"]["raw_angle"], is_occ=scans[(g + k) % N_SCENES]["raw"]["is_occ"],
                                         weighting=weighting, init_pose=scans[(g + k) % N_SCENES]["raw"]["init_pose"]) for k in range(K)])
               for g in range(N_SCENES)] for r in first}

    def step(r):
        def go(g):
            b = blk[r][g]
            rc = fn(m[r].h, b["n"], b["raw_arr"], b["deltas"].ctypes.data_as(_dp), b["probs"].ctypes.data_as(_dp),
                    b["kept"].ctypes.data_as(_ip))
            assert rc == 0, L.slamhip_last_error()
            return upd[r](g)
        return go
    row = measure(ctx, {"match+batch": step("batch"), "match+deferred": step("deferred")}, K, args.calls, args.blocks)
    ctx.map_set_deferred(False)
    doc["fleet_step_K16_tiny"] = row
    print("fleet", json.dumps({k: (v if not isinstance(v, dict) else {a: b for a, b in v.items() if a != "ms_per_call_blocks"})
                               for k, v in row.items()}), flush=True)
    for x in m.values():
        x.close()
    ctx.close()

if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(doc, open(args.out, "w"), indent=1)
