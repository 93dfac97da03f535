"""The two ends of the headline's match (one slamhip_matcher_process_raw_scan per step: cfg2 hill climbing as ONE
co-resident launch, 16 rotating scenes): what the host does in front of the launch and how the result gets back.

  host ends     libslamhip_testing.so reads the host's clock at entry, behind filter + staging, at the launch call, at
                its return and when the result is seen (csrc/matchers.cpp, SLAMHIP_MATCH_END), reported through
                stats(): build_us, stage_us, replay_us.  On the bench's scans (unbounded map) and on the same scans
                with the end-point test of a bounded map (raw beam trig: a libm sincos per beam in front of the test).
  device ends   the bookkeeping workgroup's wall clock (100 MHz) where it sees the chain is over and after the
                completion word's store has been waited for (spare stamps 14 and 22 of slamhip_matcher_debug_stamps).
  per match     the shipped library, time per match over the rotating scenes.

Run on the GPU box."""
import ctypes as C
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

pkg = ge.load_package()
cell, weighting, kind, params = WORKLOADS["hc"][:4]
sc = make_scene(cell_model=cell, size=2000, scale=0.05, n_beams=1080, seed=100, weighting=weighting)
scenes = rotating_scenes(sc, 1080, weighting)


def summary(x):
    x = np.asarray(x, dtype=np.float64)
    return "median %.2f (p10 %.2f, p90 %.2f)" % (np.median(x), np.percentile(x, 10), np.percentile(x, 90))


def matcher(ctx, bounded):
    m = pkg.Matcher(ctx, kind, pkg.spe_cfg(), params)
    match = [m.make_raw_process_scan(0, s["raw_range"], s["raw_angle"], is_occ=s["is_occ"], weighting=weighting, bounded=bounded)
             for s in scenes]
    return m, match


# ---- host ends and device ends: the testing library
ctx = pkg.Context(0, testing=True)
ctx.upload_map(0, sc["map"])
L = pkg.load(testing=True)
L.slamhip_matcher_debug_stamps.argtypes = [C.c_void_p, C.POINTER(C.c_longlong)]
for bounded in (False, True):
    m, match = matcher(ctx, bounded)
    rows = []
    for i in range(32 + 480):
        kept, _ = match[i % 16](scenes[i % 16]["init_pose"])
        if i >= 32:
            st = m.stats()
            rows.append((st["build_us"], st["stage_us"], st["replay_us"], st["score_us"]))
    rows = np.array(rows)
    print("host ends, %s map, %d beams kept of 1080: entry -> filter + staging done %s us; -> launch "
          "call %s us; launch returned -> result seen %s us; arguments -> result reported %s us; resident %r" %
          ("bounded" if bounded else "unbounded", kept, summary(rows[:, 0]), summary(rows[:, 1]), summary(rows[:, 2]),
           summary(rows[:, 3]), m.resident_stats()))
    if not bounded:
        L.slamhip_matcher_debug_stamps(m.h, None)
        over = []
        for i in range(16 + 200):
            match[i % 16](scenes[i % 16]["init_pose"])
            if i >= 16:
                buf = (C.c_longlong * 512)()
                L.slamhip_matcher_debug_stamps(m.h, buf)
                over.append((buf[22] - buf[14]) / 100.0)
        print("device ends: chain seen to be over -> completion word's store waited for %s us, min %.2f, max %.2f "
              "(10 ns clock)" % (summary(over), min(over), max(over)))
    m.close()
ctx.close()

# ---- per match: the shipped library
ctx = pkg.Context(0)
ctx.upload_map(0, sc["map"])
m, match = matcher(ctx, False)
blocks = []
for block in range(12):
    ts = []
    for i in range(16 + 320):
        t0 = time.perf_counter()
        match[i % 16](scenes[i % 16]["init_pose"])
        if i >= 16:
            ts.append(1e6 * (time.perf_counter() - t0))
    blocks.append(np.mean(ts))
x = np.array(blocks[2:])
print("per match: us, mean of 320, blocks %s; median of blocks %.2f, max - min %.2f" %
      (" ".join("%.2f" % v for v in x), np.median(x), x.max() - x.min()))
