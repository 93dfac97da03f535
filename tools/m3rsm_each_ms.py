#!/usr/bin/env python3
"""Time K independent matches of the multi-resolution matcher (BF_M3RSM) in one lock-step call against lone matches one
after another.

    python tools/m3rsm_each_ms.py [--reps 20] [--size 2000] [--beams 1080] [--out FILE.json]

Scene, limits, speculation and requests: those of tools/m3rsm_many_ms.py -- a size x size OCC map with walls at 0.05 m
(tests/synth.make_scene, the benchmark's scene), a scan of --beams beams, the `max` OOPE, the default mode, the default
limits of init_bf_m3rsm (202 roots per request), speculation 32 x 3; request k is the scan with a little range noise of
its own (seeded), kept in scan slot k, matched from a pose near the scene's.  R = 1, 4, 16.  Three routes, alternating in
one process:
  lone     R times Context.scan_select + Matcher.process_scan, one after another: the only route there was before, its
           code unchanged;
  each_1   Matcher.m3rsm_match_each over the R requests, the host half of a round on the calling thread;
  each_t   the same with the default number of worker threads, min(R, 8).
Checked first: every route gives every request the same delta and probability, bit for bit.  Per route and R: wall time
(host clock around the whole route) as median / min / max over --reps runs; launches, candidates scored, committed calls
and bytes copied back (summed over the R matches for `lone`); kernel time from the library's HIP event pairs in a pass of
its own.  Needs a GPU; prints one JSON object."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import __graft_entry__ as ge  # noqa: E402

FINE, FIRST = 0, 1
LIMITS = (1.0, 1.0, np.deg2rad(5.0), np.deg2rad(0.1), 0.05)
REQUESTS = (1, 4, 16)


def spread(ts):
    ts = np.asarray(ts) * 1e3
    return dict(median=float(np.median(ts)), min=float(ts.min()), max=float(ts.max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--size", type=int, default=2000)
    ap.add_argument("--beams", type=int, default=1080)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import pyoracle as po
    from synth import make_scene
    pkg = ge.load_package()
    ctx = pkg.Context(0)  # raises without a GPU: there is nothing to time on a CPU
    sc = make_scene(cell_model=po.CELL_OCC, size=a.size, scale=0.05, n_beams=a.beams, seed=3)
    ctx.upload_map(FINE, sc["map"])
    scan = sc["scan"]
    cos_a, sin_a = pkg.beam_trig(scan.angle)
    pyr = pkg.Pyramid(ctx, FINE, pkg.OIE_DISCREPANCY, FIRST)
    cfg = pkg.spe_cfg(oope=pkg.OOPE_MAX, oie=pkg.OIE_DISCREPANCY)
    rs = np.random.RandomState(11)
    r_max = max(REQUESTS)
    poses = sc["init_pose"] + np.column_stack([rs.uniform(-0.25, 0.25, r_max), rs.uniform(-0.25, 0.25, r_max),
                                               np.deg2rad(rs.uniform(-2, 2, r_max))])
    poses[0] = sc["init_pose"]
    for k in range(r_max):
        ctx.scan_store(k, scan.range + (0.01 * rs.randn(scan.range.size) if k else 0.0), cos_a, sin_a, scan.weight, scan.factor)
    m_each = pkg.Matcher(ctx, "BF_M3RSM", cfg, [pyr, *LIMITS])
    m_lone = pkg.Matcher(ctx, "BF_M3RSM", cfg, [pyr, *LIMITS])
    counters = ("launches", "poses_evaluated", "scorer_calls")

    def run_each(threads):
        def run(n):
            m_each.set_m3rsm_threads(threads)
            rows = m_each.m3rsm_match_each([(pyr, k, poses[k]) for k in range(n)])
            st = m_each.stats()
            total = {c: st[c] for c in counters}
            total["copied_back"] = m_each.m3rsm_copied_back()
            total["super_steps"] = [m_each.m3rsm_each_stats(k)["super_steps"] for k in range(n)]
            return rows, total
        return run

    def run_lone(n):
        rows, total = [], dict.fromkeys(counters + ("copied_back",), 0)
        total["super_steps"] = []
        for k in range(n):
            ctx.scan_select(k)
            r = m_lone.process_scan(FINE, poses[k])
            st = m_lone.stats()
            for c in counters:
                total[c] += st[c]
            total["copied_back"] += m_lone.m3rsm_copied_back()
            total["super_steps"].append(st["launches"] - 1)
            rows.append(dict(delta=r["delta"], prob=r["prob"]))
        return rows, total

    routes = {"lone": run_lone, "each_1": run_each(1), "each_t": run_each(0)}
    out = dict(scene="OCC %d x %d at 0.05, %d beams, limits +-1 m, +-1 m, +-5 deg at 0.1 deg, step 0.05, speculation 32 x 3"
               % (a.size, a.size, a.beams), requests={})
    for n in REQUESTS:
        info = {}
        got = {name: fn(n) for name, fn in routes.items()}  # (the first run of a route is its warm-up too)
        for name in ("each_1", "each_t"):
            for k, (x, y) in enumerate(zip(got[name][0], got["lone"][0])):
                same = np.array_equal(np.asarray([*x["delta"], x["prob"]]).view(np.int64), np.asarray([*y["delta"], y["prob"]]).view(np.int64))
                assert same, "route %s disagrees with the lone match of request %d at R = %d: %r / %r" % (name, k, n, x, y)
        times = {name: [] for name in routes}
        for _ in range(a.reps):  # the routes alternate
            for name, fn in routes.items():
                t0 = time.perf_counter()
                fn(n)
                times[name].append(time.perf_counter() - t0)
        for name, fn in routes.items():  # kernel time: a pass of its own (the event pairs cost a little)
            ctx.profile_enable(True)
            ctx.profile_read(reset=True)
            for _ in range(3):
                fn(n)
            ctx.synchronize()
            kernel_ms = ctx.profile_read(reset=True)[0] / 3
            ctx.profile_enable(False)
            st = got[name][1]
            info[name] = dict(ms=spread(times[name]), runs=len(times[name]), kernel_ms=kernel_ms, launches=st["launches"],
                              candidates_scored=st["poses_evaluated"], committed_calls=st["scorer_calls"],
                              copied_back_bytes=st["copied_back"])
        info["threads_each_t"] = min(n, 8)
        info["super_steps_per_request"] = got["lone"][1]["super_steps"]
        info["lone_spread_ms"] = info["lone"]["ms"]["max"] - info["lone"]["ms"]["min"]
        info["ratio_lone_over_each_1"] = info["lone"]["ms"]["median"] / info["each_1"]["ms"]["median"]
        info["ratio_lone_over_each_t"] = info["lone"]["ms"]["median"] / info["each_t"]["ms"]["median"]
        out["requests"][str(n)] = info
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    m_each.close()
    m_lone.close()
    pyr.close()
    ctx.close()


if __name__ == "__main__":
    main()
