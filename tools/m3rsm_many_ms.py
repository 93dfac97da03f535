#!/usr/bin/env python3
"""Time the many-to-many search of the multi-resolution matcher (BF_M3RSM) against lone matches one after another.

    python tools/m3rsm_many_ms.py [--reps 20] [--size 2000] [--beams 1080] [--out FILE.json]

Scene: the one of tools/m3rsm_ms.py -- a size x size OCC map with walls at 0.05 m (tests/synth.make_scene, the benchmark's
scene), a scan of --beams beams, the `max` OOPE, the default mode (canonical tree sum, device sincos), the default limits
of init_bf_m3rsm (+-1 m, +-1 m, +-5 deg at 0.1 deg, step 0.05: 202 roots per request) and the default speculation.
R = 1, 4, 16 requests on that map: request k is the scan with a little range noise of its own (seeded), kept in scan slot
k, matched from a pose near the scene's (within +-0.25 m, +-2 deg, seeded).  Two routes, alternating in one process:
  many   Matcher.m3rsm_match_many over the R requests: one search, one queue, one best finest probability;
  lone   R times Context.scan_select + Matcher.process_scan, one after another, and the best of the R results -- the only
         route there was before, its code unchanged.
Checked first: both routes name the same request, delta and probability.  Per route and R: wall time (host clock around
the whole route, which waits for its last download) as median / min / max over --reps runs; launches, candidates scored
and committed calls (summed over the R matches for `lone`); kernel time from the library's HIP event pairs in a pass of
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
    m_many = pkg.Matcher(ctx, "BF_M3RSM", cfg, [pyr, *LIMITS])
    m_lone = pkg.Matcher(ctx, "BF_M3RSM", cfg, [pyr, *LIMITS])
    counters = ("launches", "poses_evaluated", "scorer_calls")

    def run_many(n):
        r = m_many.m3rsm_match_many([(pyr, k, poses[k]) for k in range(n)])
        st = m_many.stats()
        return r, {c: st[c] for c in counters}

    def run_lone(n):
        best, total = None, dict.fromkeys(counters, 0)
        for k in range(n):
            ctx.scan_select(k)
            r = m_lone.process_scan(FINE, poses[k])
            st = m_lone.stats()
            for c in counters:
                total[c] += st[c]
            if best is None or r["prob"] > best["prob"]:
                best = dict(request=k, delta=r["delta"], prob=r["prob"])
        return best, total

    routes = {"many": run_many, "lone": run_lone}
    out = dict(scene="OCC %d x %d at 0.05, %d beams, limits +-1 m, +-1 m, +-5 deg at 0.1 deg, step 0.05, speculation 32 x 3"
               % (a.size, a.size, a.beams), requests={})
    for n in REQUESTS:
        info = {}
        got = {name: fn(n) for name, fn in routes.items()}  # (the first run of either route is the warm-up too)
        rm, rl = got["many"][0], got["lone"][0]
        assert rm["request"] == rl["request"] and rm["prob"] == rl["prob"] and np.array_equal(rm["delta"], rl["delta"]), \
            "the routes disagree at R = %d: %r / %r" % (n, rm, rl)
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
                              candidates_scored=st["poses_evaluated"], committed_calls=st["scorer_calls"])
        info["winner"] = dict(request=int(rm["request"]), delta=[float(v) for v in rm["delta"]], prob=float(rm["prob"]))
        info["ratio_lone_over_many"] = info["lone"]["ms"]["median"] / info["many"]["ms"]["median"]
        out["requests"][str(n)] = info
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    m_many.close()
    m_lone.close()
    pyr.close()
    ctx.close()


if __name__ == "__main__":
    main()
