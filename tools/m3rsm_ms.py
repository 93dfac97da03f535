#!/usr/bin/env python3
"""Time the multi-resolution matcher (BF_M3RSM) on the GPU against the route the pyramid API alone offers.

    python tools/m3rsm_ms.py [--reps 20] [--grid-reps 20] [--size 2000] [--beams 1080] [--out FILE.json]
                             [--pose-trig device|host|raw_exact] [--strict] [--no-grid]

Scene: a size x size OCC map with walls at 0.05 m (tests/synth.make_scene, the benchmark's scene), a scan of --beams
beams, the `max` OOPE, the default mode (canonical tree sum, device sincos) and the documented default limits of
init_bf_m3rsm: +-1 m, +-1 m, +-5 deg at 0.1 deg, translation step 0.05 (202 roots).
  (a) the matcher at its default speculation (width, depth), and the grid width in {8, 32, 128, 256} x depth in {1, 2, 3};
  (b) what the pyramid API alone offers: the same engine core with one slamhip_pyramid_score_matches launch and download
      per popped match (slamhip_matcher_set_m3rsm_speculation(m, 0, 0)).
All routes run in one process and alternate match by match, after a check that they return the same result and the same
trace.  Per route: wall time per match (host clock around process_scan, which waits for its last download) as median /
min / max over the matches; launches, super-steps, branching pops per super-step, candidates scored per committed call;
kernel time per match from the library's HIP event pairs (slamhip_profile_enable), measured in a pass of its own.
`ratio_b_over_a` is median (b) over median (a) at the default.  --pose-trig and --strict (the beam-order sum) select the
scoring mode of every route -- raw_exact: the reference's default trig provider bit for bit, one tabulation launch in
front of every scoring launch --, --no-grid leaves the grid out.  Needs a GPU; prints one JSON object."""
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
GRID = [(w, d) for d in (1, 2, 3) for w in (8, 32, 128, 256)]


def spread(ts):
    ts = np.asarray(ts) * 1e3
    return dict(median=float(np.median(ts)), min=float(ts.min()), max=float(ts.max()))


def branching_pops(trace, step):
    """popped matches that were refined: the distinct calls some later call is a child of, by the refinement rule"""
    from m3rsm_cases import children
    parent_of, pops = {}, set()
    for row in trace:
        k = row[:5].tobytes()
        if k in parent_of:
            pops.add(parent_of[k])
        for kid in children(row[1:5], step):
            parent_of[np.asarray([row[0], *kid]).tobytes()] = k
    return len(pops)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--grid-reps", type=int, default=20)
    ap.add_argument("--size", type=int, default=2000)
    ap.add_argument("--beams", type=int, default=1080)
    ap.add_argument("--out", default=None)
    ap.add_argument("--pose-trig", choices=("device", "host", "raw_exact"), default="device")
    ap.add_argument("--strict", action="store_true")
    ap.add_argument("--no-grid", action="store_true")
    a = ap.parse_args()
    import pyoracle as po
    from synth import make_scene
    pkg = ge.load_package()
    ctx = pkg.Context(0)  # raises without a GPU: there is nothing to time on a CPU
    sc = make_scene(cell_model=po.CELL_OCC, size=a.size, scale=0.05, n_beams=a.beams, seed=3)
    ctx.upload_map(FINE, sc["map"])
    scan = sc["scan"]
    cos_a, sin_a = pkg.beam_trig(scan.angle)
    ctx.scan_upload(scan.range, cos_a, sin_a, scan.weight, scan.factor)
    ctx.scan_set_angles(scan.angle)  # (read by raw_exact only)
    pyr = pkg.Pyramid(ctx, FINE, pkg.OIE_DISCREPANCY, FIRST)
    pose_trig = {"device": pkg.POSE_TRIG_DEVICE, "host": pkg.POSE_TRIG_HOST, "raw_exact": pkg.POSE_TRIG_RAW_EXACT}[a.pose_trig]
    cfg = pkg.spe_cfg(oope=pkg.OOPE_MAX, oie=pkg.OIE_DISCREPANCY, pose_trig=pose_trig,
                      sum_order=pkg.SUM_SEQUENTIAL if a.strict else pkg.SUM_TREE256)
    pose = sc["init_pose"]

    def matcher(width, depth):
        m = pkg.Matcher(ctx, "BF_M3RSM", cfg, [pyr, *LIMITS])
        if (width, depth) != (None, None):
            m.set_m3rsm_speculation(width, depth)
        return m

    routes = {"default": matcher(None, None), "per_pop": matcher(0, 0)}
    for w, d in ([] if a.no_grid else GRID):
        routes["W%d_D%d" % (w, d)] = matcher(w, d)
    # every route returns the same match, call for call
    ref, info = None, {}
    for name, m in routes.items():
        r = m.process_scan(FINE, pose)
        trace = m.m3rsm_trace()
        if ref is None:
            ref = (r, trace)
            n_roots = 2 * len(set(trace[:, 0].tolist()))
            pops = branching_pops(trace, LIMITS[4])
        assert r["prob"] == ref[0]["prob"] and np.array_equal(r["delta"], ref[0]["delta"]), "the routes disagree (%s)" % name
        assert np.array_equal(trace.view(np.int64), ref[1].view(np.int64)), "the routes' traces disagree (%s)" % name
        st = m.stats()
        steps = st["launches"] - 1
        info[name] = dict(launches=st["launches"], super_steps=steps, scorer_calls=st["scorer_calls"],
                          candidates_scored=st["poses_evaluated"], pops_per_super_step=pops / max(steps, 1),
                          candidates_per_call=st["poses_evaluated"] / st["scorer_calls"])
    for m in routes.values():  # warm-up
        m.process_scan(FINE, pose)
    times = {name: [] for name in routes}
    for k in range(max(a.reps, a.grid_reps)):  # the routes alternate
        for name, m in routes.items():
            if k >= (a.reps if name in ("default", "per_pop") else a.grid_reps):
                continue
            t0 = time.perf_counter()
            m.process_scan(FINE, pose)
            times[name].append(time.perf_counter() - t0)
    for name, m in routes.items():  # kernel time: a pass of its own (the event pairs cost a little)
        ctx.profile_enable(True)
        ctx.profile_read(reset=True)
        for _ in range(3):
            m.process_scan(FINE, pose)
        ctx.synchronize()
        info[name]["kernel_ms"] = ctx.profile_read(reset=True)[0] / 3
        ctx.profile_enable(False)
        info[name]["match_ms"] = spread(times[name])
        info[name]["matches"] = len(times[name])
    best = min((n for n in routes if n.startswith("W")), key=lambda n: info[n]["match_ms"]["median"], default=None)
    out = dict(pose_trig=a.pose_trig, sum_order="sequential" if a.strict else "tree256", scene="OCC %d x %d at 0.05, %d beams, limits +-1 m, +-1 m, +-5 deg at 0.1 deg, step 0.05" % (a.size, a.size, a.beams),
               roots=int(n_roots), branching_pops=int(pops), result=dict(delta=ref[0]["delta"].tolist(), prob=ref[0]["prob"]),
               routes=info, fastest_grid_point=best,
               ratio_b_over_a=info["per_pop"]["match_ms"]["median"] / info["default"]["match_ms"]["median"])
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    for m in routes.values():
        m.close()
    pyr.close()
    ctx.close()


if __name__ == "__main__":
    main()
