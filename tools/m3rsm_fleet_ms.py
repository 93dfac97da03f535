#!/usr/bin/env python3
"""Time the two fleet calls of the multi-resolution matcher (BF_M3RSM) against the routes they replace.

    python tools/m3rsm_fleet_ms.py [--reps 20] [--size 2000] [--beams 1080] [--parts a,b] [--lib PATH] [--out FILE.json]

(a) refresh: K pyramids over size x size OCC maps at 0.05 m (tests/synth.make_scene, the benchmark's scene), the window
    the adapter's reach rule gives a 10 m scan around the scene's pose (host/slamhip_m3rsm_map.h: reach + two cells), K = 1,
    4, 16.  Two sets of twin maps; before every run the same random cells of the window are rewritten on both, then
      batch   one Context.pyramid_refresh_batch over the K pyramids of set A,
      lone    K Pyramid.refresh calls one after another on set B,
    each followed by Context.synchronize() inside the timed span.  After EVERY run the refreshed window of every level of
    every pyramid is downloaded from both sets and compared bit for bit.
(b) match: K raw scans (the scene's scan with range noise of its own per request, every beam's is_occ set, every third
    request with a fifth of its beams dropped by is_occ) from poses near the scene's, K = 4, 16.
      raw     one Matcher.m3rsm_match_each_raw,
      host    per request filter_scan + scan_weights + beam_trig + Context.scan_store, then one Matcher.m3rsm_match_each.
    Every request's delta and probability are compared bit for bit on EVERY call.
Per route and K: wall time as median / min / max over --reps runs, the routes alternating (the order swaps every run);
launches of the refresh routes; kernel time of the refresh routes from the library's HIP event pairs in a pass of its
own.  "claim" is false where one route's median lies inside the other's spread.  --parts: which of (a), (b) to run.
--lib PATH: another build of libslamhip.so (the parent commit's).  Needs a GPU; prints one JSON object."""
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

LIMITS = (1.0, 1.0, np.deg2rad(5.0), np.deg2rad(0.1), 0.05)
REFRESH_K = (1, 4, 16)
MATCH_K = (4, 16)
ID_STRIDE = 20  # map ids per pyramid: the fine map and up to 19 levels


def spread(ts):
    ts = np.asarray(ts) * 1e3
    return dict(median=float(np.median(ts)), min=float(ts.min()), max=float(ts.max()))


def verdict(a, b):
    """a claim only where neither median lies inside the other route's spread"""
    inside = b["min"] <= a["median"] <= b["max"] or a["min"] <= b["median"] <= a["max"]
    return dict(ratio_second_over_first=b["median"] / a["median"], claim=not inside)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def level_windows(pyr, origin, win):
    """per level (map_id, x0, y0, w, h): the cells whose blocks meet the fine window"""
    x0, y0, w, h = win
    out = []
    info = pyr.info()
    for lv, g in enumerate(info, 1):
        if lv == len(info):
            out.append((g["map_id"], 0, 0, 1, 1))
            continue
        cx0, cx1 = ((x0 - origin[0]) >> lv) + g["origin"][0], ((x0 + w - 1 - origin[0]) >> lv) + g["origin"][0]
        cy0, cy1 = ((y0 - origin[1]) >> lv) + g["origin"][1], ((y0 + h - 1 - origin[1]) >> lv) + g["origin"][1]
        out.append((g["map_id"], cx0, cy0, cx1 - cx0 + 1, cy1 - cy0 + 1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--size", type=int, default=2000)
    ap.add_argument("--beams", type=int, default=1080)
    ap.add_argument("--out", default=None)
    ap.add_argument("--parts", default="a,b")
    ap.add_argument("--lib", default=None)
    a = ap.parse_args()
    parts = a.parts.split(",")
    import pyoracle as po
    from synth import make_scene
    pkg = ge.load_package()
    if a.lib:
        pkg.LIB_PATH = os.path.abspath(a.lib)
    ctx = pkg.Context(0)  # raises without a GPU: there is nothing to time on a CPU
    sc = make_scene(cell_model=po.CELL_OCC, size=a.size, scale=0.05, n_beams=a.beams, seed=3)
    m = sc["map"]
    out = dict(scene="OCC %d x %d at 0.05, %d beams" % (a.size, a.size, a.beams), lib=a.lib or "the tree's", refresh={}, match={})

    # ---- (a) refresh -------------------------------------------------------------------------------------------------
    if "a" in parts:
        k_max = max(REFRESH_K)
        sets = []
        for s in range(2):
            pyrs = []
            for k in range(k_max):
                fine = (s * k_max + k) * ID_STRIDE
                ctx.upload_map(fine, m)
                pyrs.append(pkg.Pyramid(ctx, fine, pkg.OIE_DISCREPANCY, fine + 1))
            sets.append(pyrs)
        reach = 10.0 + 2 * m.scale
        px, py = sc["init_pose"][0], sc["init_pose"][1]
        x0 = max(0, int(np.floor((px - reach) / m.scale)) + m.origin[0])
        y0 = max(0, int(np.floor((py - reach) / m.scale)) + m.origin[1])
        x1 = min(m.width - 1, int(np.floor((px + reach) / m.scale)) + m.origin[0])
        y1 = min(m.height - 1, int(np.floor((py + reach) / m.scale)) + m.origin[1])
        win = (x0, y0, x1 - x0 + 1, y1 - y0 + 1)
        windows = [[level_windows(p, m.origin, win) for p in pyrs] for pyrs in sets]
        out["refresh_window"] = dict(x0=win[0], y0=win[1], w=win[2], h=win[3], levels=len(sets[0][0].info()))
        rs = np.random.RandomState(5)

        def dirty(n):
            for k in range(n):
                flat = rs.choice(win[2] * win[3], 400, replace=False)  # (distinct cells: the dirty log's order between equal cells is not fixed)
                cells = np.column_stack([win[0] + flat % win[2], win[1] + flat // win[2]])
                vals = rs.rand(400, 1)
                for s in range(2):
                    ctx.map_apply_dirty((s * k_max + k) * ID_STRIDE, cells, vals)
            ctx.synchronize()

        def run_batch(n):
            ctx.pyramid_refresh_batch([(sets[0][k], *win) for k in range(n)])
            ctx.synchronize()

        def run_lone(n):
            for k in range(n):
                sets[1][k].refresh(*win)
            ctx.synchronize()

        def compare(n):
            for k in range(n):
                for (ia, *wa), (ib, *wb) in zip(windows[0][k], windows[1][k]):
                    assert wa == wb
                    ga, gb = ctx.map_download_window(ia, *wa, 1), ctx.map_download_window(ib, *wb, 1)
                    assert np.array_equal(bits(ga), bits(gb)), "pyramid %d: the batch's level on map id %d differs from the lone call's" % (k, ia)

        routes = (("batch", run_batch), ("lone", run_lone))
        for n in REFRESH_K:
            times = {name: [] for name, _ in routes}
            for rep in range(a.reps + 1):  # (run 0 is the warm-up)
                dirty(n)
                for name, fn in (routes if rep % 2 == 0 else routes[::-1]):
                    t0 = time.perf_counter()
                    fn(n)
                    if rep:
                        times[name].append(time.perf_counter() - t0)
                compare(n)
            info = {name: dict(ms=spread(ts), runs=len(ts)) for name, ts in times.items()}
            info["batch"].update(ctx.pyramid_refresh_batch_stats())
            info["lone"]["launches"] = n * len(sets[1][0].info())
            for name, fn in routes:  # kernel time: a pass of its own (the event pairs cost a little)
                ctx.profile_enable(True)
                ctx.profile_read(reset=True)
                for _ in range(3):
                    fn(n)
                info[name]["kernel_ms"] = ctx.profile_read(reset=True)[0] / 3
                ctx.profile_enable(False)
            info.update(verdict(info["batch"]["ms"], info["lone"]["ms"]))
            out["refresh"][str(n)] = info
        for pyrs in sets:
            for p in pyrs:
                p.close()
        for i in range(2 * k_max):
            ctx.map_release(i * ID_STRIDE)

    # ---- (b) match ---------------------------------------------------------------------------------------------------
    if "b" in parts:
        ctx.upload_map(0, m)
        pyr = pkg.Pyramid(ctx, 0, pkg.OIE_DISCREPANCY, 1)
        cfg = pkg.spe_cfg(oope=pkg.OOPE_MAX, oie=pkg.OIE_DISCREPANCY)
        scan = sc["scan"]
        k_max = max(MATCH_K)
        rs = np.random.RandomState(11)
        poses = sc["init_pose"] + np.column_stack([rs.uniform(-0.25, 0.25, k_max), rs.uniform(-0.25, 0.25, k_max),
                                                   np.deg2rad(rs.uniform(-2, 2, k_max))])
        geom = dict(width=m.width, height=m.height, origin=m.origin, scale=m.scale, bounded=False)
        reqs = []
        for k in range(k_max):
            occ = np.ones(scan.range.size, np.int32)
            if k % 3 == 2:
                occ[::5] = 0
            reqs.append(dict(pyramid=pyr, range=scan.range + (0.01 * rs.randn(scan.range.size) if k else 0.0), angle=scan.angle,
                             is_occ=occ, factor=scan.factor, init_pose=poses[k], weighting="even"))
        m_raw = pkg.Matcher(ctx, "BF_M3RSM", cfg, [pyr, *LIMITS])
        m_host = pkg.Matcher(ctx, "BF_M3RSM", cfg, [pyr, *LIMITS])

        def run_raw(n):
            return m_raw.m3rsm_match_each_raw(reqs[:n])

        def run_host(n):
            table = []
            for k, r in enumerate(reqs[:n]):
                kept = pkg.filter_scan(r["range"], r["angle"], r["is_occ"], r["init_pose"], geom)
                rng, ang = r["range"][kept], r["angle"][kept]
                cos_a, sin_a = pkg.beam_trig(ang)
                ctx.scan_store(k, rng, cos_a, sin_a, pkg.scan_weights("even", rng, ang), r["factor"][kept])
                table.append((pyr, k, r["init_pose"]))
            return m_host.m3rsm_match_each(table)

        routes = (("raw", run_raw), ("host", run_host))
        for n in MATCH_K:
            times = {name: [] for name, _ in routes}
            for rep in range(a.reps + 1):
                got = {}
                for name, fn in (routes if rep % 2 == 0 else routes[::-1]):
                    t0 = time.perf_counter()
                    got[name] = fn(n)
                    if rep:
                        times[name].append(time.perf_counter() - t0)
                for k, (x, y) in enumerate(zip(got["raw"], got["host"])):
                    assert np.array_equal(bits([*x["delta"], x["prob"]]), bits([*y["delta"], y["prob"]])), \
                        "request %d at K = %d: the raw route %r, the host route %r" % (k, n, x, y)
            info = {name: dict(ms=spread(ts), runs=len(ts)) for name, ts in times.items()}
            info["raw"]["launches"] = m_raw.stats()["launches"]
            info["host"]["launches"] = m_host.stats()["launches"]
            info["kept"] = [g["kept"] for g in got["raw"]]
            info.update(verdict(info["raw"]["ms"], info["host"]["ms"]))
            out["match"][str(n)] = info
        m_raw.close()
        m_host.close()
        pyr.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
