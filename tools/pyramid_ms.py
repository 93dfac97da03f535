#!/usr/bin/env python3
"""Time the map pyramid and the bound scorer on the GPU (csrc/map_pyramid.hip) against the routes they replace.

    python tools/pyramid_ms.py [--reps 20] [--out FILE.json]

For a 2000 x 2000 OCC map and a 2000 x 2000 TBM map (random payloads, a third of the cells unknown):
  build_ms       Pyramid.rebuild + the wait: every level from the fine map, on the device (host clock around the call and
                 a stream synchronise); median and min / max over --reps calls after two warm-up calls
  refresh_ms     Pyramid.refresh of a 64 x 64 window in the middle of the map + the wait
  host_route_ms  what the parent commit offers for the same levels: Context.map_download_window of the fine map +
                 pyramid_build_host + Context.map_upload_window of every level into maps bound beforehand; split into
                 its three parts
  kernel_ms      the levels' kernels alone, first to last: the HIP event pair the library records around them while
                 profiling is on (slamhip_profile_enable), mean over the calls
  traffic        the ALGORITHMIC bytes of a build -- the fine map read once, every level written once: cells x bytes per
                 cell x (1 + sum over the levels of 4^-k) -- over kernel_ms, and that rate's share of the 8 TB/s HBM peak
                 and of the 6.3 TB/s a copy kernel reaches (the kernels also write and read back each level's 8-byte
                 winner coordinates and read every level below the last once: not counted)
For the 206 root candidates of the documented limits (config/common/bf_m3rsm.properties) x 1080 beams on the OCC map:
  score_ms       Pyramid.score_matches, one launch; against one Context.score_poses call per distinct (level, rectangle)
                 -- two calls of 103 poses here --, alternating; kernel_ms as above
The levels and the bounds of the two routes are compared bit for bit before anything is timed.  Needs a GPU; prints one
JSON object."""
import argparse
import json
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

HBM_PEAK_GBS, HBM_COPY_GBS = 8000.0, 6300.0
FINE, FIRST, SPARE = 0, 1, 100  # map ids: the fine map, the pyramid's levels, the host route's levels


def spread(ts):
    ts = np.asarray(ts) * 1e3
    return dict(median=float(np.median(ts)), min=float(ts.min()), max=float(ts.max()))


def make_map(pkg, model, size, rs):
    stride = pkg.STRIDE[model]
    if stride == 1:
        payload = rs.randint(1, 1024, (size, size, 1)) / 1024.0
        unknown = np.array([0.5])
        payload[payload == 0.5] = 0.25
    else:
        payload = rs.dirichlet([1, 1, 1, 1], size * size).reshape(size, size, 4)
        unknown = np.array([1.0, 0.0, 0.0, 0.0])
    payload[rs.rand(size, size) < 1.0 / 3.0] = unknown
    return types.SimpleNamespace(cell_model=model, payload=payload, origin=(size // 2, size // 2), scale=0.05, unknown=unknown,
                                 width=size, height=size)


def timed(fn, ctx):
    t0 = time.perf_counter()
    fn()
    ctx.synchronize()
    return time.perf_counter() - t0


def kernel_ms(ctx, fn, reps):
    ctx.profile_enable(True)
    ctx.profile_read(reset=True)
    for _ in range(reps):
        fn()
    ctx.synchronize()
    ms = ctx.profile_read(reset=True)[0] / reps
    ctx.profile_enable(False)
    return ms


def build_case(pkg, ctx, name, model, size, reps):
    m = make_map(pkg, model, size, np.random.RandomState(11))
    stride = pkg.STRIDE[model]
    ctx.upload_map(FINE, m)
    pyr = pkg.Pyramid(ctx, FINE, pkg.OIE_DISCREPANCY, FIRST)
    info = pyr.info()
    host = pkg.pyramid_build_host(m, pkg.OIE_DISCREPANCY)
    for lv, h in zip(info, host):
        got = ctx.map_download_window(lv["map_id"], 0, 0, lv["width"], lv["height"], stride)
        assert np.array_equal(got.view(np.int64), h["payload"].view(np.int64)), "the two routes disagree"
        ctx.map_bind(SPARE + lv["map_id"], model, lv["width"], lv["height"], lv["origin"], lv["scale"], m.unknown)
    win = (size // 2 - 32, size // 2 - 32, 64, 64)
    for _ in range(2):
        pyr.rebuild()
        pyr.refresh(*win)
    ctx.synchronize()
    t_build, t_refresh, t_down, t_host, t_up = [], [], [], [], []
    for _ in range(reps):  # the routes alternate
        t_build.append(timed(pyr.rebuild, ctx))
        t_refresh.append(timed(lambda: pyr.refresh(*win), ctx))
        t0 = time.perf_counter()
        pay = ctx.map_download_window(FINE, 0, 0, size, size, stride)
        t1 = time.perf_counter()
        m.payload = pay
        levels = pkg.pyramid_build_host(m, pkg.OIE_DISCREPANCY)
        t2 = time.perf_counter()
        for lv, h in zip(info, levels):
            ctx.map_upload_window(SPARE + lv["map_id"], 0, 0, h["payload"])
        t3 = time.perf_counter()
        t_down.append(t1 - t0)
        t_host.append(t2 - t1)
        t_up.append(t3 - t2)
    k_build = kernel_ms(ctx, pyr.rebuild, reps)
    k_refresh = kernel_ms(ctx, lambda: pyr.refresh(*win), reps)
    cell_bytes = 8 * stride
    traffic = size * size * cell_bytes + sum(lv["width"] * lv["height"] * cell_bytes for lv in info)
    gbs = traffic / (k_build * 1e-3) / 1e9
    total = np.asarray(t_down) + np.asarray(t_host) + np.asarray(t_up)
    res = dict(map="%s %d x %d" % (name, size, size), levels=len(info), build_ms=spread(t_build), refresh_ms=spread(t_refresh),
               host_route_ms=spread(total), download_ms=spread(t_down), host_build_ms=spread(t_host), upload_ms=spread(t_up),
               build_kernel_ms=k_build, refresh_kernel_ms=k_refresh, algorithmic_bytes=traffic, build_gbs=gbs,
               share_of_hbm_peak=gbs / HBM_PEAK_GBS, share_of_copy_rate=gbs / HBM_COPY_GBS,
               speedup_median=float(np.median(total) / np.median(t_build)))
    for lv in info:
        ctx.map_release(SPARE + lv["map_id"])
    return res, pyr, m


def score_case(pkg, ctx, pyr, reps, beams=1080):
    rs = np.random.RandomState(3)
    ang = np.linspace(-np.pi, np.pi, beams, endpoint=False)
    cos_a, sin_a = pkg.beam_trig(ang)
    ctx.scan_upload(2.0 + 40.0 * rs.rand(beams), cos_a, sin_a, np.full(beams, 1.0 / beams))
    rot, rect = pkg.m3rsm_root_candidates((1.0, 1.0, 2 * 0.087), 0.0017)
    base = np.array([0.31, -0.17, 0.2])
    cfg = pkg.spe_cfg(oope=pkg.OOPE_MAX, oie=pkg.OIE_DISCREPANCY)
    ids = pyr.level_map_ids()
    got, level = pyr.score_matches(cfg, base, rot, rect)
    cx, cy = rect[:, 2] + (rect[:, 3] - rect[:, 2]) / 2, rect[:, 0] + (rect[:, 1] - rect[:, 0]) / 2
    poses = np.stack([base[0] + cx, base[1] + cy, rot + base[2]], axis=1)
    groups = {}
    for i in range(rot.size):
        groups.setdefault((int(level[i]), tuple(rect[i])), []).append(i)
    calls = [(ids[lv], pkg.spe_cfg(oope=pkg.OOPE_MAX, oie=pkg.OIE_DISCREPANCY, area=r), np.asarray(idx)) for (lv, r), idx in groups.items()]

    def per_group():
        out = np.zeros(rot.size)
        for map_id, c, idx in calls:
            out[idx] = ctx.score_poses(map_id, c, poses[idx])
        return out

    assert np.array_equal(per_group().view(np.int64), got.view(np.int64)), "the two routes disagree"
    for _ in range(2):
        pyr.score_matches(cfg, base, rot, rect)
        per_group()
    t_one, t_groups = [], []
    for _ in range(reps):
        t_one.append(timed(lambda: pyr.score_matches(cfg, base, rot, rect), ctx))
        t_groups.append(timed(per_group, ctx))
    k_one = kernel_ms(ctx, lambda: pyr.score_matches(cfg, base, rot, rect), reps)
    k_groups = kernel_ms(ctx, per_group, reps)
    return dict(candidates=int(rot.size), beams=beams, distinct_level_rect=len(calls), levels_used=sorted(set(level.tolist())),
                score_ms=spread(t_one), per_group_ms=spread(t_groups), score_kernel_ms=k_one, per_group_kernel_ms=k_groups,
                speedup_median=float(np.median(t_groups) / np.median(t_one)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--size", type=int, default=2000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = ge.load_package()
    ctx = pkg.Context(0)  # raises without a GPU: there is nothing to time on a CPU
    occ, pyr, _ = build_case(pkg, ctx, "OCC", pkg.CELL_OCC, a.size, a.reps)
    score = score_case(pkg, ctx, pyr, a.reps)
    pyr.close()
    ctx.map_release(FINE)
    tbm, pyr, _ = build_case(pkg, ctx, "TBM", pkg.CELL_TBM, a.size, a.reps)
    pyr.close()
    ctx.close()
    line = json.dumps(dict(reps=a.reps, build=[occ, tbm], score=score))
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
