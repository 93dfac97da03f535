#!/usr/bin/env python3
"""Time the map render on the GPU (csrc/map_render.hip) against the route it replaces.

    python tools/render_ms.py [--reps 20] [--out FILE.json]

For a 2000 x 2000 OCC map and a 4000 x 4000 TBM map (random payloads), whole map, both formats:
  render_ms    Context.map_render: kernel + one device-to-host copy of 1 byte per cell + the wait (host clock around the
               call, which ends in a stream synchronise); median and min / max over --reps calls after two warm-up calls
  download_ms  the only route to the same bytes without the kernel: Context.map_download_window of the whole window (8
               or 32 bytes per cell over PCIe) + render_cells on the host; split into its two parts
  kernel_ms    the render kernel alone: the HIP event pair the library records around it while profiling is on
               (slamhip_profile_enable), mean over the calls
  traffic      the bytes the kernel has to move (cells x (8 or 32 read + 1 written)) over kernel_ms, and that rate's
               share of the 8 TB/s HBM peak and of the 6.3 TB/s a copy kernel reaches
The bytes of the two routes are compared before anything is timed.  Needs a GPU; prints one JSON object."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

HBM_PEAK_GBS, HBM_COPY_GBS = 8000.0, 6300.0


def spread(ts):
    ts = np.asarray(ts) * 1e3
    return dict(median=float(np.median(ts)), min=float(ts.min()), max=float(ts.max()))


def case(pkg, ctx, name, model, size, kind, reps):
    rs = np.random.RandomState(7)
    stride = pkg.STRIDE[model]
    if stride == 1:
        payload = rs.rand(size, size, 1)
        unknown = [0.5]
    else:
        payload = rs.dirichlet([1, 1, 1, 1], size * size).reshape(size, size, 4)
        unknown = [1.0, 0.0, 0.0, 0.0]
    ctx.map_bind(0, model, size, size, [size // 2, size // 2], 0.05, unknown)
    ctx.map_upload_window(0, 0, 0, payload)
    del payload
    cells = size * size
    res = dict(map="%s %d x %d" % (name, size, size), cells=cells, read_bytes_per_cell=8 * (1 if stride == 1 else 4))
    for fmt, fname in ((pkg.RENDER_OCCGRID, "occgrid"), (pkg.RENDER_PGM, "pgm")):
        got = ctx.map_render(0, fmt, kind)
        pay = ctx.map_download_window(0, 0, 0, size, size, stride)
        want = pkg.render_cells(model, pay, fmt, kind)
        assert np.array_equal(got, want[::-1] if fmt == pkg.RENDER_PGM else want), "the two routes disagree"
        ctx.map_render(0, fmt, kind)
        t_render, t_down, t_conv = [], [], []
        for _ in range(reps):  # the two routes alternate
            t0 = time.perf_counter()
            ctx.map_render(0, fmt, kind)
            t1 = time.perf_counter()
            pay = ctx.map_download_window(0, 0, 0, size, size, stride)
            t2 = time.perf_counter()
            pkg.render_cells(model, pay, fmt, kind)
            t3 = time.perf_counter()
            t_render.append(t1 - t0)
            t_down.append(t2 - t1)
            t_conv.append(t3 - t2)
        ctx.profile_enable(True)
        ctx.profile_read(reset=True)
        for _ in range(reps):
            ctx.map_render(0, fmt, kind)
        kernel_ms = ctx.profile_read(reset=True)[0] / reps
        ctx.profile_enable(False)
        traffic = cells * (res["read_bytes_per_cell"] + 1)
        gbs = traffic / (kernel_ms * 1e-3) / 1e9
        total = np.asarray(t_down) + np.asarray(t_conv)
        res[fname] = dict(render_ms=spread(t_render), download_route_ms=spread(total), download_ms=spread(t_down),
                          host_convert_ms=spread(t_conv), kernel_ms=kernel_ms, kernel_traffic_bytes=traffic, kernel_gbs=gbs,
                          share_of_hbm_peak=gbs / HBM_PEAK_GBS, share_of_copy_rate=gbs / HBM_COPY_GBS,
                          speedup_median=float(np.median(total) / np.median(t_render)))
    ctx.map_release(0)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = ge.load_package()
    ctx = pkg.Context(0)  # raises without a GPU: there is nothing to time on a CPU
    out = dict(reps=a.reps, cases=[case(pkg, ctx, "OCC", pkg.CELL_OCC, 2000, 0, a.reps),
                                   case(pkg, ctx, "TBM", pkg.CELL_TBM, 4000, pkg.OCC_TBM_CONSISTENT, a.reps)])
    ctx.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
