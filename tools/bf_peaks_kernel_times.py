"""What the peaks reduction adds to a sweep: the kernels' own times of the lone slamhip_matcher_bf_peaks call, from a kernel
trace, beside the scoring launch's -- the `kernel_times` block of the record tools/bf_peaks_ms.py writes.  Two steps:

    rocprofv3 --kernel-trace --stats -d DIR -o peaks -- python tools/bf_peaks_kernel_times.py run
    python tools/bf_peaks_kernel_times.py summarize DIR/peaks_results.db --into profiles/<date>_bf_peaks_ms.json

run        bf_peaks_ms.py's scene, K = 1: per sweep (201 x 201 x 1, 41 x 41 x 21) and radius ((3, 3, 0), (2, 2, 2)) CALLS lone
           calls one after another.  Needs a GPU.
summarize  reads the trace's `kernels` view (name, start, end in ns), cuts the dispatches into groups of CALLS calls by
           counting the ordering kernel -- every call ends with one -- and writes per group and kernel the median [min, max]
           microseconds per dispatch into the JSON document's `kernel_times`.  Needs no GPU."""
import argparse
import json
import os
import sqlite3
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWEEPS = (("201x201x1", [-1.0, 1.0, 0.01, -1.0, 1.0, 0.01, 0.0, 0.0, 1.0]),
          ("41x41x21", [-0.2, 0.2, 0.01, -0.2, 0.2, 0.01, -0.1, 0.1, 0.01]))
RADII = ((3, 3, 0), (2, 2, 2))
CALLS = 30
KERNELS = ("k_bf_poses", "k_score_point", "k_bf_peaks_plane", "k_bf_peaks_theta", "k_bf_peaks_order")


def run():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import __graft_entry__ as ge
    from bench_legs.common import rotating_scenes
    from synth import make_scene
    pkg = ge.load_package()
    ctx = pkg.Context(0)
    sc = make_scene(cell_model=0, size=1000, scale=0.05, n_beams=1080, seed=100)
    s = rotating_scenes(sc, 1080, "even")[0]
    ctx.upload_map(0, sc["map"])
    ctx.scan_upload(s["range"], *pkg.beam_trig(s["angle"]), s["weight"])
    for name, r9 in SWEEPS:
        m = pkg.Matcher(ctx, "BF", pkg.spe_cfg(), r9)
        for radius in RADII:
            for _ in range(CALLS):
                r = m.bf_peaks(0, s["init_pose"], radius, 0.97, 0.0, 16)
            print(name, radius, r["shape"], r["n_found"], flush=True)
        m.close()
    ctx.close()


def summarize(db_path, into):
    db = sqlite3.connect(db_path)
    cur = db.cursor()
    cols = [r[1] for r in cur.execute("pragma table_info(kernels)")]
    ni, si, ei = cols.index("name"), cols.index("start"), cols.index("end")
    groups, done = {}, 0
    for row in cur.execute("select * from kernels order by start"):
        short = next((k for k in KERNELS if k in row[ni]), None)
        if short is None:
            continue  # (uploads, fills)
        groups.setdefault((done // CALLS, short), []).append((row[ei] - row[si]) / 1e3)
        if short == "k_bf_peaks_order":
            done += 1
    labels = [(name, radius) for name, _ in SWEEPS for radius in RADII]
    assert done == CALLS * len(labels), "the trace holds %d calls, not %d" % (done, CALLS * len(labels))
    rows = []
    for g, (name, radius) in enumerate(labels):
        row = {"sweep": name, "radius": list(radius)}
        for k in KERNELS:
            v = groups[(g, k)]
            assert len(v) == CALLS, (name, radius, k, len(v))
            row[k] = [round(statistics.median(v), 2), round(min(v), 2), round(max(v), 2)]
        rows.append(row)
        print(name, radius, " ".join("%s %.2f" % (k, row[k][0]) for k in KERNELS))
    block = {"what": "the lone call's kernels, microseconds per dispatch: median [min, max] of %d calls per row, from a kernel trace "
                     "of its own run (K = 1, bf_peaks_ms.py's scene): the scoring launch beside the three peaks launches" % CALLS,
             "made_by": "tools/bf_peaks_kernel_times.py (run under rocprofv3 --kernel-trace, then summarize)", "rows": rows}
    if into:
        doc = json.load(open(into))
        doc["kernel_times"] = block
        json.dump(doc, open(into, "w"), indent=1)
    return block


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    sub.add_parser("run")
    sp = sub.add_parser("summarize")
    sp.add_argument("db")
    sp.add_argument("--into", default=None, help="the JSON record of tools/bf_peaks_ms.py to put the block into")
    a = ap.parse_args()
    if a.cmd == "run":
        run()
    else:
        summarize(a.db, a.into)
