#!/usr/bin/env python3
"""Golden vectors FAR FROM THE WORLD ORIGIN, captured from the compiled reference.  Writes tests/golden/placed.npz.

Every other golden was recorded around (0, 0).  Here the scenes of tests/placed_scenes.py stand at the four Q stations
-- one per quadrant, 1000 ... 2000 m out at 0.1 m cells, true headings 0.3 / 3.1 / -2.9 / 7.6 -- and everything the
reference does there is recorded as data:

  per station and cell class (mean, tbm, gmapping), const and area occupancy estimator
      a MAP_UNBOUNDED_LAZY_TILED map that starts around (0, 0) and grows out to the station; three
      GridMapScanAdder::append_scan calls from jittered station poses (quality 0.9, blur 0.3, GMapping 0); after each one
      a WINDOW EXPORT of the 108 x 76 cells around the scene -- payload and update counters -- never the whole map
      (tbm under the area estimator: the last snapshot alone; its four masses per cell do not compress);
  on the final const-estimator maps
      estimate_scan_probability of 64 poses around the station under the cached AND the raw trigonometry provider
      (mean + even weights, tbm + VinySlam weights), the Max / Mean / OverlapWeighted OOPEs over an oblong analysis area
      (24 poses), the GMapping OOPE on the GMapping map (one estimator, hence one cache, across the poses);
      process_scan traces: HC [6, 0.1, 0.1], [128, 0.1, 0.1], [128, 1e-9, 1e-9], MC [666666, 0.2, 0.1, 20, 100] and BF
      over 9 x 9 x 5 poses (mean map, cached provider), HC [6, 0.1, 0.1] on the tbm map (raw provider) and over the
      GMapping OOPE; filter_scan of the raw scan at the station pose.

The ground truth is synth.make_world on a 64-cell raster (a box of 5.6 m with pillars): the whole scene, blur and pose
jitter included, fits the 108 x 76 window, so the window IS the map as far as any end point can tell.

Asserted here, so that a fixture that lost one of them cannot be written: every window's origin lies outside the window,
the quadrants' signs, nothing touched next to the window's rim, every trace accepts candidates (but [128, 1e-9, 1e-9]: steps that
small move no end point into another cell; that trace is there for its tail), the [128, ...] traces end in repeated
best poses.
The file is written with fixed zip time stamps: two runs give the same bytes.

Run where oracle/_ref/libslamref.so exists, in a fresh process (the area estimator's static Shift_Amount is pinned
first, as in make_golden_area.py):  python tests/golden/make_golden_placed.py"""
import io
import os
import sys
import zipfile

import numpy as np

GOLDEN_DIR = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(GOLDEN_DIR))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pyoracle as po  # noqa: E402
import placed_scenes as ps  # noqa: E402

SCALE, RASTER, N_BEAMS = 0.1, 64, 360
WIN_W, WIN_H = 108, 76  # (at most 128 x 96; no square, the width no multiple of 16)
RIM = 2  # cells next to the window's rim that must stay untouched
STD_BASE, TBM_BASE = (0.95, 1.0, 0.01, 1.0), (0.95, 0.04, 0.01, 0.003)
CLASSES = {"mean": (po.REF_CELL_MEAN, STD_BASE, 0.3), "tbm": (po.REF_CELL_TBM, TBM_BASE, 0.3),
           "gmapping": (po.REF_CELL_GMAPPING, STD_BASE, 0.0)}
QUALITY = 0.9
WIN_AREA = (0.0, 0.25, 0.0, 0.15)  # bot, top, left, right: oblong; the reference re-centres it on the end point
HC_TRACES = {"hc6": [6, 0.1, 0.1], "hc128": [128, 0.1, 0.1], "hc128tiny": [128, 1e-9, 1e-9]}
MC_PARAMS = [666666, 0.2, 0.1, 20, 100]
BF_PARAMS = [-0.2, 0.2, 0.05, -0.2, 0.2, 0.05, -0.04, 0.04, 0.02]  # 9 x 9 x 5
SIGNS = {"Q1": (1, 1), "Q2": (-1, 1), "Q3": (-1, -1), "Q4": (1, -1)}


def save_stable(path, arrays):
    """np.savez_compressed with fixed time stamps and a fixed member order."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def window_box(station):
    (kx, ky), _ = ps.STATIONS[station]
    return kx - WIN_W // 2, ky - WIN_H // 2


def trace_fields(t, prefix):
    return {prefix + "prob": np.array(t["prob"]), prefix + "delta": t["delta"], prefix + "n_calls": np.array(t["n_calls"]),
            prefix + "poses": t["poses"], prefix + "scores": t["scores"], prefix + "accepted": t["accepted"]}


def check_trace(t, name, tail, want_accepts=True):
    """acceptances behind the initial pose (call 0 is always one); tail: how many calls at the end ARE the best pose"""
    assert t["accepted"][0] == 1
    acc = np.nonzero(t["accepted"])[0]
    if want_accepts:
        assert len(acc) > 1, "%s: no candidate was accepted" % name
    if tail:
        best = t["poses"][acc[-1]]
        n = 0
        while n < t["n_calls"] and np.array_equal(t["poses"][-1 - n], best):
            n += 1
        assert n >= 6, "%s: the trace does not end in repeated best poses (%d)" % (name, n)
        return n
    return 0


def main():
    if not po.ref_available():
        sys.exit("oracle/_ref/libslamref.so missing: run `make -C oracle ref` where the reference tree exists")
    R = po.Ref()
    pin = R.map_create(po.REF_CELL_MEAN, po.MAP_UNBOUNDED_PLAIN, 20, 20, SCALE)  # Shift_Amount = 0.01 * scale (Q27)
    R.append_scan(pin, R.scan_create([0.01], [0.0]), (0.05, 0.05, 0.0), occ_est=1)
    out = dict(scale=np.array(SCALE), raster=np.array(RASTER), n_beams=np.array(N_BEAMS), window=np.array([WIN_W, WIN_H]),
               shift_amount=np.array(0.01 * SCALE), quality=np.array(QUALITY), win_area=np.array(WIN_AREA),
               mc_params=np.array(MC_PARAMS, dtype=np.float64), bf_params=np.array(BF_PARAMS))
    for k, v in HC_TRACES.items():
        out[k + "_params"] = np.array(v, dtype=np.float64)
    for name, (_c, base, blur) in CLASSES.items():
        out[name + "_base"], out[name + "_blur"] = np.array(base), np.array(blur)
    tails = {}
    for st in ps.Q_STATIONS:
        (kx, ky), heading = ps.STATIONS[st]
        x0, y0 = window_box(st)
        origin = (-x0, -y0)
        assert not (0 <= origin[0] < WIN_W) and not (0 <= origin[1] < WIN_H), "the window's origin must lie outside it"
        sc = ps.place(st, size=RASTER, scale=SCALE, n_beams=N_BEAMS, raw=True)
        assert (np.sign(sc["true_pose"][:2]) == SIGNS[st]).all() and min(abs(sc["true_pose"][:2])) > 1000.0, st
        assert sc["true_pose"][2] == heading
        r, a, o = sc["raw"]
        rs = np.random.RandomState(ps.SEEDS[st])
        o = o.copy()
        o[rs.rand(r.size) < 0.08] = 0  # max-range readings: no obstacle at the end of the beam
        assert o.sum() > 300 and (o == 0).sum() > 10 and r.max() < 4.5
        inc = a[1] - a[0]
        a_min, a_max_passed = a[0], a[-1] + 2 * inc
        pre = st + "_"
        out.update({pre + "raw_range": r, pre + "raw_angle": a, pre + "raw_occ": o, pre + "a_min": np.array(a_min),
                    pre + "a_inc": np.array(inc), pre + "a_max_passed": np.array(a_max_passed),
                    pre + "true_pose": sc["true_pose"], pre + "init_pose": sc["init_pose"],
                    pre + "origin": np.array(origin)})
        app_poses = np.array([sc["local"] + rs.randn(3) * [0.01, 0.01, 0.002] for _ in range(3)]) + sc["shift"]
        out[pre + "append_poses"] = app_poses
        raw_scan = R.scan_create(r, a, o)
        final = {}
        for name, (cell, base, blur) in CLASSES.items():
            for est in (0, 1):
                m = R.map_create(cell, po.MAP_UNBOUNDED_LAZY_TILED, WIN_W, WIN_H, SCALE, 0.5)
                for k, p in enumerate(app_poses):
                    R.append_scan(m, raw_scan, p, quality=QUALITY, occ_est=est, base=base, blur=blur)
                    md = m.window(x0, y0, WIN_W, WIN_H)
                    tag = "%s%s%s_step%d_" % (pre, name, "_area" if est else "", k)
                    aux = m.aux_window(x0, y0, WIN_W, WIN_H)
                    if (name, est) != ("tbm", 1) or k == 2:  # (tbm + area: four continuous masses per cell -- the last snapshot alone)
                        out[tag + "payload"] = md.payload
                        if aux is not None:
                            out[tag + "aux"] = aux
                    stride = md.payload.shape[2]
                    touched = (md.payload != md.unknown[:stride]).any(axis=2)
                    assert touched.sum() > 1000, (tag, touched.sum())
                    inner = np.zeros_like(touched)
                    inner[RIM:-RIM, RIM:-RIM] = True
                    assert not touched[~inner].any(), tag + ": touched cells next to the window's rim"
                    wide = m.window(x0 - 8, y0 - 8, WIN_W + 16, WIN_H + 16)  # ... and none beyond it
                    ring = np.ones(wide.payload.shape[:2], bool)
                    ring[8:-8, 8:-8] = False
                    assert (wide.payload[ring] == md.unknown[:stride]).all(), tag + ": touched cells outside the window"
                g = m.geometry()
                assert g["width"] > 9000 and g["height"] > 9000, "the map was expected to span back to (0, 0)"
                if est == 0:
                    final[name] = (m, md)
                    out[pre + name + "_unknown"] = md.unknown
        # ---- scoring on the final const-estimator maps
        poses = ps.candidates(sc, 64, 100 + ps.SEEDS[st])
        out[pre + "poses"] = poses
        for tname, trig in (("cached", po.TRIG_CACHED), ("raw", po.TRIG_RAW)):
            scan = R.scan_create(r, a, o, trig, a_min, a_max_passed, inc)
            if trig == po.TRIG_CACHED:
                out[pre + "tab_sin"], out[pre + "tab_cos"] = scan.trig_table()
            for name, weighting in (("mean", 0), ("tbm", 1)):
                m, _md = final[name]
                spe = R.spe_create(po.OOPE_OBSTACLE, po.OIE_DISCREPANCY, weighting)
                fs = R.filter_scan(spe, scan, sc["init_pose"], m)
                fr, fa, _fo, ff = fs.get()
                key = "%s%s_%s_" % (pre, name, tname)
                # the filter kept the occupied points, in order, factors 1: recorded once per station as indices
                kept = np.nonzero(o)[0].astype(np.int32)
                assert np.array_equal(fr, r[kept]) and np.array_equal(fa, a[kept]) and np.all(ff == 1.0)
                out[pre + "kept"] = kept
                wts = R.scan_weights(spe, fs)
                if weighting:
                    assert tname == "cached" or np.array_equal(wts, out[pre + "viny_weight"])
                    out[pre + "viny_weight"] = wts
                else:
                    assert np.all(wts == 1.0 / kept.size)
                out[key + "scores"] = R.score(spe, fs, m, poses)
                for kname, kind in (("max", po.OOPE_MAX), ("mean", po.OOPE_MEAN), ("overlap", po.OOPE_OVERLAP)):
                    spe2 = R.spe_create(kind, po.OIE_DISCREPANCY, weighting)
                    fs2 = R.filter_scan(spe2, scan, sc["init_pose"], m)
                    out[key + "win_" + kname] = R.score(spe2, fs2, m, poses[:24], WIN_AREA)
            # the GMapping OOPE: ONE estimator (one cache) scores all poses in order
            m, _md = final["gmapping"]
            gposes = ps.candidates(sc, 64, 200 + ps.SEEDS[st], sigma=(0.05, 0.05, 0.02))
            out[pre + "gm_poses"] = gposes
            spe = R.spe_create(po.OOPE_GMAPPING, po.OIE_DISCREPANCY, 0)
            fs = R.filter_scan(spe, scan, sc["init_pose"], m)
            key = "%sgmapping_%s_" % (pre, tname)
            assert np.array_equal(fs.get()[0], r[out[pre + "kept"]])
            out[key + "scores"] = R.score(spe, fs, m, gposes)
            if trig == po.TRIG_RAW:
                mt = R.matcher_create(po.SM_HC, R.spe_create(po.OOPE_GMAPPING, po.OIE_DISCREPANCY, 0), HC_TRACES["hc6"])
                t = R.process_scan(mt, scan, sc["init_pose"], m)
                check_trace(t, key + "hc6", False)
                out.update(trace_fields(t, key + "hc6_"))
                m, _md = final["tbm"]
                mt = R.matcher_create(po.SM_HC, R.spe_create(po.OOPE_OBSTACLE, po.OIE_DISCREPANCY, 1), HC_TRACES["hc6"])
                t = R.process_scan(mt, scan, sc["init_pose"], m)
                check_trace(t, pre + "tbm_raw_hc6", False)
                out.update(trace_fields(t, pre + "tbm_raw_hc6_"))
            else:
                m, _md = final["mean"]
                spe = R.spe_create(po.OOPE_OBSTACLE, po.OIE_DISCREPANCY, 0)
                for hname, prm in HC_TRACES.items():
                    t = R.process_scan(R.matcher_create(po.SM_HC, spe, prm), scan, sc["init_pose"], m)
                    tails[(st, hname)] = (check_trace(t, pre + hname, hname != "hc6", want_accepts=hname != "hc128tiny"), int(t["accepted"].sum()) - 1, t["n_calls"])
                    out.update(trace_fields(t, "%smean_cached_%s_" % (pre, hname)))
                t = R.process_scan(R.matcher_create(po.SM_MC, spe, MC_PARAMS), scan, sc["init_pose"], m)
                check_trace(t, pre + "mc", False)
                out.update(trace_fields(t, pre + "mean_cached_mc_"))
                t = R.process_scan(R.matcher_create(po.SM_BF, spe, BF_PARAMS), scan, sc["init_pose"], m)
                check_trace(t, pre + "bf", False)
                assert t["n_calls"] >= 9 * 9 * 5
                out.update(trace_fields(t, pre + "mean_cached_bf_"))
    path = os.path.join(GOLDEN_DIR, "placed.npz")
    save_stable(path, out)
    size = os.path.getsize(path)
    assert size < 900 * 1024, "placed.npz has %d bytes: larger than the largest fixture committed so far" % size
    print("wrote placed.npz %d KiB; closed tails (identical poses at the end of the trace) %r" % (size // 1024, tails))


if __name__ == "__main__":
    main()
