#!/usr/bin/env python3
"""G7: the GMapping scorer (GmappingOccupancyObservationPE with its run cache, HC over it, GmappingParticleFilter) of the
COMPILED REFERENCE on windows that are no squares.  Writes tests/golden/gmapping_oblong.npz.

    python tests/golden/make_golden_gmapping_oblong.py        (where oracle/_ref/libslamref.so exists)

Every map the suite scored GMapping on was a square with equal origin components (tests/synth.py) or a crop with a
60-cell margin: no end cell near a rim, x and y exchangeable.  Here (tests/gmapping_oblong_cases.py has the layout):
  * two UnboundedPlainGridMaps of GmappingBaseCells at 0.1 m, `wide` 77 x 45 and `tall` 45 x 77 cells -- no side a
    multiple of 4 --, recorded WHOLE; the origin's components differ (asserted).  Contents: three append_scans of a
    360-beam scan generated from a ground truth (a room whose walls lie 3 cells inside the rims, a pillar) with the robot
    more than 1 m off the world origin in both axes, then single cells through GridMap::update: full cells in the four
    corners, along every rim and one cell inside it, a free cell between full ones, diagonal-only neighbours -- each with
    an obstacle mean off its cell's centre.  geometry() is asserted around every write: a map that grew is not written;
  * scans of 1 / 64 / 65 / 257 / 1080 beams generated from the same ground truth (beams 61 .. 66 and 253 .. 258
    shortened to 12 mm: one run of equal end cells across 63 -> 64 and 255 -> 256), filtered by the reference, even
    weights, raw trig provider; the 1080-beam scan once more behind the cached provider;
  * per (map, scan, group) one pose sequence scored by ONE scorer object: Ref.score at fullness_th 0.1 and 0.5;
  * one HC(6, 0.1, 0.1) trace per map with skip_rate 3 from a pose that puts beams across two rims;
  * three GmappingParticleFilter steps on a `wide` map (8 particles, map update off as in make_golden.gen_gmapping_pf).
What every group has to reach is asserted here (gmapping_oblong_cases.reaches / run_spans) and again by
tests/test_oracle_gmapping_oblong.py.  The output is a function of this script alone: two runs give the same bytes."""
import os
import sys

import numpy as np

GOLDEN_DIR = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(GOLDEN_DIR))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pyoracle as po  # noqa: E402
from gmapping_oblong_cases import (GROUPS, MAPS, MARGIN_CELLS, RIM_GROUPS, ROBOT_CELL, ROBOT_THETA, SCALE,  # noqa: E402
                                   SCAN_SIZES, SHORT, WALL, anchored_poses, cell_centre_frac, end_cells, group_targets,
                                   inner_poses, obstacle_of, reaches, run_spans, single_cells)
from make_golden import map_fields, trace_fields  # noqa: E402

PF_GP = [0.0, 0.1, 0.0, 0.03, 0.0, 0.0, 0.0, 0.0]
PF_DELTAS = [[0.0, 0.0, 0.0], [0.05, 0.03, 0.04], [-0.04, 0.06, -0.05]]
PF_N = 8


def ground_truth(R, name):
    """MockGridCell map: the room's walls WALL cells inside the rims and a pillar, occupancy 1"""
    W, H = MAPS[name]
    gt = R.map_create(po.REF_CELL_MOCK, po.MAP_UNBOUNDED_PLAIN, W, H, SCALE, 0.0)
    g0 = gt.geometry()
    ox, oy = g0["origin"]
    cells = [(x, y) for x in range(WALL, W - WALL) for y in (WALL, H - 1 - WALL)]
    cells += [(x, y) for y in range(WALL, H - WALL) for x in (WALL, W - 1 - WALL)]
    px, py = W // 2 - 4, H // 2 - 3
    cells += [(px + i, py + j) for i in range(3) for j in range(2)]
    for x, y in cells:
        gt.update(x - ox, y - oy, 1.0)
    assert gt.geometry() == g0
    return gt


def robot_pose(name, origin):
    x, y = cell_centre_frac(*ROBOT_CELL[name], origin, (0.5, 0.5))
    return np.array([x, y, ROBOT_THETA[name]])


def fill_map(R, m, gt, name):
    """the history both the scored map and the filter's map get"""
    g0 = m.geometry()
    W, H = MAPS[name]
    assert (g0["width"], g0["height"]) == (W, H), g0
    origin = g0["origin"]
    assert origin[0] != origin[1], "the origin must tell x from y"
    pose = robot_pose(name, origin)
    assert min(abs(pose[0]), abs(pose[1])) >= 1.0 and abs(abs(pose[0]) - abs(pose[1])) > 0.1
    raw = R.scan_generate(gt, pose, 15, 270, 360)
    r, _a, o, _f = raw.get()
    assert o.all() and r.max() < 8.0, "every beam of the mapping scan hits a wall"
    rs = np.random.RandomState(7)
    for _k in range(3):
        jit = pose + rs.randn(3) * [0.01, 0.01, 0.002]
        assert m.geometry() == g0
        R.append_scan(m, raw, jit, quality=1.0, base=(0.95, 1.0, 0.01, 1.0), blur=0.0)
        assert m.geometry() == g0, "the window must not grow"
    for ix, iy, full in single_cells(W, H):
        assert m.geometry() == g0
        for _rep in range(64):  # (a cell the scans saw as free takes several hits to pass fullness_th 0.1; most take one)
            m.update(ix - origin[0], iy - origin[1], 1.0 if full else 0.0, 1.0, is_occ=full, obst=obstacle_of(ix, iy, origin))
            assert m.geometry() == g0, "the window must not grow"
            if not full or m.to_data().payload[iy, ix, 0] >= 0.12:
                break
    return pose


def check_single_cells(md, name):
    W, H = MAPS[name]
    occ = md.payload[..., 0]
    for ix, iy, full in single_cells(W, H):
        assert (occ[iy, ix] >= 0.1) == full, (name, ix, iy, occ[iy, ix])
    cx, cy = W // 2 - 9, H // 2 + 5
    assert occ[cy, cx] >= 0.1 and 0 <= occ[cy, cx + 1] < 0.1 and occ[cy, cx + 2] >= 0.1  # a free cell between full ones
    for (ax, ay), (bx, by) in (((cx + 7, cy - 3), (cx + 8, cy - 2)), ((cx - 4, cy - 6), (cx - 5, cy - 5))):
        assert occ[ay, ax] >= 0.1 and occ[by, bx] >= 0.1 and occ[ay, bx] < 0.1 and occ[by, ax] < 0.1  # diagonal only
    full = occ >= 0.1
    means = md.payload[..., 1:][full] / SCALE
    off = np.abs(means - np.floor(means) - 0.5)
    assert np.count_nonzero(off.max(axis=1) > 0.05) > full.sum() // 2, "obstacle means are no cell centres"
    assert np.count_nonzero((occ >= 0.1) & (occ < 0.5)) > 3 and np.count_nonzero(occ >= 0.5) > 100  # th 0.5 differs
    return full


def make_scans(R, gt, name, pose, m, out):
    """the scored scans: generated from the ground truth at the robot's pose, short runs put in, filtered"""
    scans = {}
    # (the generator's beam count is what its accumulated angle gives, and a beam that hits nothing is left out: one
    # long scan, of which every size takes its share -- 1080 the first 1080 beams, evenly spaced for the cached provider)
    gr, ga, go, _f = R.scan_generate(gt, pose, 15, 270, 1100).get()
    assert gr.size >= 1080 and go.all() and np.ptp(np.diff(ga)) < 1e-12
    for n in SCAN_SIZES:
        pick = np.arange(n) if n == 1080 else np.round(np.linspace(7, gr.size - 9, n) if n > 1 else [gr.size * 0.4]).astype(int)
        r, a = gr[pick].copy(), ga[pick].copy()
        assert r.size == n
        r[61:67] = SHORT
        r[253:259] = SHORT
        inc = (a[-1] - a[0]) / (n - 1) if n > 1 else 1.0
        variants = [("s%d" % n, po.TRIG_RAW)] + ([("s%dc" % n, po.TRIG_CACHED)] if n == 1080 else [])
        for key, trig in variants:
            if trig == po.TRIG_CACHED:
                acc = np.zeros(n)  # accumulated, as CachedTrigonometryProvider::update builds its table
                v = a[0]
                for k in range(n):
                    acc[k] = v
                    v += inc
                assert np.abs(acc - a).max() < 1e-9
                scan = R.scan_create(r, a, None, trig, a[0], a[-1] + 2 * inc, inc)
            else:
                scan = R.scan_create(r, a)
            spe = R.spe_create(po.OOPE_GMAPPING, po.OIE_DISCREPANCY, 0)
            fs = R.filter_scan(spe, scan, pose, m)
            fr, fa, _fo, ff = fs.get()
            assert np.array_equal(fr, r) and np.array_equal(fa, a) and np.all(ff == 1.0)  # unbounded map: nothing is filtered
            w = R.scan_weights(spe, fs)
            pre = "%s_%s_" % (name, key)
            if trig == po.TRIG_CACHED:
                ts, tc = scan.trig_table()
                out.update({pre + "a_min": np.array(a[0]), pre + "a_inc": np.array(inc), pre + "tab_sin": ts,
                            pre + "tab_cos": tc})
                idx = np.round((a - a[0]) / inc).astype(np.int64)
                assert idx.max() < ts.size and np.array_equal(idx, np.arange(n))
            else:
                out.update({pre + "range": fr, pre + "angle": fa, pre + "weight": w, pre + "factor": ff})
            scans[key] = (scan, po.ScanData(fr, fa, w, ff))
    return scans


def main():
    if not po.ref_available():
        sys.exit("oracle/_ref/libslamref.so missing: run `make -C oracle ref` where the reference tree exists")
    R = po.Ref()
    out = dict(scale=np.array(SCALE))
    n_scores = n_seq = 0
    for mi, (name, (W, H)) in enumerate(MAPS.items()):
        gt = ground_truth(R, name)
        m = R.map_create(po.REF_CELL_GMAPPING, po.MAP_UNBOUNDED_PLAIN, W, H, SCALE)
        g0 = m.geometry()
        origin = g0["origin"]
        pose = fill_map(R, m, gt, name)
        md = m.to_data()
        full = check_single_cells(md, name)
        out.update(map_fields(md, name + "_map_"))
        out[name + "_robot_pose"] = pose
        scans = make_scans(R, gt, name, pose, m, out)
        targets = group_targets(W, H)
        spans = {63: False, 255: False}
        for key, (scan_h, sd) in scans.items():
            raw_key = key[:-1] if key.endswith("c") else key  # (the cached scan is the same scan: the same poses)
            parts, lens = [], []
            for gi, grp in enumerate(GROUPS):
                if grp == "inner":
                    poses = inner_poses(name, origin, 40 + mi)
                else:
                    poses, _anchors = anchored_poses(sd.range, sd.angle, targets[grp], origin, gi)
                ec, margin = end_cells(sd, poses, origin)
                assert margin > MARGIN_CELLS, (name, key, grp, margin)
                assert reaches(grp, W, H, ec), (name, key, grp)
                for first in spans:
                    spans[first] |= run_spans(ec, full, first, W, H)
                parts.append(poses)
                lens.append(len(poses))
            scores = np.zeros((2, sum(lens)))
            at = 0
            for grp, poses in zip(GROUPS, parts):
                for ti, th in enumerate((0.1, 0.5)):
                    # ONE scorer object (one OOPE cache) per sequence: the cache carries across poses (Q19)
                    # (it filters the scan itself first: EvenSPW takes its weight from the scan it filtered)
                    spe = R.spe_create(po.OOPE_GMAPPING, po.OIE_DISCREPANCY, 0, gm_th=th)
                    fs = R.filter_scan(spe, scan_h, pose, m)
                    assert fs.size() == sd.n and np.array_equal(R.scan_weights(spe, fs), sd.weight)
                    s = R.score(spe, fs, m, poses)
                    assert m.geometry() == g0 and np.all(np.isfinite(s)), (name, key, grp, th)
                    scores[ti, at:at + len(poses)] = s
                    n_scores += s.size
                    n_seq += 1
                s = scores[0, at:at + len(poses)]
                # far: every score 0.  A rim group whose scores are all 0 could not tell a window from its transposition
                # (the lone beam of the 1-beam scan aimed two cells outside reaches nothing: per group over all scans, CPU test)
                assert (not s.any()) if grp == "far" else (s.any() or sd.n == 1), (name, key, grp)
                at += len(poses)
            if key == raw_key:
                out["%s_%s_poses" % (name, key)] = np.concatenate(parts)
            else:
                assert np.array_equal(out["%s_%s_poses" % (name, raw_key)], np.concatenate(parts))
            out["%s_%s_scores" % (name, key)] = scores
            if "group_len" in out:
                assert out["group_len"].tolist() == lens
            out["group_len"] = np.array(lens)
        assert spans[63] and spans[255], spans
        # HC(6, 0.1, 0.1), skip_rate 3, from a pose that throws the scan's wall hits across the right and the bottom rim
        r, a = out[name + "_s1080_range"], out[name + "_s1080_angle"]
        scan = R.scan_create(r, a)
        init = pose + [(WALL + 0.4) * SCALE, -(WALL - 0.2) * SCALE, 0.02]
        spe3 = R.spe_create(po.OOPE_GMAPPING, po.OIE_DISCREPANCY, 0, skip_rate=3)
        t = R.process_scan(R.matcher_create(po.SM_HC, spe3, [6, 0.1, 0.1]), scan, init, m)
        assert m.geometry() == g0
        fs3 = R.filter_scan(spe3, scan, init, m)
        out[name + "_hc_init"] = init
        hr, ha = fs3.get()[:2]
        assert np.array_equal(hr, r[::3]) and np.array_equal(ha, a[::3])  # (skip_rate 3: what the tests take from s1080)
        out.update(trace_fields(t, name + "_hc6_skip3_"))
        acc = t["poses"][t["accepted"] != 0]
        assert len(acc) >= 2, "the climb must move"
        ec, _ = end_cells(po.ScanData(hr, ha), acc, origin)
        inside = (ec[..., 0] >= 0) & (ec[..., 0] < W) & (ec[..., 1] >= 0) & (ec[..., 1] < H)
        beyond = ~inside
        on_rim = inside & ((ec[..., 0] == 0) | (ec[..., 0] == W - 1) | (ec[..., 1] == 0) | (ec[..., 1] == H - 1))
        print(name, "HC: %d calls, %d accepted; beams beyond / on a rim per accepted pose:" % (t["n_calls"], len(acc)),
              beyond.sum(axis=1), on_rim.sum(axis=1))
        # (the climb walks back towards the room: its first accepted poses have beams on and beyond a rim, its last none)
        assert np.count_nonzero(beyond.any(axis=1) & on_rim.any(axis=1)) >= 3, "accepted poses put beams on and across a rim"
        out[name + "_map_after"] = m.to_data().payload
        assert np.array_equal(out[name + "_map_after"], md.payload, equal_nan=True), "scoring wrote to the map"
        del out[name + "_map_after"]

    # three filter steps on a `wide` map of the filter's own (UnboundedLazyTiledGridMap sized through w, h)
    name = "wide"
    W, H = MAPS[name]
    gt = ground_truth(R, name)
    seeds = np.arange(1000, 1000 + PF_N, dtype=np.uint32)
    g = po.RefGmapping(R, PF_N, W, H, SCALE, PF_GP, seeds, skip_rate=3, map_max_range=0.0)
    mview = g.map()
    pose0 = fill_map(R, mview, gt, name)
    g0 = mview.geometry()
    md = mview.to_data()
    assert np.array_equal(md.payload, out["wide_map_payload"]) and md.origin == tuple(out["wide_map_origin"])
    out["pf_gp"], out["pf_seeds"], out["pf_n_steps"] = np.array(PF_GP), seeds, np.array(len(PF_DELTAS))
    true = np.zeros(3)
    for k, d in enumerate(PF_DELTAS):
        true = true + np.array(d)
        tp = pose0 + true
        tp[:2] = (np.floor(tp[:2] / SCALE) + 0.5) * SCALE  # the scan generator refuses poses on a cell boundary
        r, a, o, _ = R.scan_generate(gt, tp, 15, 270, 720).get()
        assert o.all()
        dd = pose0 if k == 0 else np.array(d)
        extra = np.arange(5000 + 100 * k, 5000 + 100 * k + PF_N, dtype=np.uint32)
        res, poses, w, ms = g.step(R.scan_create(r, a, o), dd, 7 + k, extra)
        assert mview.geometry() == g0
        pre = "pf_step%d_" % k
        out.update({pre + "range": r, pre + "angle": a, pre + "delta": dd, pre + "resampled": np.array(int(res)),
                    pre + "poses": poses, pre + "weights": w, pre + "master": ms})
        assert min(np.abs(poses[:, 0]).min(), np.abs(poses[:, 1]).min()) >= 1.0
    assert np.array_equal(mview.to_data().payload, md.payload)
    # what both maps (all three steps) share is kept once: the generator's angles depend on nothing but the beam count
    for k in [k for k in out if k.startswith("tall_s") and k.split("_")[-1] in ("angle", "weight", "factor", "sin", "cos", "min", "inc")]:
        assert np.array_equal(out[k], out["wide" + k[4:]]), k
        del out[k]
    for k in (1, 2):
        assert np.array_equal(out["pf_step%d_angle" % k], out["pf_step0_angle"])
        del out["pf_step%d_angle" % k]
    path = os.path.join(GOLDEN_DIR, "gmapping_oblong.npz")
    np.savez_compressed(path, **{k: out[k] for k in sorted(out)})
    print("wrote gmapping_oblong.npz %d KiB: %d scores in %d sequences, origins %s / %s" % (
        os.path.getsize(path) // 1024, n_scores, n_seq,
        out["wide_map_origin"].tolist(), out["tall_map_origin"].tolist()))


if __name__ == "__main__":
    main()
