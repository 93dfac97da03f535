#!/usr/bin/env python3
"""Generate tests/golden/placed_generate.npz from the COMPILED REFERENCE: LaserScanGenerator::laser_scan_2D far from the
world origin, at the four Q stations of tests/placed_scenes.py (one per quadrant, 1000 ... 2000 m out at 0.1 m cells).

    python tests/golden/make_golden_placed_generate.py

The sibling of make_golden_scan_generate.py (whose maps all hold (0, 0)) and of make_golden_placed.py (whose way of
getting there it shares): every map is a MAP_UNBOUNDED_LAZY_TILED map that starts around (0, 0) and grows out to the
station; what is recorded of it is the WINDOW of 108 x 76 cells around the station, never the whole map -- asserted to
hold every cell that was ever touched, so the window is the map as far as any beam can tell.

Per station <st>
  maps   <st>_cecum (a cecum stamped at occupancy 1, threshold 1) and <st>_mean, <st>_tbm, <st>_gmapping (three
         append_scans of scans generated from the cecum): _payload [76, 108, stride], _origin (outside the window),
         _scale, _unknown, _cell_model
  calls  <st>_cecum_short (2 m), _cecum_long (100 m: walks of 1000 cells, nearly all of them outside the window),
         _cecum_ties (from a cell centre along the slopes 1/3: vertex ties), _cecum_astray (one find_astray_call search
         run AT the station: a walk the reference restarts with Bresenham), _cecum_touch (beams that clip the corner of
         an occupied cell), _slam_mean, _slam_tbm, _slam_gmapping (8 m); per call <c>:
         <c>_map (name of the map), <c>_poses [3, 3], <c>_lsp (max_dist, fov_deg, pts_nm), <c>_threshold, <c>_occ_kind,
         <c>_range [3, B], <c>_status [3, B] uint8, <c>_hit_step [3, B] (index of the hit cell in the reference's
         world_to_cells list; -1 no hit, -2 the end point floors into no cell of the list)
  every call has 37 ... 90 beams; the third pose of the cecum_short / cecum_long / slam calls stands outside the window.

A pose enters only when the library's host routine accepts it (no "cell boundary" refusal) and reports no status 2 for
it on the window: the reference's own assertions end the process, and a failed assertion is no recorded result.  Out
here the reference's are_equal tolerance, 1e-7 * max(1, |a|, |b|), is 1e-4 ... 2e-4 m wide, so a pose that was fine next
to (0, 0) may be refused: it is then moved by 1.1 mm steps until it passes (printed).

Asserted per station, so that a fixture that lost a case cannot be written: tie, astray, touch, leaves_window, hit_early,
hit_late, no_hit, robot_outside; every window's origin lies outside it; nothing was touched outside the window.

Measured where this fixture was made (one process, all four stations): 2 s wall clock, 0.1 GB peak resident set, a
fixture of 111 KiB -- the tiled maps allocate only the tiles that were touched, however far the map spans.  The three N
stations of placed_scenes.py (500 ... 1500 cells out) are not used here: they are meant for the reference's DENSE
pyramid maps, and no station had to be moved inward for this fixture."""
import math
import os
import resource
import sys
import time

import numpy as np

GOLDEN_DIR = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(GOLDEN_DIR))
sys.path.insert(0, ROOT)
sys.path.insert(0, GOLDEN_DIR)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pyoracle as po  # noqa: E402
import placed_scenes as ps  # noqa: E402
import __graft_entry__ as ge  # noqa: E402
from make_golden_placed import save_stable  # noqa: E402
from make_golden_scan_generate import TOP, angle_list, occupancy  # noqa: E402
from test_gpu_mapupdate_edges import _walk_goes_astray  # noqa: E402  (a plain restatement of the walk: case search only)

S = 0.1
WIN_W, WIN_H = 108, 76
STAT_KEYS = ("robot_outside", "max_cells", "short_walks", "astray", "tie", "leaves_window", "hit_early", "hit_late", "touch",
             "no_hit", "unlocated")


class Station:
    def __init__(self, R, pkg, name, variant):
        self.R, self.pkg, self.name, self.variant = R, pkg, name, variant
        (self.kx, self.ky), _ = ps.STATIONS[name]
        self.x0, self.y0 = self.kx - WIN_W // 2, self.ky - WIN_H // 2
        self.shift = ps.shift_m(name, S)
        self.stats = dict.fromkeys(STAT_KEYS, 0)
        self.moved = 0

    def window(self, m):
        """the window's mirror; asserts that the ring of 8 cells around it was never touched"""
        md = m.window(self.x0, self.y0, WIN_W, WIN_H)
        assert not (0 <= md.origin[0] < WIN_W) and not (0 <= md.origin[1] < WIN_H), "the window's origin must lie outside it"
        wide = m.window(self.x0 - 8, self.y0 - 8, WIN_W + 16, WIN_H + 16)
        ring = np.ones(wide.payload.shape[:2], bool)
        ring[8:-8, 8:-8] = False
        assert (wide.payload[ring] == md.unknown[:md.payload.shape[2]]).all(), "touched cells outside the window"
        occupancy(md)
        return md

    def accepted(self, md, pose, angles, max_dist, thr):
        """the library's host routine on the window: no refusal, no status 2"""
        try:
            _, st = self.pkg.generate_scans_host(md, [pose], angles, max_dist, thr, 0, self.variant)
        except self.pkg.SlamHipError:
            return False
        return not np.any(st == 2)

    def settle(self, md, local, angles, max_dist, thr):
        """local pose (next to (0, 0)) -> a pose at the station every beam of which the reference will answer"""
        local = np.array(local, dtype=np.float64)
        for k in range(40):
            pose = local + [0.0011 * k, 0.0011 * k, 0.0] + self.shift
            if self.accepted(md, pose, angles, max_dist, thr):
                self.moved += k > 0
                return pose
        raise AssertionError("%s: no acceptable pose next to %r" % (self.name, local))


def run_call(stn, out, name, map_name, m, md, poses, max_dist, fov_deg, pts_nm, thr):
    R, stats = stn.R, stn.stats
    angles = angle_list(fov_deg, pts_nm)
    B = angles.size
    assert 37 <= B <= 90, B
    rng, status, step = np.zeros((3, B)), np.zeros((3, B), np.uint8), -np.ones((3, B), np.int64)
    w, h = WIN_W, WIN_H
    for k, p in enumerate(poses):
        assert stn.accepted(md, p, angles, max_dist, thr), "a pose the reference may refuse"
        r, a, o, _ = R.scan_generate(m, p, max_dist, fov_deg, pts_nm, thr).get()
        assert np.all(o == 1)
        idx = np.searchsorted(angles, a)
        assert np.array_equal(angles[idx], a), "a scan angle that is not in the accumulated list"
        rng[k, idx], status[k, idx] = r, 1
        rc = (math.floor(p[0] / md.scale), math.floor(p[1] / md.scale))
        if not (0 <= rc[0] + md.origin[0] < w and 0 <= rc[1] + md.origin[1] < h):
            stats["robot_outside"] += 1
        for b in range(B):
            ang = angles[b] + p[2]
            ex, ey = p[0] + max_dist * math.cos(ang), p[1] + max_dist * math.sin(ang)
            cells = R.world_to_cells(m, p[0], p[1], ex, ey)
            dx, dy = abs(int(cells[-1][0] - cells[0][0])), abs(int(cells[-1][1] - cells[0][1]))
            stats["max_cells"] = max(stats["max_cells"], len(cells))
            stats["short_walks"] += len(cells) < 64
            diag = int(np.sum((np.diff(cells[:, 0]) != 0) & (np.diff(cells[:, 1]) != 0)))
            astray = _walk_goes_astray(md.scale, p[0], p[1], ex, ey)
            stats["astray"] += bool(astray)
            stats["tie"] += (not astray) and diag > 0
            assert len(cells) == max(dx, dy) + 1 if astray else len(cells) >= dx + dy + 1 - diag
            ixs, iys = cells[:, 0] + md.origin[0], cells[:, 1] + md.origin[1]
            inside = (ixs >= 0) & (ixs < w) & (iys >= 0) & (iys < h)
            stats["leaves_window"] += bool(np.any(~inside))
            if status[k, b]:
                hx = math.floor((p[0] + rng[k, b] * math.cos(ang)) / md.scale)
                hy = math.floor((p[1] + rng[k, b] * math.sin(ang)) / md.scale)
                at = np.flatnonzero((cells[:, 0] == hx) & (cells[:, 1] == hy))
                if at.size != 1:
                    step[k, b] = -2
                    stats["unlocated"] += 1
                    continue
                step[k, b] = at[0]
                stats["hit_early"] += at[0] < 64
                stats["hit_late"] += at[0] >= 64
                occ = np.full(len(cells), md.unknown_occ)  # a candidate before the hit cell in the list was a touch
                occ[inside] = md.occ[iys[inside], ixs[inside]]
                stats["touch"] += bool(np.any(~(occ[:at[0]] < thr)))
            else:
                stats["no_hit"] += 1
    out.update({name + "_map": np.array(map_name), name + "_occ_kind": np.array(0), name + "_poses": np.asarray(poses, dtype=np.float64),
                name + "_lsp": np.array([max_dist, fov_deg, pts_nm], dtype=np.float64), name + "_threshold": np.array(thr),
                name + "_range": rng, name + "_status": status, name + "_hit_step": step})
    print("%-18s beams %3d hits %3d" % (name, 3 * B, int(status.sum())))
    return name


def put_map(out, name, md):
    out.update({name + "_payload": md.payload, name + "_origin": np.array(md.origin), name + "_scale": np.array(md.scale),
                name + "_unknown": np.asarray(md.unknown, dtype=np.float64), name + "_cell_model": np.array(md.cell_model)})


def find_astray_call(stn, md, pts_nm, fov_deg, thr):
    """make_golden_scan_generate.find_astray_call with every coordinate AT the station: a pose, heading and max_dist whose
    beam k ends a hair off a grid corner so that the walk goes astray -- and which the host routine accepts"""
    rs = np.random.RandomState(7)
    angles = angle_list(fov_deg, pts_nm)
    tiny = [1e-9, -1e-9, 1e-7, -1e-7, 3e-8, -3e-8, 1e-6, -1e-6, 1e-8, -1e-8]
    for _ in range(400000):
        x0 = (stn.kx + rs.randint(-20, 20) + 0.5) * S + rs.choice(tiny)
        y0 = (stn.ky + rs.randint(-15, 15) + 0.5) * S + rs.choice(tiny)
        tx = (stn.kx + rs.randint(-60, 60)) * S + rs.choice(tiny)
        ty = (stn.ky + rs.randint(-60, 60)) * S + rs.choice(tiny)
        k = rs.randint(angles.size)
        dist = math.hypot(tx - x0, ty - y0)
        th = math.atan2(ty - y0, tx - x0) - angles[k]
        ang = angles[k] + th
        if dist > 1.0 and _walk_goes_astray(S, x0, y0, x0 + dist * math.cos(ang), y0 + dist * math.sin(ang)):
            pose = np.array([x0, y0, th])
            if stn.accepted(md, pose, angles, dist, thr):
                return pose, dist
    raise AssertionError("no astray walk found at " + stn.name)


def find_touch_poses(stn, m, md, max_dist, fov_deg, pts_nm, thr):
    """make_golden_scan_generate.find_touch_poses at the station: poses with a beam whose list of cells holds an occupied
    cell BEFORE the one it hits -- the ray passes its corner so closely that the two edge intersections are are_equal"""
    rs = np.random.RandomState(11)
    angles = angle_list(fov_deg, pts_nm)
    found = []
    for _ in range(4000):
        x0 = (stn.kx + rs.randint(-10, 10) + 0.5) * S + rs.choice([3e-8, -3e-8, 5e-8, -5e-8, 0.0])
        y0 = (stn.ky + rs.randint(-8, 8) + 0.5) * S + rs.choice([3e-8, -3e-8, 5e-8, -5e-8])
        q, pp = rs.choice([1, 2, 3, -1, -2, -3]), rs.choice([1, 2, 3, -1, -2, -3])
        k = rs.randint(angles.size)
        pose = np.array([x0, y0, math.atan2(pp, q) - angles[k]])
        try:
            rng, st = stn.pkg.generate_scans_host(md, [pose], angles, max_dist, thr, 0, stn.variant)
        except stn.pkg.SlamHipError:
            continue
        if np.any(st == 2) or st[0, k] != 1:
            continue
        ang = angles[k] + pose[2]
        cells = stn.R.world_to_cells(m, x0, y0, x0 + max_dist * math.cos(ang), y0 + max_dist * math.sin(ang))
        hx = math.floor((x0 + rng[0, k] * math.cos(ang)) / S)
        hy = math.floor((y0 + rng[0, k] * math.sin(ang)) / S)
        at = np.flatnonzero((cells[:, 0] == hx) & (cells[:, 1] == hy))
        if at.size != 1:
            continue
        ixs, iys = cells[:at[0], 0] + md.origin[0], cells[:at[0], 1] + md.origin[1]
        inside = (ixs >= 0) & (ixs < WIN_W) & (iys >= 0) & (iys < WIN_H)
        occ = np.full(at[0], md.unknown_occ)
        occ[inside] = md.occ[iys[inside], ixs[inside]]
        if np.any(~(occ < thr)):
            found.append(pose)
            if len(found) == 3:
                return found
    raise AssertionError("no touch found at " + stn.name)


def main():
    if not po.ref_available():
        sys.exit("oracle/_ref/libslamref.so is not built (run __graft_entry__.build() where the reference tree is)")
    t0 = time.time()
    R = po.Ref()
    pkg = ge.load_package()
    variant = pkg.scan_gen_libm_variant()
    out = dict(libm_variant=np.array(pkg.libm_variant()), sincos_variant=np.array(variant), window=np.array([WIN_W, WIN_H]))
    calls, all_stats = [], {}
    a36 = angle_list(270, 36)
    for st in ps.Q_STATIONS:
        stn = Station(R, pkg, st, variant)
        pre = st + "_"
        # ---- the hand-made map: the cecum of scan_generate.npz, stamped at the station
        gt = R.map_create(po.REF_CELL_MOCK, po.MAP_UNBOUNDED_LAZY_TILED, WIN_W, WIN_H, S, 0.5)
        gt.stamp_text(R.cecum_text(25, 17, TOP), (stn.kx - 12, stn.ky + 12))
        g = gt.geometry()
        assert g["width"] > 9000 and g["height"] > 9000, "the map was expected to span back to (0, 0)"
        md = stn.window(gt)
        assert (md.occ >= 1.0).sum() > 40
        put_map(out, pre + "cecum", md)
        a89 = angle_list(270, 89)
        local = [[0.053, -0.348, 0.3], [0.6721, 0.9133, -2.1], [-7.137, 1.013, 0.05]]  # the last one: outside the window
        poses = [stn.settle(md, p, a89, 100.0, 1.0) for p in local]
        calls.append(run_call(stn, out, pre + "cecum_short", pre + "cecum", gt, md, poses, 2.0, 270, 36, 1.0))
        calls.append(run_call(stn, out, pre + "cecum_long", pre + "cecum", gt, md, poses, 100.0, 270, 89, 1.0))
        # ties: headings that send beams through grid vertices (slope 1/3 from a cell centre)
        c0 = np.array([(stn.kx + 0.5) * S, (stn.ky + 0.5) * S]), np.array([(stn.kx - 4 + 0.5) * S, (stn.ky + 2 + 0.5) * S])
        tie_poses = [np.array([c0[0][0], c0[0][1], math.atan2(1, 3) - a36[20]]), stn.settle(md, [0.0513, -0.4502, 0.2], a36, 0.7, 1.0),
                     np.array([c0[1][0], c0[1][1], math.atan2(1, 3) - a36[9]])]
        calls.append(run_call(stn, out, pre + "cecum_ties", pre + "cecum", gt, md, tie_poses, 0.7, 270, 36, 1.0))
        assert stn.stats["tie"] > 0, "no beam with a vertex tie"
        before = stn.stats["astray"]
        ap, adist = find_astray_call(stn, md, 36, 270, 1.0)
        others = [stn.settle(md, p, a36, adist, 1.0) for p in local[:2]]
        calls.append(run_call(stn, out, pre + "cecum_astray", pre + "cecum", gt, md, [ap] + others, adist, 270, 36, 1.0))
        assert stn.stats["astray"] > before, "the astray walk did not survive"
        tposes = find_touch_poses(stn, gt, md, 100.0, 270, 36, 1.0)
        calls.append(run_call(stn, out, pre + "cecum_touch", pre + "cecum", gt, md, tposes, 100.0, 270, 36, 1.0))
        # ---- SLAM-built maps of the cell classes the compiled reference harness builds
        a180 = angle_list(270, 180)
        built = [stn.settle(md, p, a180, 15.0, 1.0) for p in ([0.053, -0.348, 0.0], [0.253, -0.612, 0.8], [-0.33, -0.21, 2.0])]
        a60 = angle_list(270, 60)
        for tag, cell, thr in (("mean", po.REF_CELL_MEAN, 0.6), ("tbm", po.REF_CELL_TBM, 0.55), ("gmapping", po.REF_CELL_GMAPPING, 0.7)):
            m = R.map_create(cell, po.MAP_UNBOUNDED_LAZY_TILED, WIN_W, WIN_H, S, 0.5)
            for p in built:
                R.append_scan(m, R.scan_generate(gt, p, 15, 270, 180, 1.0), p, quality=0.9)
            mdm = stn.window(m)
            assert (mdm.payload != mdm.unknown[:mdm.payload.shape[2]]).any(axis=2).sum() > 100
            put_map(out, pre + tag, mdm)
            mposes = [stn.settle(mdm, p, a60, 8.0, thr) for p in local]
            calls.append(run_call(stn, out, pre + "slam_" + tag, pre + tag, m, mdm, mposes, 8.0, 270, 60, thr))
        s = stn.stats
        print(st, s, "poses moved off a refusal:", stn.moved)
        assert s["robot_outside"] > 0 and s["no_hit"] > 0 and s["hit_early"] > 0 and s["hit_late"] > 0, st
        assert s["short_walks"] > 0 and s["max_cells"] > 300 and s["leaves_window"] > 0 and s["tie"] > 0 and s["astray"] > 0, st
        assert s["touch"] > 0, st + ": no beam whose first candidate is a touch"
        all_stats[st] = s
        out[pre + "stats"] = np.array([s[k] for k in STAT_KEYS])
    out["calls"], out["stat_keys"] = np.array(calls), np.array(STAT_KEYS)
    path = os.path.join(GOLDEN_DIR, "placed_generate.npz")
    save_stable(path, out)
    size = os.path.getsize(path)
    assert size <= os.path.getsize(os.path.join(GOLDEN_DIR, "placed.npz")), "placed_generate.npz is larger than placed.npz"
    print("wrote placed_generate.npz %d KiB in %.0f s, peak resident set %.1f GB" %
          (size // 1024, time.time() - t0, resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1e6))


if __name__ == "__main__":
    main()
