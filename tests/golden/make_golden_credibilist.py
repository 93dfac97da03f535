#!/usr/bin/env python3
"""Generate tests/golden/credibilist.npz from the COMPILED REFERENCE: the CredibilistCell of
src/slams/credibilist/grid_cell.h through the reference's scan adder, scorers, matchers and world.

Runs only where the reference tree is present.  tests/golden/credibilist_harness.cpp (ours; it includes the unmodified
reference headers) is compiled with the reference's own flags, as oracle/Makefile does, into oracle/_ref/ (git-ignored);
the binary is never committed.  The fixture is data only: the inputs made here and what the reference computed.

    python tests/golden/make_golden_credibilist.py [path/to/reference]

Contents of credibilist.npz
  cells   cell_belief [n, 4], cell_prob [n] = 1 - discrepancy(scorer's observation), cell_occ [n]: random update
          sequences through CredibilistCell::operator+= (every step kept), a never-observed cell, and hand-made edges
          (vacuous, massless, pure masses, masses near 1e-300; edges have no occupancy: cell_occ is NaN there)
  scene   a 160 x 160 map at 0.05 m built by WallDistanceBlurringScanAdder from 3 scans of 97 beams: map_after [3, h, w, 4],
          the scans (map_pose, map_quality, map_cached, map_range), the scan adder's settings; a 4th scan to match
          (match_range, init_pose), its filtered form per trig provider ({raw,cached}_f_*), 64 poses (one with every end
          point outside the window) and the reference's estimate_scan_probability for them: {raw,cached}_{obstacle,max,
          mean,overlap}_scores
  traces  hc_* / mc_*: process_scan observer traces of HillClimbingScanMatcher(6, 0.1, 0.1) and MonteCarloScanMatcher
          (seeded, 100 attempts) on that scene with the cached provider
  world   5 scans through SingleStateHypothesisLaserScanGridWorld with init_credibilist_slam's qualities (0.9 / 0.6):
          world_odom, world_range, world_pose (after each scan), world_quality, world_final [h, w, 4]
"""
import os
import subprocess
import sys

import numpy as np

GOLDEN_DIR = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(GOLDEN_DIR))
REFERENCE = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("REFERENCE", "/root/reference")
OUT_DIR = os.path.join(ROOT, "oracle", "_ref")

N_BEAMS, FOV = 97, np.deg2rad(240.0)
MAP_W = MAP_H = 160
SCALE, BLUR = 0.05, 0.1
BASE = (0.95, 1.0, 0.01, 1.0)       # slam/occupancy_estimator defaults (utils/init_occupancy_mapping.h)
AREA = (-0.06, 0.06, -0.06, 0.06)   # sp_analysis_area of the window OOPEs: bot, top, left, right
HC = (6, 0.1, 0.1)
MC = (20261018, 0.2, 0.1, 100, 100)
# the room: outer walls and one pillar, as axis-aligned boxes (x0, y0, x1, y1); all of it inside the 8 m window
BOXES = [(-2.6, -2.1, 2.6, 2.3), (0.9, 0.7, 1.3, 1.2)]


def cast(pose, a_min, a_inc):
    """ranges of N_BEAMS beams from `pose` against BOXES (exact ray / segment intersections: every beam hits)"""
    out = np.zeros(N_BEAMS)
    for i in range(N_BEAMS):
        d = pose[2] + a_min + i * a_inc
        dx, dy = np.cos(d), np.sin(d)
        best = np.inf
        for (x0, y0, x1, y1) in BOXES:
            for (wx, lo, hi, vertical) in ((x0, y0, y1, True), (x1, y0, y1, True), (y0, x0, x1, False), (y1, x0, x1, False)):
                den = dx if vertical else dy
                if abs(den) < 1e-12:
                    continue
                t = (wx - (pose[0] if vertical else pose[1])) / den
                if t <= 1e-9:
                    continue
                other = (pose[1] + t * dy) if vertical else (pose[0] + t * dx)
                if lo <= other <= hi:
                    best = min(best, t)
        assert np.isfinite(best)
        out[i] = best
    return out


def build():
    os.makedirs(OUT_DIR, exist_ok=True)
    exe = os.path.join(OUT_DIR, "credibilist_harness")
    subprocess.check_call(["g++", "-std=c++14", "-O3", "-w", "-I" + os.path.join(REFERENCE, "src"), "-o", exe,
                           os.path.join(GOLDEN_DIR, "credibilist_harness.cpp")])
    return exe


def main():
    if not os.path.isdir(os.path.join(REFERENCE, "src", "slams", "credibilist")):
        sys.exit("reference tree not found at %s" % REFERENCE)
    exe = build()
    rs = np.random.RandomState(20261018)
    a_min, a_inc = -FOV / 2, FOV / (N_BEAMS - 1)
    inp = [N_BEAMS, a_min, a_inc, MAP_W, MAP_H, SCALE, BLUR, *BASE, *AREA]

    # cells
    n_cells, n_steps = 400, 8
    obs = np.empty((n_cells, n_steps, 3))
    obs[..., 0] = rs.choice([0.95, 0.01, 0.5, 0.0, 1.0], size=(n_cells, n_steps), p=[0.3, 0.4, 0.1, 0.1, 0.1])
    obs[..., 0] = np.where(rs.rand(n_cells, n_steps) < 0.3, rs.rand(n_cells, n_steps), obs[..., 0])
    obs[..., 1] = rs.choice([1.0, 0.7, 0.04, 0.0], size=(n_cells, n_steps), p=[0.6, 0.2, 0.1, 0.1])
    obs[..., 2] = rs.choice([0.9, 0.6, 1.0, 0.3], size=(n_cells, n_steps))
    inp += [n_cells, n_steps, *obs.ravel()]
    t = 1e-300
    edges = np.array([[1, 0, 0, 0], [0, 0, 0, 0], [0, 0, 1, 0], [0, 1, 0, 0], [0, 0, 0, 1],
                      [t, 0, 0, 0], [0, t, 0, 0], [0, 0, t, 0], [0, 0, 0, t], [t, t, t, t], [t, 0, t, 0], [0, t, 0, t],
                      [3 * t, t, 2 * t, 0], [1, 0, t, 0], [t, 0, 1, 0], [0.5, 0, 0.5, 0], [0.25, 0.25, 0.25, 0.25],
                      [5e-324, 0, 5e-324, 0], [5e-324, 0, 0, 0], [0.1, 0.2, 0.3, 0.4], [1e300, 0, 1e300, 0]], dtype=np.float64)
    inp += [len(edges), *edges.ravel()]

    # scene
    map_pose = np.array([[0.0, 0.0, 0.1], [0.3, -0.2, 0.6], [-0.4, 0.25, -0.5]])
    map_quality = np.array([0.6, 0.9, 0.9])
    map_cached = np.array([1, 1, 0])  # the last append with the raw provider (slamhip_map_append_scan_raw's golden)
    map_range = np.stack([cast(p, a_min, a_inc) for p in map_pose])
    inp += [len(map_pose)]
    for p, q, c, r in zip(map_pose, map_quality, map_cached, map_range):
        inp += [*p, q, c, *r]
    true_pose = np.array([0.15, 0.1, 0.25])
    init_pose = true_pose + [0.06, -0.05, 0.03]
    match_range = cast(true_pose, a_min, a_inc)
    n_poses = 64
    poses = init_pose + rs.randn(n_poses, 3) * [0.1, 0.1, 0.05]
    poses[0] = poses[1] = init_pose
    poses[2] = [400.0, 400.0, 0.3]  # every end point outside the window: the prototype cell
    inp += [*init_pose, *match_range, n_poses, *poses.ravel(), *HC, *MC]

    # world
    n_world = 5
    wtrue = np.array([[0.0, 0.0, 0.0], [0.12, 0.05, 0.08], [0.25, 0.02, 0.2], [0.3, -0.1, 0.35], [0.2, -0.22, 0.5]])
    world_odom = np.diff(np.vstack([[0.0, 0.0, 0.0], wtrue]), axis=0)
    world_odom[1:] += rs.randn(n_world - 1, 3) * [0.04, 0.04, 0.02]
    world_odom[3] = np.diff(wtrue, axis=0)[2]  # one exact odometry step
    world_range = np.stack([cast(p, a_min, a_inc) for p in wtrue])
    inp += [n_world]
    for o, r in zip(world_odom, world_range):
        inp += [*o, *r]

    f_in, f_out = os.path.join(OUT_DIR, "credibilist_in.bin"), os.path.join(OUT_DIR, "credibilist_out.bin")
    np.asarray(inp, dtype=np.float64).tofile(f_in)
    subprocess.check_call([exe, f_in, f_out])
    o = np.fromfile(f_out, dtype=np.float64)
    pos = [0]

    def take(n, shape=None):
        v = o[pos[0]:pos[0] + n]
        assert v.size == n
        pos[0] += n
        return v.reshape(shape) if shape else v

    def take_map():
        w, h, ox, oy = [int(v) for v in take(4)]
        assert (w, h, ox, oy) == (MAP_W, MAP_H, MAP_W // 2, MAP_H // 2), "the map grew: keep the room inside the window"
        return take(w * h * 4, (h, w, 4))

    out = dict(n_beams=np.array(N_BEAMS), a_min=np.array(a_min), a_inc=np.array(a_inc),
               a_max_passed=np.array(a_min + (N_BEAMS - 1) * a_inc + 2 * a_inc), map_scale=np.array(SCALE),
               map_origin=np.array([MAP_W // 2, MAP_H // 2]), blur=np.array(BLUR), base=np.array(BASE), area=np.array(AREA))
    c = take(n_cells * n_steps * 6, (n_cells * n_steps, 6))
    e = take(len(edges))
    fresh = take(6)
    out["cell_belief"] = np.vstack([c[:, :4], fresh[None, :4], edges])
    out["cell_prob"] = np.concatenate([c[:, 4], fresh[4:5], e])
    out["cell_occ"] = np.concatenate([c[:, 5], fresh[5:6], np.full(len(edges), np.nan)])
    out["cell_obs"] = obs
    out.update(map_pose=map_pose, map_quality=map_quality, map_cached=map_cached, map_range=map_range,
               map_after=np.stack([take_map() for _ in map_pose]))
    out.update(init_pose=init_pose, true_pose=true_pose, match_range=match_range, poses=poses)
    for trig in ("raw", "cached"):
        n = int(take(1)[0])
        for k in ("range", "angle", "factor", "weight"):
            out["%s_f_%s" % (trig, k)] = take(n)
        for k in ("obstacle", "max", "mean", "overlap"):
            out["%s_%s_scores" % (trig, k)] = take(n_poses)
    for name, prm in (("hc", HC), ("mc", MC)):
        n = int(take(1)[0])
        res = take(4)
        out.update({name + "_params": np.array(prm, dtype=np.float64), name + "_n_calls": np.array(n),
                    name + "_prob": np.array(res[0]), name + "_delta": res[1:].copy(), name + "_poses": take(3 * n, (n, 3)),
                    name + "_scores": take(n), name + "_accepted": take(n).astype(np.int32)})
    wp = take(4 * n_world, (n_world, 4))
    out.update(world_odom=world_odom, world_range=world_range, world_pose=wp[:, :3].copy(), world_quality=wp[:, 3].copy(),
               world_final=take_map())
    assert pos[0] == o.size
    path = os.path.join(GOLDEN_DIR, "credibilist.npz")
    np.savez_compressed(path, **out)
    print("wrote credibilist.npz", os.path.getsize(path) // 1024, "KiB")
    print("hc calls", int(out["hc_n_calls"]), "accepted", int(out["hc_accepted"].sum()), "mc calls", int(out["mc_n_calls"]),
          "accepted", int(out["mc_accepted"].sum()), "world qualities", out["world_quality"],
          "scores", out["cached_obstacle_scores"][:4], "filtered", out["cached_f_range"].size, out["raw_f_range"].size)


if __name__ == "__main__":
    main()
