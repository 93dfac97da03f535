#!/usr/bin/env python3
"""Generate tests/golden/m3rsm_rawtrig.npz from the COMPILED REFERENCE: whole matches of
BruteForceMultiResolutionScanMatcher with the scan under the reference's DEFAULT trig provider, RawTrigonometryProvider
(src/core/trigonometry_utils.h:17-35: std::cos / std::sin(base + a) per beam; use_trig_cache = false), with the full
trace of scorer calls -- what SLAMHIP_POSE_TRIG_RAW_EXACT of the BF_M3RSM matcher is held to, bit for bit.

Runs only where the reference tree is present.  tests/golden/m3rsm_rawtrig_harness.cpp (ours; it includes the unmodified
reference headers; m3rsm_harness.cpp with the raw provider) is compiled with the reference's own flags into oracle/_ref/
(git-ignored); the binary is never committed.  The fixture is data only: the inputs made here and what the reference
computed.  Scene makers and checks are make_golden_m3rsm.py's, imported.

    python tests/golden/make_golden_m3rsm_rawtrig.py [path/to/reference]

Scenes (all: MaxOccupancyObservationPE, EvenSPW):
  occ_square, occ_1beam, tbm_square, cred_square   the shapes of m3rsm.npz
  edge_occ, edge_tbm   EDGE scenes, the recipe of the reference's HC smoke fixture: a 33x33 map at 0.125 (cell edges are
      exact doubles), the robot on a cell centre, ranges odd multiples of 1/16 (so the end point of a beam along an
      axis lies exactly on a cell edge), beam angles multiples of 1/32 and heading and rotation step multiples of 1/64
      (so heading + rotation + angle is exactly 0 for a beam of every other rotation: the raw provider's direction is
      (1, 0) there, the cached provider's angle addition is a last place off, and floor() picks another cell); limits
      0.5 m at step 1/16, so windows' rims lie on cell edges too.

Asserted here (the fixture is not written otherwise):
  * what make_golden_m3rsm.py asserts whatever the provider: validate() is true and the levels are the tight ones;
    every call is a root or a child of an earlier call at its rotation by the rule of include/slamhip.h "EXPAND"; a run
    of the engine with prerotate_scan = false gives the same trace bit for bit; at most 4500 calls per scene; every
    level follows from its rectangle;
  * each edge scene has at least one call whose score differs BITWISE between the raw run and the run of the same
    binary under CachedTrigonometryProvider (compared call by call over the common prefix of equal rotation and
    rectangle); over the file at least 10 such calls, and in at least one scene another number of calls or another delta.

Contents: n_scenes, libm_variant (of the generating host: 1 = glibc's FMA build, 0 = the plain one); per scene s<i>_ what
m3rsm.npz holds -- name, cls, model, oie, scale, origin, unknown, payload, pose, scan [n, 5] (range, cos a, sin a, weight,
factor; cos / sin = libm's of the angle), limits, delta, prob, trace [n_calls, 7] --, angle [n], trig (a_min, a_max,
a_inc: the cached provider's table), edge (0 / 1), delta_cached, prob_cached, trace_cached.
"""
import io
import os
import subprocess
import sys
import zipfile

import numpy as np

GOLDEN_DIR = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, GOLDEN_DIR)
import make_golden_m3rsm as base  # noqa: E402

ROOT, REFERENCE, OUT_DIR, MAX_CALLS, DEG = base.ROOT, base.REFERENCE, base.OUT_DIR, base.MAX_CALLS, base.DEG
SEED = int(os.environ.get("M3RSM_RAWTRIG_SEED", "20261019"))
SMALL = ["occ_square", "occ_1beam", "tbm_square", "cred_square"]
# name, class, pose (a cell centre, heading k / 64), true pose - pose, a_min, beams, limits
EDGE = [
    ("edge_occ", "occ", (0.1875, -0.0625, 0.25), (0.125, -0.0625, 2 / 64), -1.5, 67, (0.5, 0.5, 5 / 64, 1 / 64, 1 / 16)),
    ("edge_tbm", "tbm", (-0.0625, 0.1875, -0.5), (-0.0625, 0.125, -2 / 64), -1.0, 67, (0.5, 0.25, 4 / 64, 1 / 64, 1 / 16)),
]


def build():
    os.makedirs(OUT_DIR, exist_ok=True)
    exe = os.path.join(OUT_DIR, "m3rsm_rawtrig_harness")
    subprocess.check_call(["g++", "-std=c++14", "-O3", "-w", "-I" + os.path.join(REFERENCE, "src"), "-o", exe,
                           os.path.join(GOLDEN_DIR, "m3rsm_rawtrig_harness.cpp")])
    return exe


def edge_scan(rs, n, a_min, true_pose, w, h, origin, scale):
    """n beams at a_min + i / 32 from `true_pose` to the middle of the room's walls, the ranges snapped to odd multiples
    of 1 / 16 (a cell centre + such a range along an axis is a cell edge), a few of them a cell off"""
    x0, x1, y0, y1 = base.room(w, h, origin)
    lo = np.array([(x0 + 0.5) * scale, (y0 + 0.5) * scale])
    hi = np.array([(x1 + 0.5) * scale, (y1 + 0.5) * scale])
    a_inc = 1 / 32
    angles = a_min + a_inc * np.arange(n)
    ranges = np.zeros(n)
    for i, a in enumerate(angles):
        d = np.array([np.cos(true_pose[2] + a), np.sin(true_pose[2] + a)])
        t = [((hi[k] if d[k] > 0 else lo[k]) - true_pose[k]) / d[k] for k in range(2) if abs(d[k]) > 1e-12]
        r = min(v for v in t if v > 0) + scale * int(rs.randint(-1, 2)) * (rs.rand() < 0.15)
        ranges[i] = (2 * np.round((r * 16 - 1) / 2) + 1) / 16
    return ranges, angles, a_min, a_min + (n + 0.5) * a_inc, a_inc


def write_npz(path, out):
    """np.savez_compressed with the members in sorted order and a fixed time stamp: the same bytes from the same data"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for key in sorted(out):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(out[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def libm_variant():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    return int(ge.load_package().libm_variant())


def rotations_of(rec, rot_roots):
    """the rotation of every call of a prerotated run: the scan it was scored with, known from the root layer"""
    by_scan = {}
    for j in range(len(rot_roots)):
        by_scan.setdefault(rec[j, 9:11].tobytes(), rot_roots[j])
        assert by_scan[rec[j, 9:11].tobytes()] == rot_roots[j], "two rotations with the same first point"
    return np.array([by_scan[rec[j, 9:11].tobytes()] for j in range(len(rec))])


def n_bitwise_different(trace, other):
    """calls of the common prefix of equal (rotation, rectangle) whose scores differ bitwise"""
    n = min(len(trace), len(other))
    same = np.all(trace[:n, :5].view(np.int64) == other[:n, :5].view(np.int64), axis=1)
    k = n if same.all() else int(np.argmin(same))
    return int(np.sum(trace[:k, 5].view(np.int64) != other[:k, 5].view(np.int64)))


def make_scenes(small=SMALL, edge=EDGE, shift=(0, 0)):
    """the scenes named in `small` and the edge scenes `edge`, the whole scene moved by `shift` cells
    (make_golden_placed_pyramid.py: a station; an edge scene stays one: a shift of whole 0.125 m cells is an exact double)"""
    scenes = []
    for k, (name, cls, (w, h, origin), scale, n_beams, limits) in enumerate(s for s in base.SCENES if s[0] in small):
        rs = np.random.RandomState(SEED + k)
        cid, model, stride = base.CLASSES[cls]
        o = origin or (w // 2, h // 2)
        o = (o[0] - shift[0], o[1] - shift[1])
        obs = base.observations(np.random.RandomState(SEED + 100 + k), cid, w, h, o)
        x0, x1, y0, y1 = base.room(w, h, o)
        mid = np.array([(x0 + x1 + 1) / 2 * scale, (y0 + y1 + 1) / 2 * scale])
        pose = np.array([mid[0] + (0.3 + 0.4 * rs.rand()) * scale, mid[1] + (-0.2 + 0.4 * rs.rand()) * scale, 0.3 * rs.randn()])
        true_pose = pose + np.array([0.13, -0.09, 2.2 * DEG])
        ranges, angles, a_min, a_max, a_inc = base.cast_scan(rs, n_beams, true_pose, w, h, o, scale)
        scenes.append(dict(name=name, cls=cls, cid=cid, model=model, stride=stride, oie=0, w=w, h=h, origin=o, scale=scale, obs=obs,
                           pose=pose, ranges=ranges, angles=angles, trig=(a_min, a_max, a_inc), limits=limits, edge=0))
    for k, (name, cls, pose, off, a_min, n_beams, limits) in enumerate(edge):
        rs = np.random.RandomState(SEED + 50 + k)
        cid, model, stride = base.CLASSES[cls]
        w, h, o, scale = 33, 33, (16 - shift[0], 16 - shift[1]), 0.125
        obs = base.observations(np.random.RandomState(SEED + 150 + k), cid, w, h, o)
        pose = np.array(pose, dtype=np.float64) + [shift[0] * scale, shift[1] * scale, 0.0]
        assert np.all(np.round(pose[:2] * 16) == pose[:2] * 16) and np.all(np.round(pose[:2] * 16) % 2 == 1), "not a cell centre"
        ranges, angles, a_min, a_max, a_inc = edge_scan(rs, n_beams, a_min, pose + np.array(off), w, h, o, scale)
        t = pose[2] + np.arange(-8, 9) / 64
        assert np.any((t[:, None] + angles[None, :]) == 0.0), "no beam along the x axis at any rotation"
        scenes.append(dict(name=name, cls=cls, cid=cid, model=model, stride=stride, oie=0, w=w, h=h, origin=o, scale=scale, obs=obs,
                           pose=pose, ranges=ranges, angles=angles, trig=(a_min, a_max, a_inc), limits=limits, edge=1))
    return scenes


def run(exe, scenes, variant, tag="m3rsm_rawtrig"):
    """the harness over `scenes`: every per-scene assertion of this generator, then the fixture's arrays, the number of
    scores that differ bitwise between the providers and the scenes in which the provider moves the match"""
    inp = [len(scenes)]
    for m in scenes:
        inp += [m["cid"], m["oie"], m["w"], m["h"], m["scale"], m["origin"][0], m["origin"][1], len(m["obs"]), *m["obs"].ravel(),
                *m["pose"], len(m["ranges"]), *m["ranges"], *m["angles"], *m["trig"], *m["limits"]]
    f_in, f_out = os.path.join(OUT_DIR, tag + "_in.bin"), os.path.join(OUT_DIR, tag + "_out.bin")
    np.asarray(inp, dtype=np.float64).tofile(f_in)
    subprocess.check_call([exe, f_in, f_out])
    o = np.fromfile(f_out, dtype=np.float64)
    pos = [0]

    def take(n, shape=None):
        v = o[pos[0]:pos[0] + n]
        assert v.size == n
        pos[0] += n
        return v.reshape(shape).copy() if shape else v.copy()

    out = {"n_scenes": np.array(len(scenes)), "libm_variant": np.array(variant)}
    n_diff_all, moved = 0, []
    for i, m in enumerate(scenes):
        pre, stride = "s%d_" % i, m["stride"]
        n_scales, valid = (int(v) for v in take(2))
        assert valid == 1, "validate() is false for scene %s" % m["name"]
        proto = take(stride)
        levels = []
        for k in range(n_scales):
            lw, lh, ox, oy = (int(v) for v in take(4))
            sc = float(take(1)[0])
            cells = take(lw * lh * (stride + 2), (lh, lw, stride + 2))
            levels.append(dict(w=lw, h=lh, origin=(ox, oy), scale=sc, payload=cells[..., :stride], unknown=cells[..., stride] != 0,
                               impact=cells[..., stride + 1]))
        base.check_levels(m, levels, proto)
        n = int(take(1)[0])
        assert n == len(m["ranges"]), "filter_scan dropped a point"
        scan6 = take(6 * n, (n, 6))
        scan, angle = scan6[:, :5].copy(), scan6[:, 5].copy()
        assert np.array_equal(angle, m["angles"]) and np.array_equal(scan[:, 0], m["ranges"])
        # rows: pose x, y, theta, bot, top, left, right, value, scale_id, first point x, y
        res_a = take(4)
        rec_a = take(int(take(1)[0]) * 11).reshape(-1, 11)
        res_b = take(4)
        rec_b = take(int(take(1)[0]) * 11).reshape(-1, 11)
        res_d = take(4)
        rec_d = take(int(take(1)[0]) * 11).reshape(-1, 11)
        n_calls = len(rec_a)
        assert n_calls <= MAX_CALLS and len(rec_d) <= MAX_CALLS, "%s: %d / %d calls" % (m["name"], n_calls, len(rec_d))
        assert np.all(np.isfinite(rec_a[:, 7])) and np.all(np.isfinite(res_a))
        rot_roots, rect_roots = base.root_candidates(m["limits"])
        nr = len(rot_roots)
        traces = []
        for rec in (rec_a, rec_d):
            assert np.array_equal(rec[:nr, 3:7], rect_roots), "the root layer is not the one m3rsm_root_candidates gives"
            rot = rotations_of(rec, rot_roots)
            rect = rec[:, 3:7]
            assert np.all(rec[:, 2] == 0), "the run is not prerotated"
            assert np.array_equal(m["pose"][0] + (rect[:, 2] + (rect[:, 3] - rect[:, 2]) / 2), rec[:, 0])
            assert np.array_equal(m["pose"][1] + (rect[:, 0] + (rect[:, 1] - rect[:, 0]) / 2), rec[:, 1])
            traces.append(np.column_stack([rot, rect, rec[:, 7], rec[:, 8]]))
        trace, trace_cached = traces
        rot, rect = trace[:, 0], trace[:, 1:5]
        # run B, not prerotated: the same trace bit for bit, at headings base + rotation
        assert len(rec_b) == n_calls, "%s: the non-prerotated run makes %d calls, not %d" % (m["name"], len(rec_b), n_calls)
        assert np.array_equal(rec_a[:, [0, 1, 3, 4, 5, 6, 7, 8]].view(np.int64), rec_b[:, [0, 1, 3, 4, 5, 6, 7, 8]].view(np.int64))
        assert np.array_equal(m["pose"][2] + rot, rec_b[:, 2]), "a heading of run B is not base + rotation"
        assert np.array_equal(res_a.view(np.int64), res_b.view(np.int64))
        # the trace follows the rules
        step = np.float64(m["limits"][4])
        allowed = {base.key(rot_roots[j], rect_roots[j]) for j in range(nr)}
        for j in range(n_calls):
            assert base.key(rot[j], rect[j]) in allowed, "%s: call %d is no root and no child of an earlier call" % (m["name"], j)
            for kid in base.children(rect[j], step)[1]:
                allowed.add(base.key(rot[j], kid))
        lv_scale = np.array([lv["scale"] for lv in levels])
        side = np.maximum(rect[:, 1] - rect[:, 0], rect[:, 3] - rect[:, 2])
        assert np.array_equal(rec_a[:, 8], [int(np.argmax(t <= lv_scale)) for t in side])
        win = np.nonzero((rect[:, 0] == rect[:, 1]) & (rect[:, 2] == rect[:, 3]) & (rect[:, 2] == res_a[0]) & (rect[:, 0] == res_a[1])
                         & (rot == res_a[2]))[0]
        assert len(win) and np.any(rec_a[win, 7] == res_a[3])
        # raw against cached
        n_diff = n_bitwise_different(trace, trace_cached)
        n_diff_all += n_diff
        if len(trace) != len(trace_cached) or not np.array_equal(res_a[:3], res_d[:3]):
            moved.append(m["name"])
        assert not m["edge"] or n_diff >= 1, "%s: the raw and the cached provider give the same scores" % m["name"]
        out.update({pre + "name": np.array(m["name"]), pre + "cls": np.array(m["cls"]), pre + "model": np.array(m["model"]),
                    pre + "oie": np.array(m["oie"]), pre + "scale": np.array(m["scale"]), pre + "origin": np.array(m["origin"]),
                    pre + "unknown": proto, pre + "payload": levels[0]["payload"], pre + "pose": m["pose"], pre + "scan": scan,
                    pre + "angle": angle, pre + "trig": np.array(m["trig"]), pre + "edge": np.array(m["edge"]),
                    pre + "limits": np.array(m["limits"]), pre + "delta": res_a[:3], pre + "prob": np.array(res_a[3]),
                    pre + "trace": trace, pre + "delta_cached": res_d[:3], pre + "prob_cached": np.array(res_d[3]),
                    pre + "trace_cached": trace_cached})
        print("%-12s %5d calls (cached %5d), %4d scores differ bitwise, delta (%+.4f, %+.4f, %+.5f) (cached (%+.4f, %+.4f, %+.5f)), "
              "prob %.6f" % (m["name"], n_calls, len(rec_d), n_diff, *res_a[:3], *res_d[:3], res_a[3]))
    assert pos[0] == o.size
    if tag != "m3rsm_rawtrig":  # (a run for another fixture: the dense levels written out whole are large)
        os.remove(f_in), os.remove(f_out)
    return out, n_diff_all, moved


def main():
    if not os.path.isfile(os.path.join(REFERENCE, "src", "core", "scan_matchers", "bf_multi_res_scan_matcher.h")):
        sys.exit("reference tree not found at %s" % REFERENCE)
    variant = libm_variant()
    assert variant in (0, 1), "this host's libm is neither build of glibc's sin / cos"
    exe = build()
    scenes = make_scenes()
    out, n_diff_all, moved = run(exe, scenes, variant)
    assert n_diff_all >= 10, "hardly a call that tells the providers apart (%d)" % n_diff_all
    assert moved, "no scene in which the provider changes the number of calls or the delta"
    path = os.path.join(GOLDEN_DIR, "m3rsm_rawtrig.npz")
    write_npz(path, out)
    size = os.path.getsize(path)
    assert size <= 930 * 1024, "the fixture is larger than the bound make_golden_m3rsm.py holds its own to (%d bytes)" % size
    print("wrote m3rsm_rawtrig.npz: %d scenes, libm variant %d, %d bitwise different scores, provider moves the match in %s, %d KiB"
          % (len(scenes), variant, n_diff_all, moved, size // 1024))


if __name__ == "__main__":
    main()
