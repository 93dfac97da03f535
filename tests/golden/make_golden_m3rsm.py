#!/usr/bin/env python3
"""Generate tests/golden/m3rsm.npz from the COMPILED REFERENCE: whole matches of BruteForceMultiResolutionScanMatcher
(src/core/scan_matchers/bf_multi_res_scan_matcher.h) over M3RSMRescalableGridMap<UnboundedPlainGridMap>, with the full
trace of scorer calls the reference's M3RSMEngine (m3rsm_engine.h:252-365) makes.

Runs only where the reference tree is present.  tests/golden/m3rsm_harness.cpp (ours; it includes the unmodified
reference headers) is compiled with the reference's own flags into oracle/_ref/ (git-ignored); the binary is never
committed.  The fixture is data only: the inputs made here and what the reference computed.

    python tests/golden/make_golden_m3rsm.py [path/to/reference]

Scenes (all: MaxOccupancyObservationPE, EvenSPW, the cached trig provider; a square room drawn into the map -- walls of
high occupancy, a floor of low occupancy with about a quarter of it never observed -- and a scan cast from inside it):
  occ_square   GridCell 33x33 at 0.1, 67 beams, limits +-0.4 m, +-0.4 m, +-5 deg at 1 deg, step 0.05
  occ_oblong   the same map, limits +-0.4 m in x and +-0.2 m in y: one-sided splits
  occ_step07   step 0.07 over +-0.3 / +-0.45: a step that does not divide the range
  occ_1beam    a 1-beam scan on the 37x29 map with origin (11, 20) at 0.05
  tbm_square, cred_square   TbmOccConsistentCell and CredibilistCell under the discrepancy OIE

Asserted here (the fixture is not written otherwise):
  * validate() of the reference is true, and its levels are the tight ones: the checks of make_golden_pyramid.py (every
    cell is updated at most upward);
  * every recorded rectangle is a root or the split / point child of an earlier call at the same rotation, by the rule
    of include/slamhip.h "EXPAND";
  * a second run of the reference's engine with prerotate_scan = false gives the same trace bit for bit (values,
    rectangles, levels, poses), its headings being base heading + rotation;
  * a third run with every score multiplied by 1 +- 1e-12 gives the same delta and the same number of calls;
  * every scene has at most 4500 calls; over all scenes the trace holds >= 10 one-sided splits, >= 50 five-point
    expansions and calls on >= 4 levels.

Contents: n_scenes; per scene s<i>_: name, cls, model, oie, scale, origin, unknown [stride], payload [h, w, stride],
pose, scan [n, 5] (range, cos a, sin a, weight, factor), limits (max_x, max_y, max_th, rotation step, translation step),
delta [3], prob, trace [n_calls, 7] (rotation, bot, top, left, right, score, level).
"""
import os
import subprocess
import sys

import numpy as np

GOLDEN_DIR = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(GOLDEN_DIR))
REFERENCE = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("REFERENCE", "/root/reference")
OUT_DIR = os.path.join(ROOT, "oracle", "_ref")
MAX_CALLS = 4500
SEED = int(os.environ.get("M3RSM_SEED", "20261019"))
EPS = 2.220446049250313e-16

# name, harness class id, SLAMHIP_CELL_* model, stride
CLASSES = {"occ": (0, 0, 1), "tbm": (1, 1, 4), "cred": (2, 3, 4)}
DEG = np.pi / 180
# name, class, (w, h, origin or None), scale, beams, (max_x, max_y, max_th, rotation step, translation step)
SCENES = [
    ("occ_square", "occ", (33, 33, None), 0.1, 67, (0.4, 0.4, 5 * DEG, 1 * DEG, 0.05)),
    ("occ_oblong", "occ", (33, 33, None), 0.1, 67, (0.4, 0.2, 5 * DEG, 1 * DEG, 0.05)),
    ("occ_step07", "occ", (33, 33, None), 0.1, 67, (0.3, 0.45, 5 * DEG, 1 * DEG, 0.07)),
    ("occ_1beam", "occ", (37, 29, (11, 20)), 0.05, 1, (0.4, 0.4, 5 * DEG, 1 * DEG, 0.05)),
    ("tbm_square", "tbm", (33, 33, None), 0.1, 67, (0.4, 0.4, 5 * DEG, 1 * DEG, 0.05)),
    ("cred_square", "cred", (33, 33, None), 0.1, 67, (0.4, 0.4, 5 * DEG, 1 * DEG, 0.05)),
]


def build():
    os.makedirs(OUT_DIR, exist_ok=True)
    exe = os.path.join(OUT_DIR, "m3rsm_harness")
    subprocess.check_call(["g++", "-std=c++14", "-O3", "-w", "-I" + os.path.join(REFERENCE, "src"), "-o", exe,
                           os.path.join(GOLDEN_DIR, "m3rsm_harness.cpp")])
    return exe


def room(w, h, origin):
    """the wall ring of the room in external cells: [x0, x1] x [y0, y1], three cells inside the map's rim"""
    return 3 - origin[0], w - 4 - origin[0], 3 - origin[1], h - 4 - origin[1]


def observations(rs, cid, w, h, origin):
    """x, y, is_occ, prob, est_quality, quality per update, in the order they are applied: the cell that decides the
    number of levels first, then walls and floor in a seeded random order, then a second pass that raises some cells"""
    x0, x1, y0, y1 = room(w, h, origin)
    cells = [(x - origin[0], y - origin[1]) for y in range(h) for x in range(w)]
    far = max(cells, key=lambda c: (abs(c[0]) + abs(c[1]), c))

    def is_wall(c):
        on_x = c[0] in (x0, x1) and y0 <= c[1] <= y1
        on_y = c[1] in (y0, y1) and x0 <= c[0] <= x1
        return on_x or on_y

    chosen = [c for c in cells if c != far and (is_wall(c) or rs.rand() >= 0.25)]
    order = [far] + [chosen[i] for i in rs.permutation(len(chosen))]
    obs, first = [], {}
    for c in order:
        wall = is_wall(c)
        if cid == 0:
            k = int(rs.choice(range(840, 1000, 8))) if wall else int(rs.choice(range(8, 240, 8)))
            first[c] = k
            obs.append([c[0], c[1], float(k > 512), k / 1024.0, 1.0, 1.0])
        else:
            prob = float(rs.choice([0.8, 0.95])) if wall else float(rs.choice([0.05, 0.2, 0.35]))
            obs.append([c[0], c[1], float(prob > 0.5), prob, float(rs.choice([1.0, 0.7])), float(rs.choice([0.9, 0.6]))])
    for c in order:  # the second pass raises about a fifth of them
        if rs.rand() >= 0.2:
            continue
        if cid == 0:
            obs.append([c[0], c[1], 1.0, (first[c] + 4 + 8 * int(rs.randint(0, 3))) / 1024.0, 1.0, 1.0])
        else:
            obs.append([c[0], c[1], 1.0, 0.97, 1.0, 0.9])
    return np.asarray(obs, dtype=np.float64)


def cast_scan(rs, n, pose, w, h, origin, scale):
    """n beams from `pose` to the middle of the room's walls (a little noise on the ranges)"""
    x0, x1, y0, y1 = room(w, h, origin)
    lo = np.array([(x0 + 0.5) * scale, (y0 + 0.5) * scale])
    hi = np.array([(x1 + 0.5) * scale, (y1 + 0.5) * scale])
    a_inc = 2 * np.pi / 90
    a_min = -np.pi / 2
    angles = a_min + a_inc * np.arange(n)
    ranges = np.zeros(n)
    for i, a in enumerate(angles):
        d = np.array([np.cos(pose[2] + a), np.sin(pose[2] + a)])
        t = [((hi[k] if d[k] > 0 else lo[k]) - pose[k]) / d[k] for k in range(2) if abs(d[k]) > 1e-12]
        ranges[i] = min(v for v in t if v > 0) + 0.2 * scale * rs.randn()
    return ranges, angles, a_min, a_min + (n + 0.5) * a_inc, a_inc


def check_levels(m, levels, proto):
    """make_golden_pyramid.py's checks: the reference's levels are the tight ones"""
    stride, n_scales = m["stride"], len(levels)
    fine = levels[0]
    assert (fine["w"], fine["h"], fine["origin"]) == (m["w"], m["h"], tuple(m["origin"])), "the fine map grew"
    assert fine["scale"] == m["scale"] and np.isinf(levels[-1]["scale"]) and (levels[-1]["w"], levels[-1]["h"]) == (1, 1)
    updated = np.zeros((m["h"], m["w"]), bool)
    updated[(m["obs"][:, 1] + m["origin"][1]).astype(int), (m["obs"][:, 0] + m["origin"][0]).astype(int)] = True
    same_as_proto = np.all(fine["payload"].view(np.int64) == proto.view(np.int64), axis=-1)
    assert np.array_equal(fine["unknown"], ~updated) and np.array_equal(same_as_proto, ~updated), "a cell equals the prototype"
    fy, fx = np.nonzero(updated)
    ex, ey = fx - m["origin"][0], fy - m["origin"][1]
    f_imp, f_pay = fine["impact"][fy, fx], fine["payload"][fy, fx]
    for k in range(1, n_scales):
        lv = levels[k]
        top = k == n_scales - 1
        if not top:
            assert lv["scale"] == levels[k - 1]["scale"] * 2
        bx, by = (np.zeros_like(ex), np.zeros_like(ey)) if top else (ex >> k, ey >> k)
        seen = np.zeros((lv["h"], lv["w"]), bool)
        for X, Y in sorted(set(zip(bx.tolist(), by.tolist()))):
            ix, iy = X + lv["origin"][0], Y + lv["origin"][1]
            assert 0 <= ix < lv["w"] and 0 <= iy < lv["h"], "a block outside the reference's level window"
            sel = (bx == X) & (by == Y)
            imp = np.sort(np.unique(f_imp[sel]))
            assert np.all(np.diff(imp) > 1e-6), "two impacts of a block closer than 1e-6"
            best = f_imp[sel] == imp[-1]
            pays = f_pay[sel][best].view(np.int64)
            assert np.all(pays == pays[0]), "equal maximal impacts with different payloads"
            assert not lv["unknown"][iy, ix] and lv["impact"][iy, ix] == imp[-1], "a level cell is not the block's maximum"
            assert np.array_equal(lv["payload"][iy, ix].view(np.int64), pays[0])
            seen[iy, ix] = True
        assert np.array_equal(lv["unknown"], ~seen), "a level cell without a known fine cell is known"
        assert np.all(lv["payload"][~seen].view(np.int64) == proto.view(np.int64))
    k_built = 0
    while max(m["origin"][0], m["w"] - m["origin"][0], m["origin"][1], m["h"] - m["origin"][1]) > 2 ** k_built:
        k_built += 1
    assert n_scales == k_built + 2, "the level list is not the one the rule gives"


def children(rect, step):
    """the refinement rule of include/slamhip.h "EXPAND" in numpy doubles: (kind, [rects])"""
    bot, top, left, right = (np.float64(v) for v in rect)
    hside, vside = right - left, top - bot
    hb, vb = step < hside + EPS, step < vside + EPS
    cx, cy = left + hside / 2, bot + vside / 2
    if hb and vb:
        return "split4", [(bot, cy, left, cx), (cy, top, left, cx), (bot, cy, cx, right), (cy, top, cx, right)]
    if hb:
        return "split2", [(bot, top, left, cx), (bot, top, cx, right)]
    if vb:
        return "split2", [(bot, cy, left, right), (cy, top, left, right)]
    if hside + vside <= 0:
        return "point", []
    return "points5", [(bot, bot, left, left), (top, top, left, left), (bot, bot, right, right), (top, top, right, right),
                       (cy, cy, cx, cx)]


def key(rot, rect):
    return np.asarray([rot, *rect], dtype=np.float64).tobytes()


def root_candidates(limits):
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    return ge.load_package().m3rsm_root_candidates((limits[0], limits[1], 2 * limits[2]), limits[3])


def make_scenes(specs, shift=(0, 0)):
    """the scenes of `specs` -- (index into SCENES, which seeds the draws; the SCENES entry) -- with the whole scene moved by
    `shift` cells (make_golden_placed_pyramid.py: a station): the room, the pose and the scan's origin follow the map's
    origin, the draws are the same numbers as without the shift"""
    scenes, maps = [], {}
    for k, (name, cls, (w, h, origin), scale, n_beams, limits) in specs:
        rs = np.random.RandomState(SEED + k)
        cid, model, stride = CLASSES[cls]
        o = origin or (w // 2, h // 2)
        o = (o[0] - shift[0], o[1] - shift[1])
        mk = (cls, w, h, o, scale)
        if mk not in maps:  # the occ scenes on the 33x33 map share it
            maps[mk] = observations(np.random.RandomState(SEED + 100 + k), cid, w, h, o)
        x0, x1, y0, y1 = room(w, h, o)
        mid = np.array([(x0 + x1 + 1) / 2 * scale, (y0 + y1 + 1) / 2 * scale])
        pose = np.array([mid[0] + (0.3 + 0.4 * rs.rand()) * scale, mid[1] + (-0.2 + 0.4 * rs.rand()) * scale, 0.3 * rs.randn()])
        # the scan is cast from a pose a little off the one the match starts at: the matcher has something to find
        true_pose = pose + np.array([0.13, -0.09, 2.2 * DEG])
        ranges, angles, a_min, a_max, a_inc = cast_scan(rs, n_beams, true_pose, w, h, o, scale)
        scenes.append(dict(name=name, cls=cls, cid=cid, model=model, stride=stride, oie=0, w=w, h=h, origin=o, scale=scale,
                           obs=maps[mk], pose=pose, ranges=ranges, angles=angles, trig=(a_min, a_max, a_inc), limits=limits))
    return scenes


def run(exe, scenes, tag="m3rsm"):
    """the harness over `scenes`: every assertion of this generator per scene, then the fixture's arrays and the counters
    (one-sided splits, five-point expansions, the set of levels called on)"""
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

    out = {"n_scenes": np.array(len(scenes))}
    n_one_sided, n_five, all_levels = 0, 0, set()
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
        check_levels(m, levels, proto)
        n = int(take(1)[0])
        assert n == len(m["ranges"]), "filter_scan dropped a point"
        scan = take(5 * n, (n, 5))
        # run A: the matcher.  rows: pose x, y, theta, bot, top, left, right, value, scale_id, first point x, y
        res_a = take(4)
        rec_a = take(int(take(1)[0]) * 11).reshape(-1, 11)
        res_b = take(4)
        rec_b = take(int(take(1)[0]) * 11).reshape(-1, 11)
        res_c = take(5)
        n_calls = len(rec_a)
        assert n_calls <= MAX_CALLS, "%s: %d calls" % (m["name"], n_calls)
        assert np.all(np.isfinite(rec_a[:, 7])) and np.all(np.isfinite(res_a))
        # the rotation of every call of run A: the prerotated scan it was scored with, known from the root layer
        rot_roots, rect_roots = root_candidates(m["limits"])
        nr = len(rot_roots)
        assert np.array_equal(rec_a[:nr, 3:7], rect_roots), "the root layer is not the one m3rsm_root_candidates gives"
        by_scan = {}
        for j in range(nr):
            by_scan.setdefault(rec_a[j, 9:11].tobytes(), rot_roots[j])
            assert by_scan[rec_a[j, 9:11].tobytes()] == rot_roots[j], "two rotations with the same first point"
        rot = np.array([by_scan[rec_a[j, 9:11].tobytes()] for j in range(n_calls)])
        rect = rec_a[:, 3:7]
        assert np.all(rec_a[:, 2] == 0), "run A is not prerotated"
        assert np.array_equal(m["pose"][0] + (rect[:, 2] + (rect[:, 3] - rect[:, 2]) / 2), rec_a[:, 0])
        assert np.array_equal(m["pose"][1] + (rect[:, 0] + (rect[:, 1] - rect[:, 0]) / 2), rec_a[:, 1])
        # run B, not prerotated: the same trace bit for bit, at headings base + rotation
        assert len(rec_b) == n_calls, "%s: the non-prerotated run makes %d calls, not %d" % (m["name"], len(rec_b), n_calls)
        assert np.array_equal(rec_a[:, [0, 1, 3, 4, 5, 6, 7, 8]].view(np.int64), rec_b[:, [0, 1, 3, 4, 5, 6, 7, 8]].view(np.int64))
        assert np.array_equal(m["pose"][2] + rot, rec_b[:, 2]), "a heading of run B is not base + rotation"
        assert np.array_equal(res_a.view(np.int64), res_b.view(np.int64))
        # run C, perturbed scores: the same delta and number of calls
        assert np.array_equal(res_c[:3], res_a[:3]) and int(res_c[4]) == n_calls, \
            "%s: a 1e-12 perturbation moves the match (%r, %d calls against %r, %d)" % (m["name"], res_c[:3], res_c[4], res_a[:3], n_calls)
        # the trace follows the rules
        step = np.float64(m["limits"][4])
        allowed = {key(rot_roots[j], rect_roots[j]): ("root", 0) for j in range(nr)}
        for j in range(n_calls):
            kind = allowed.get(key(rot[j], rect[j]))
            assert kind is not None, "%s: call %d is no root and no child of an earlier call" % (m["name"], j)
            n_one_sided += kind == ("split2", 0)
            n_five += kind == ("points5", 4)
            ck, kids = children(rect[j], step)
            for c, kid in enumerate(kids):
                allowed[key(rot[j], kid)] = (ck, c)
        # the level of every call is the first whose scale holds the rectangle's longer side
        lv_scale = np.array([lv["scale"] for lv in levels])
        side = np.maximum(rect[:, 1] - rect[:, 0], rect[:, 3] - rect[:, 2])
        assert np.array_equal(rec_a[:, 8], [int(np.argmax(t <= lv_scale)) for t in side])
        all_levels |= set(rec_a[:, 8].astype(int).tolist())
        # the result is the winning point
        win = np.nonzero((rect[:, 0] == rect[:, 1]) & (rect[:, 2] == rect[:, 3]) & (rect[:, 2] == res_a[0]) & (rect[:, 0] == res_a[1])
                         & (rot == res_a[2]))[0]
        assert len(win) and np.any(rec_a[win, 7] == res_a[3])
        trace = np.column_stack([rot, rect, rec_a[:, 7], rec_a[:, 8]])
        out.update({pre + "name": np.array(m["name"]), pre + "cls": np.array(m["cls"]), pre + "model": np.array(m["model"]),
                    pre + "oie": np.array(m["oie"]), pre + "scale": np.array(m["scale"]), pre + "origin": np.array(m["origin"]),
                    pre + "unknown": proto, pre + "payload": levels[0]["payload"], pre + "pose": m["pose"], pre + "scan": scan,
                    pre + "limits": np.array(m["limits"]), pre + "delta": res_a[:3], pre + "prob": np.array(res_a[3]),
                    pre + "trace": trace})
        print("%-12s %5d calls, delta (%+.4f, %+.4f, %+.5f), prob %.6f, levels %s"
              % (m["name"], n_calls, res_a[0], res_a[1], res_a[2], res_a[3], sorted(set(rec_a[:, 8].astype(int).tolist()))))
    assert pos[0] == o.size
    if tag != "m3rsm":  # (a run for another fixture: the dense levels written out whole are large)
        os.remove(f_in), os.remove(f_out)
    return out, n_one_sided, n_five, all_levels


def main():
    if not os.path.isfile(os.path.join(REFERENCE, "src", "core", "scan_matchers", "bf_multi_res_scan_matcher.h")):
        sys.exit("reference tree not found at %s" % REFERENCE)
    exe = build()
    scenes = make_scenes(list(enumerate(SCENES)))
    out, n_one_sided, n_five, all_levels = run(exe, scenes)
    assert n_one_sided >= 10, "hardly a one-sided split among the calls (%d)" % n_one_sided
    assert n_five >= 50, "hardly a five-point expansion among the calls (%d)" % n_five
    assert len(all_levels) >= 4, "calls on fewer than four levels"
    path = os.path.join(GOLDEN_DIR, "m3rsm.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size <= 930 * 1024, "the fixture is larger than the largest one committed (%d bytes)" % size
    print("wrote m3rsm.npz: %d scenes, %d one-sided splits, %d five-point expansions, levels %s, %d KiB"
          % (len(scenes), n_one_sided, n_five, sorted(all_levels), size // 1024))


if __name__ == "__main__":
    main()
