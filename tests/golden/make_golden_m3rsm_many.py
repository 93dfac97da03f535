#!/usr/bin/env python3
"""Generate tests/golden/m3rsm_many.npz from the COMPILED REFERENCE: its M3RSMEngine (src/core/scan_matchers/
m3rsm_engine.h:252-365) given SEVERAL scan matching requests -- each its own scan, pose and
M3RSMRescalableGridMap<UnboundedPlainGridMap> -- and driven by the loop of BruteForceMultiResolutionScanMatcher::
process_scan (bf_multi_res_scan_matcher.h:44-65), with the full trace of scorer calls over all requests.

Runs only where the reference tree is present.  tests/golden/m3rsm_many_harness.cpp (ours; it includes the unmodified
reference headers) is compiled with the reference's own flags into oracle/_ref/ (git-ignored); the binary is never
committed.  The fixture is data only: the inputs made here and what the reference computed.

    python tests/golden/make_golden_m3rsm_many.py [path/to/reference]

Scenes (all: MaxOccupancyObservationPE, EvenSPW, the cached trig provider; rooms, updates and scans made as
make_golden_m3rsm.py makes them; a request's scan is cast from its pose plus an offset of its own, with noise of its own, so
the requests fit their maps differently well):
  occ_scans    many scans, one map: GridCell 33x33 at 0.1; three requests with 67, 40 and 1 beams from three poses;
               limits +-0.4 m, +-0.4 m, +-5 deg at 1 deg, step 0.05
  occ_m2m      many-to-many: GridCell 33x33 at 0.1 centred and 37x29 at 0.05 with origin (11, 20) -- different extent,
               origin and scale, so the same rectangle lies on a different level of either (both have 7 scales: 17 and 26
               cells from the origin are both within 2^5) --, two scans on each: four requests; limits +-0.3 / +-0.45,
               step 0.07
  tbm_pair, cred_pair   TbmOccConsistentCell / CredibilistCell 33x33 at 0.1 under the discrepancy OIE, two requests each

Asserted here (the fixture is not written otherwise):
  * validate() of the reference is true for every map and its levels are the tight ones (make_golden_m3rsm.py's checks);
  * the root layers come request by request in the order given, each the list m3rsm_root_candidates gives; every later
    call is the split / point child, by the rule of include/slamhip.h "EXPAND", of an earlier call of the SAME request
    at the same rotation; every call's level is the first of ITS map whose scale holds the rectangle's longer side;
  * a run with prerotate_scan = false gives the same trace bit for bit, its headings the request's heading + rotation;
  * a run with every score multiplied by 1 +- 1e-12 gives the same winner, delta and number of calls;
  * the winner is the request whose LONE match (run in the same harness) has the largest probability, with that match's
    delta and probability;
  * in at least one scene the winner is not request 0; in at least one scene the shared search makes fewer calls than
    the lone matches together; after the root layers every scene's trace interleaves calls of at least two requests;
  * every scene makes at most 6000 calls; the fixture is at most 930 KiB.

Contents: n_scenes; per scene s<i>_: name, cls, model, oie, limits (max_x, max_y, max_th, rotation step, translation
step), n_maps, per map m<j>_scale, m<j>_origin, m<j>_unknown [stride], m<j>_payload [h, w, stride]; n_requests, per request
r<j>_map, r<j>_pose, r<j>_scan [n, 5] (range, cos a, sin a, weight, factor); winner, delta [3], prob; trace [n_calls, 8]
(request, rotation, bot, top, left, right, score, level); lone [n_requests, 5] (delta, prob, calls of the lone match).
"""
import os
import subprocess
import sys

import numpy as np
from make_golden_m3rsm import (CLASSES, DEG, GOLDEN_DIR, OUT_DIR, REFERENCE, SEED, cast_scan, check_levels, children, key,
                               observations, room, root_candidates)

MAX_CALLS = 6000
# per map: (w, h, origin or None, scale); per request: (map, beams, offset of the scan's true pose, range noise in cells)
SCENES = [
    ("occ_scans", "occ", [(33, 33, None, 0.1)], (0.4, 0.4, 5 * DEG, 1 * DEG, 0.05),
     [(0, 67, (0.13, -0.09, 2.2), 0.5), (0, 40, (-0.21, 0.17, -3.1), 0.2), (0, 1, (0.05, 0.02, 1.0), 0.2)]),
    ("occ_m2m", "occ", [(33, 33, None, 0.1), (37, 29, (11, 20), 0.05)], (0.3, 0.45, 5 * DEG, 1 * DEG, 0.07),
     [(0, 67, (0.13, -0.09, 2.2), 0.5), (0, 40, (-0.08, 0.22, -1.3), 0.2), (1, 67, (0.11, 0.06, -2.4), 0.4),
      (1, 40, (-0.05, -0.12, 3.3), 0.1)]),
    ("tbm_pair", "tbm", [(33, 33, None, 0.1)], (0.4, 0.4, 5 * DEG, 1 * DEG, 0.05),
     [(0, 67, (0.13, -0.09, 2.2), 0.5), (0, 40, (-0.21, 0.17, -3.1), 0.2)]),
    ("cred_pair", "cred", [(33, 33, None, 0.1)], (0.4, 0.4, 5 * DEG, 1 * DEG, 0.05),
     [(0, 40, (0.13, -0.09, 2.2), 0.2), (0, 67, (-0.21, 0.17, -3.1), 0.5)]),
]


class NoNoise:
    """cast_scan's noise source switched off: a request adds noise of its own size"""
    @staticmethod
    def randn():
        return 0.0


def build():
    os.makedirs(OUT_DIR, exist_ok=True)
    exe = os.path.join(OUT_DIR, "m3rsm_many_harness")
    subprocess.check_call(["g++", "-std=c++14", "-O3", "-w", "-I" + os.path.join(REFERENCE, "src"), "-o", exe,
                           os.path.join(GOLDEN_DIR, "m3rsm_many_harness.cpp")])
    return exe


def make_scenes(specs):
    """the scenes of `specs` (entries like SCENES'; a map spec may carry a fifth element, a shift in cells by which the
    whole map -- and with its room the poses and scans of its requests -- is moved: make_golden_placed_pyramid.py)"""
    scenes = []
    for k, (name, cls, map_specs, limits, req_specs) in enumerate(specs):
        cid, model, stride = CLASSES[cls]
        maps = []
        for j, (w, h, origin, scale, *shift) in enumerate(map_specs):
            o = origin or (w // 2, h // 2)
            if shift:
                o = (o[0] - shift[0][0], o[1] - shift[0][1])
            maps.append(dict(w=w, h=h, origin=o, scale=scale, stride=stride,
                             obs=observations(np.random.RandomState(SEED + 1000 + 10 * k + j), cid, w, h, o)))
        reqs = []
        for j, (mi, n_beams, off, noise) in enumerate(req_specs):
            rs = np.random.RandomState(SEED + 2000 + 10 * k + j)
            m = maps[mi]
            x0, x1, y0, y1 = room(m["w"], m["h"], m["origin"])
            mid = np.array([(x0 + x1 + 1) / 2 * m["scale"], (y0 + y1 + 1) / 2 * m["scale"]])
            pose = np.array([mid[0] + (-0.5 + rs.rand()) * 4 * m["scale"], mid[1] + (-0.5 + rs.rand()) * 4 * m["scale"],
                             0.3 * rs.randn()])
            true_pose = pose + np.array([off[0], off[1], off[2] * DEG])
            ranges, angles, a_min, a_max, a_inc = cast_scan(NoNoise, n_beams, true_pose, m["w"], m["h"], m["origin"], m["scale"])
            ranges = ranges + noise * m["scale"] * rs.randn(n_beams)
            reqs.append(dict(map=mi, pose=pose, ranges=ranges, angles=angles, trig=(a_min, a_max, a_inc)))
        scenes.append(dict(name=name, cls=cls, cid=cid, model=model, stride=stride, oie=0, maps=maps, reqs=reqs, limits=limits))
    return scenes


def run(exe, scenes, tag="m3rsm_many"):
    """the harness over `scenes`: every assertion of this generator per scene, then the fixture's arrays and the counters
    (scenes request 0 does not win, scenes in which the shared cut saves calls)"""
    inp = [len(scenes)]
    for s in scenes:
        inp += [s["cid"], s["oie"], len(s["maps"])]
        for m in s["maps"]:
            inp += [m["w"], m["h"], m["scale"], m["origin"][0], m["origin"][1], len(m["obs"]), *m["obs"].ravel()]
        inp.append(len(s["reqs"]))  # one scan per request
        for r in s["reqs"]:
            inp += [len(r["ranges"]), *r["ranges"], *r["angles"], *r["trig"]]
        inp += [*s["limits"], len(s["reqs"])]
        for j, r in enumerate(s["reqs"]):
            inp += [r["map"], j, *r["pose"]]
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
    not_first, cut_bites = 0, 0
    for i, s in enumerate(scenes):
        pre, stride, n_req = "s%d_" % i, s["stride"], len(s["reqs"])
        map_levels = []
        for j, m in enumerate(s["maps"]):
            n_scales, valid = (int(v) for v in take(2))
            assert valid == 1, "validate() is false for map %d of scene %s" % (j, s["name"])
            proto = take(stride)
            levels = []
            for _ in range(n_scales):
                lw, lh, ox, oy = (int(v) for v in take(4))
                sc = float(take(1)[0])
                cells = take(lw * lh * (stride + 2), (lh, lw, stride + 2))
                levels.append(dict(w=lw, h=lh, origin=(ox, oy), scale=sc, payload=cells[..., :stride],
                                   unknown=cells[..., stride] != 0, impact=cells[..., stride + 1]))
            check_levels(m, levels, proto)
            map_levels.append(levels)
            out.update({pre + "m%d_scale" % j: np.array(m["scale"]), pre + "m%d_origin" % j: np.array(m["origin"]),
                        pre + "m%d_unknown" % j: proto, pre + "m%d_payload" % j: levels[0]["payload"]})
        # run M.  rows: request, pose x, y, theta, bot, top, left, right, value, scale_id, first point x, y
        res_m = take(5)
        rec_m = take(int(take(1)[0]) * 12).reshape(-1, 12)
        for j, r in enumerate(s["reqs"]):
            n = int(take(1)[0])
            assert n == len(r["ranges"]), "filter_scan dropped a point"
            out.update({pre + "r%d_map" % j: np.array(r["map"]), pre + "r%d_pose" % j: r["pose"], pre + "r%d_scan" % j: take(5 * n, (n, 5))})
        res_n = take(5)
        rec_n = take(int(take(1)[0]) * 12).reshape(-1, 12)
        res_p = take(5)
        calls_p = int(take(1)[0])
        lone = np.zeros((n_req, 5))
        lone_winner = []
        for j in range(n_req):
            res_l = take(5)
            lone_winner.append(int(res_l[0]))
            lone[j] = [*res_l[1:5], take(1)[0]]
        assert lone_winner == list(range(n_req))
        n_calls = len(rec_m)
        assert n_calls <= MAX_CALLS, "%s: %d calls" % (s["name"], n_calls)
        assert np.all(np.isfinite(rec_m[:, 8])) and np.all(np.isfinite(res_m)) and np.all(np.isfinite(lone))
        req = rec_m[:, 0].astype(int)
        rect = rec_m[:, 4:8]
        # the root layers: request by request, each the list m3rsm_root_candidates gives
        rot_roots, rect_roots = root_candidates(s["limits"])
        nr = len(rot_roots)
        assert np.array_equal(req[:nr * n_req], np.repeat(np.arange(n_req), nr)), "the root layers are not request by request"
        by_scan = {}
        for g in range(nr * n_req):
            j = g % nr
            assert np.array_equal(rect[g], rect_roots[j]), "a root layer is not the one m3rsm_root_candidates gives"
            k2 = (req[g], rec_m[g, 10:12].tobytes())
            assert by_scan.setdefault(k2, rot_roots[j]) == rot_roots[j], "two rotations of a request with the same first point"
        rot = np.array([by_scan[req[g], rec_m[g, 10:12].tobytes()] for g in range(n_calls)])
        base = np.array([s["reqs"][r]["pose"] for r in req])
        assert np.all(rec_m[:, 3] == 0), "run M is not prerotated"
        assert np.array_equal(base[:, 0] + (rect[:, 2] + (rect[:, 3] - rect[:, 2]) / 2), rec_m[:, 1])
        assert np.array_equal(base[:, 1] + (rect[:, 0] + (rect[:, 1] - rect[:, 0]) / 2), rec_m[:, 2])
        # run N, not prerotated: the same trace bit for bit, at headings base + rotation
        assert len(rec_n) == n_calls, "%s: the non-prerotated run makes %d calls, not %d" % (s["name"], len(rec_n), n_calls)
        same = [0, 1, 2, 4, 5, 6, 7, 8, 9]
        assert np.array_equal(rec_m[:, same].view(np.int64), rec_n[:, same].view(np.int64))
        assert np.array_equal(base[:, 2] + rot, rec_n[:, 3]), "a heading of run N is not base + rotation"
        assert np.array_equal(res_m.view(np.int64), res_n.view(np.int64))
        # run P, perturbed scores: the same winner, delta and number of calls
        assert np.array_equal(res_p[:4], res_m[:4]) and calls_p == n_calls, \
            "%s: a 1e-12 perturbation moves the match (%r, %d calls against %r, %d)" % (s["name"], res_p, calls_p, res_m, n_calls)
        # the winner is the request whose lone match is the best one, with that match's result
        winner = int(res_m[0])
        assert winner == int(np.argmax(lone[:, 3])) and np.sum(lone[:, 3] == lone[winner, 3]) == 1, "%s: %r / %r" % (s["name"], res_m, lone)
        assert np.array_equal(res_m[1:5].view(np.int64), lone[winner, :4].view(np.int64)), "%s: %r / %r" % (s["name"], res_m, lone)
        not_first += winner != 0
        cut_bites += n_calls < lone[:, 4].sum()
        assert n_calls <= lone[:, 4].sum()
        # the trace follows the rules, request by request
        step = np.float64(s["limits"][4])
        allowed = {(r, key(rot_roots[j], rect_roots[j])) for r in range(n_req) for j in range(nr)}
        for g in range(n_calls):
            assert (req[g], key(rot[g], rect[g])) in allowed, "%s: call %d is no root and no child of an earlier call" % (s["name"], g)
            for kid in children(rect[g], step)[1]:
                allowed.add((req[g], key(rot[g], kid)))
        side = np.maximum(rect[:, 1] - rect[:, 0], rect[:, 3] - rect[:, 2])
        for g in range(n_calls):
            lv_scale = np.array([lv["scale"] for lv in map_levels[s["reqs"][req[g]]["map"]]])
            assert rec_m[g, 9] == int(np.argmax(side[g] <= lv_scale))
        # after the root layers the calls of at least two requests interleave
        later = req[nr * n_req:]
        runs = 1 + int(np.count_nonzero(np.diff(later)))
        assert len(set(later.tolist())) >= 2 and runs >= 4, "%s: the trace does not interleave requests" % s["name"]
        # the result is a point on record
        win = np.nonzero((req == winner) & (rect[:, 0] == rect[:, 1]) & (rect[:, 2] == rect[:, 3]) & (rect[:, 2] == res_m[1])
                         & (rect[:, 0] == res_m[2]) & (rot == res_m[3]))[0]
        assert len(win) and np.any(rec_m[win, 8] == res_m[4])
        trace = np.column_stack([req.astype(np.float64), rot, rect, rec_m[:, 8], rec_m[:, 9]])
        out.update({pre + "name": np.array(s["name"]), pre + "cls": np.array(s["cls"]), pre + "model": np.array(s["model"]),
                    pre + "oie": np.array(s["oie"]), pre + "limits": np.array(s["limits"]), pre + "n_maps": np.array(len(s["maps"])),
                    pre + "n_requests": np.array(n_req), pre + "winner": np.array(winner), pre + "delta": res_m[1:4],
                    pre + "prob": np.array(res_m[4]), pre + "trace": trace, pre + "lone": lone})
        print("%-10s %5d calls (lone: %s), winner %d, delta (%+.4f, %+.4f, %+.5f), prob %.6f (lone: %s), %d runs of one request"
              % (s["name"], n_calls, lone[:, 4].astype(int).tolist(), winner, res_m[1], res_m[2], res_m[3], res_m[4],
                 ["%.6f" % v for v in lone[:, 3]], runs))
    assert pos[0] == o.size
    if tag != "m3rsm_many":  # (a run for another fixture: the dense levels written out whole are large)
        os.remove(f_in), os.remove(f_out)
    return out, not_first, cut_bites


def main():
    if not os.path.isfile(os.path.join(REFERENCE, "src", "core", "scan_matchers", "bf_multi_res_scan_matcher.h")):
        sys.exit("reference tree not found at %s" % REFERENCE)
    exe = build()
    scenes = make_scenes(SCENES)
    out, not_first, cut_bites = run(exe, scenes)
    assert not_first >= 1, "request 0 wins every scene"
    assert cut_bites >= 1, "the shared cut saves no call in any scene"
    path = os.path.join(GOLDEN_DIR, "m3rsm_many.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size <= 930 * 1024, "the fixture is larger than the largest one committed (%d bytes)" % size
    print("wrote m3rsm_many.npz: %d scenes, %d KiB" % (len(scenes), size // 1024))


if __name__ == "__main__":
    main()
