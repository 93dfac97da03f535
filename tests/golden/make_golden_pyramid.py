#!/usr/bin/env python3
"""Generate tests/golden/pyramid.npz from the COMPILED REFERENCE: the levels of M3RSMRescalableGridMap
<UnboundedPlainGridMap> (src/core/scan_matchers/m3rsm_engine.h:17-131) over small maps of every cell class the device
pyramid takes, and Match::prob_upper_bound (:156-180) of the matches the reference's M3RSMEngine makes over two of them.

Runs only where the reference tree is present.  tests/golden/pyramid_harness.cpp (ours; it includes the unmodified
reference headers) is compiled with the reference's own flags into oracle/_ref/ (git-ignored); the binary is never
committed.  The fixture is data only: the inputs made here and what the reference computed.

    python tests/golden/make_golden_pyramid.py [path/to/reference]

Maps: classes GridCell (prototype occupancy 0.5), TbmOccConsistentCell, CredibilistCell under DiscrepancyOIE, GridCell
also under OccupancyOIE (the device scores -- and bounds -- belief cells under the discrepancy OIE only); fine shapes
16x16, 15x3, 3x15, 33x33, 1x16 (origin = the centre the reference gives them), 37x29 with origin (11, 20), and 16x16 with
origin (2, 3) -- so far off centre that the reference ADDS a level while it is filled (approximationLevelExtension); its
far corner is written first, so that the added level sees every later cell --; scales 1.0, 0.1, 0.05.  About a third of
the cells are never updated, the others once in a seeded random order, then a second pass raises some of them.
Observations are drawn from small discrete sets, so that two impacts are either bit-equal or far apart.

Asserted here (the fixture is not written otherwise):
  * validate() of the reference is true;
  * no updated cell is bit-equal to the prototype, every never-updated cell is;
  * within every block of every level two distinct impacts differ by more than 1e-6, and bit-equal maximal impacts
    carry bit-equal payloads;
  * every level cell of the reference holds the impact max over the known fine cells (x, y) with floor(x / 2^k) == X,
    floor(y / 2^k) == Y -- the integer rule for GridRasterizedRectangle{coarser, world_cell_bounds(fine), false} and
    its 1e-9 offset at all three scales -- and the unknown flag exactly where the block has no known cell.
These make the reference's levels the tight ones.

Contents, per map m<i>: _cls, _model, _oie, _scale, _origin, _unknown [stride], _payload [h, w, stride],
_n_levels (levels above the fine map), per level k = 1 ..: _L<k>_origin, _L<k>_scale, _L<k>_payload [h_k, w_k, stride] (the
reference's own window of that level; cells the reference has not written hold the prototype).

Matches: the reference's own M3RSMEngine runs over the 33x33 and 37x29 maps with a recording ScanProbabilityEstimator (it
forwards to WeightedMeanPointProbabilitySPE over MaxOccupancyObservationPE and writes every call down in call order: pose,
sp_analysis_area, the map's scale_id, the value).  Per map two scans (67 beams, 1 beam; cached trig provider) and per
scan three runs: add_scan_matching_request with limits (+-0.4, +-0.4, +-5 deg) at 1 deg -- the 22 roots of the issue --
followed by next_best_match(0.05) calls until 48 branch records exist (split4_evenly), then the same with ranges
(0.4, 0.2) and (0.2, 0.4), whose deepest branches are one-sided (split_horz / split_vert), 28 records each.  The engine
is best-first over eleven rotations: on the 67-beam scans its first branches stay on the coarse levels, on the 1-beam
scans they reach the fine map.  Asserted: the pose of every call is the base pose moved by the rectangle's centre and
turned by a rotation r (recovered as the r with theta + r bit-equal to the call's heading); the recorded scale_id is
the first level whose scale holds the rectangle's longer side; every branch has its parent on record (same heading, the
rectangle that holds it with 2 or 4 times its area) and does not exceed it by more than 1e-5.

Per match set s<j>: _map (index), _pose, _scan [n, 5] (range, cos a, sin a, weight, factor: the cached provider's table
entries of the points filter_scan kept), _limits (max_x, max_y, sector, rotation step, translation step), _runs,
_n_roots (the first run's root layer: the first _n_roots rows of _cand), _cand [n, 9] (rotation, bot, top, left, right,
parent row or -1, prob_upper_bound, level, the heading the reference scored at).
"""
import os
import subprocess
import sys

import numpy as np

GOLDEN_DIR = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(GOLDEN_DIR))
REFERENCE = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("REFERENCE", "/root/reference")
OUT_DIR = os.path.join(ROOT, "oracle", "_ref")

# name, harness class id, SLAMHIP_CELL_* model, stride
CLASSES = [("grid_cell", 0, 0, 1), ("tbm_consistent", 1, 1, 4), ("credibilist", 2, 3, 4)]
SHAPES = [(16, 16, None), (15, 3, None), (3, 15, None), (33, 33, None), (1, 16, None), (37, 29, (11, 20)), (16, 16, (2, 3))]
SCALES = [1.0, 0.1, 0.05]
MATCH_SHAPES = [(33, 33, None), (37, 29, (11, 20))]
LIMITS = (0.4, 0.4, 2 * np.deg2rad(5.0), np.deg2rad(1.0), 0.05)  # max_x, max_y, sector = 2 max_th, rotation step, translation step
# runs of the reference's engine per match set: (max_x, max_y, records kept behind the root layer).  The first is LIMITS'
# square range; the other two end in a one-sided branch (split_horz / split_vert)
RUNS = [(0.4, 0.4, 48), (0.4, 0.2, 28), (0.2, 0.4, 28)]


def build():
    os.makedirs(OUT_DIR, exist_ok=True)
    exe = os.path.join(OUT_DIR, "pyramid_harness")
    subprocess.check_call(["g++", "-std=c++14", "-O3", "-w", "-I" + os.path.join(REFERENCE, "src"), "-o", exe,
                           os.path.join(GOLDEN_DIR, "pyramid_harness.cpp")])
    return exe


def observations(rs, cls, w, h, origin):
    """x, y, is_occ, prob, est_quality, quality per update, in the order they are applied"""
    cells = [(x - origin[0], y - origin[1]) for y in range(h) for x in range(w)]
    far = max(cells, key=lambda c: (abs(c[0]) + abs(c[1]), c))  # the cell that decides the number of levels
    chosen = [c for c in cells if c != far and rs.rand() >= 1.0 / 3.0]
    order = [far] + [chosen[i] for i in rs.permutation(len(chosen))]
    obs, first = [], {}
    for c in order:
        if cls == 0:
            k = int(rs.choice([j for j in range(0, 1000, 8) if j != 512]))
            first[c] = k
            obs.append([c[0], c[1], float(k > 512), k / 1024.0, 1.0, 1.0])
        else:
            prob = float(rs.choice([0.05, 0.2, 0.35, 0.65, 0.8, 0.95]))
            obs.append([c[0], c[1], float(prob > 0.5), prob, float(rs.choice([1.0, 0.7])), float(rs.choice([0.9, 0.6]))])
    for c in order:  # the second pass raises about a fifth of them
        if rs.rand() >= 0.2:
            continue
        if cls == 0:
            obs.append([c[0], c[1], 1.0, (first[c] + 4 + 8 * int(rs.randint(0, 3))) / 1024.0, 1.0, 1.0])
        else:
            obs.append([c[0], c[1], 1.0, 0.97, 1.0, 0.9])
    return np.asarray(obs, dtype=np.float64)


def scans(rs, scale, w, h):
    """two scans whose end points fall inside (and a little outside) the map: 67 beams and 1 beam"""
    out = []
    for n in (67, 1):
        a_inc = 2 * np.pi / 90
        a_min = -np.pi / 2
        angles = a_min + a_inc * np.arange(n)
        ranges = (2.0 + rs.rand(n) * (0.55 * min(max(w, 8), max(h, 8)) - 2.0)) * scale
        out.append((ranges, angles, a_min, a_min + (n + 0.5) * a_inc, a_inc))
    return out


def make_maps(rs, shapes, shift=(0, 0), match_shapes=None):
    """the maps of the fixture: shapes x SCALES x classes (GridCell under both OIEs), with their match sets.  shift: the
    whole map, observations and poses moved by that many cells (make_golden_placed_pyramid.py: a station) -- the draws
    are the same numbers as without it."""
    maps = []
    for w, h, origin in shapes:
        o = origin or (w // 2, h // 2)
        o = (o[0] - shift[0], o[1] - shift[1])
        for scale in SCALES:
            for name, cid, model, stride in CLASSES:
                for oie in ((0, 1) if cid == 0 else (0,)):
                    obs = observations(rs, cid, w, h, o)
                    sets = []
                    if (w, h, origin) in (MATCH_SHAPES if match_shapes is None else match_shapes):
                        pose = np.array([(0.3 + 0.4 * rs.rand()) * scale, (-0.2 + 0.4 * rs.rand()) * scale, 0.3 * rs.randn()])
                        pose = pose + [shift[0] * scale, shift[1] * scale, 0.0]
                        for ranges, angles, a_min, a_max, a_inc in scans(rs, scale, w, h):
                            sets.append(dict(pose=pose, ranges=ranges, angles=angles, trig=(a_min, a_max, a_inc)))
                    maps.append(dict(cls=name, cid=cid, model=model, stride=stride, oie=oie, w=w, h=h, origin=o, scale=scale, obs=obs,
                                     sets=sets))
    return maps


def crop_level(payload, origin, proto):
    """the window of a level cut down to the box of the cells that are not the prototype (a dense level of a map far from
    (0, 0) spans back to the origin: nearly all of it never written); origin moved along"""
    known = ~np.all(payload.view(np.int64) == proto.view(np.int64), axis=-1)
    if not known.any():
        return payload[:1, :1].copy(), origin
    ys, xs = np.nonzero(known)
    return payload[ys.min():ys.max() + 1, xs.min():xs.max() + 1].copy(), (origin[0] - int(xs.min()), origin[1] - int(ys.min()))


def run(exe, maps, crop=False, tag="pyramid"):
    """the harness over `maps`: every assertion of this generator, then the fixture's arrays and the counters
    (sets, candidates, maps with a level added during the fill, one-sided splits, sets that reached the fine map)"""
    inp = []
    inp.append(len(maps))
    for m in maps:
        inp += [m["cid"], m["oie"], m["w"], m["h"], m["scale"], m["origin"][0], m["origin"][1], len(m["obs"]), *m["obs"].ravel(),
                len(m["sets"])]
        for s in m["sets"]:
            inp += [*s["pose"], len(s["ranges"]), *s["ranges"], *s["angles"], *s["trig"], *LIMITS[2:], len(RUNS)]
            for run in RUNS:
                inp += list(run)
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

    out, n_sets, n_cands, extended, n_one_sided, reached_fine = {"n_maps": np.array(len(maps))}, 0, 0, 0, 0, 0
    for i, m in enumerate(maps):
        pre, stride = "m%d_" % i, m["stride"]
        n_scales, valid = (int(v) for v in take(2))
        assert valid == 1, "validate() is false for map %d" % i
        proto = take(stride)
        levels = []
        for k in range(n_scales):
            lw, lh, ox, oy = (int(v) for v in take(4))
            sc = float(take(1)[0])
            cells = take(lw * lh * (stride + 2), (lh, lw, stride + 2))
            levels.append(dict(w=lw, h=lh, origin=(ox, oy), scale=sc, payload=cells[..., :stride], unknown=cells[..., stride] != 0,
                               impact=cells[..., stride + 1]))
        fine = levels[0]
        assert (fine["w"], fine["h"], fine["origin"]) == (m["w"], m["h"], tuple(m["origin"])), "the fine map grew"
        assert fine["scale"] == m["scale"] and np.isinf(levels[-1]["scale"]) and (levels[-1]["w"], levels[-1]["h"]) == (1, 1)
        updated = np.zeros((m["h"], m["w"]), bool)
        updated[(m["obs"][:, 1] + m["origin"][1]).astype(int), (m["obs"][:, 0] + m["origin"][0]).astype(int)] = True
        same_as_proto = np.all(fine["payload"].view(np.int64) == proto.view(np.int64), axis=-1)
        assert np.array_equal(fine["unknown"], ~updated) and np.array_equal(same_as_proto, ~updated), "a cell equals the prototype"
        # the integer rule, tightness, the separation of impacts
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
        ctor = 0  # what the constructor alone makes (ensure_map_cache_is_continuous over w x h)
        while max(m["w"], m["h"]) > 2 ** (ctor + 1):
            ctor += 1
        extended += n_scales - 2 > ctor
        out.update({pre + "cls": np.array(m["cls"]), pre + "model": np.array(m["model"]), pre + "oie": np.array(m["oie"]),
                    pre + "scale": np.array(m["scale"]), pre + "origin": np.array(m["origin"]), pre + "unknown": proto,
                    pre + "payload": fine["payload"], pre + "n_levels": np.array(n_scales - 1)})
        for k in range(1, n_scales):
            pay, org = crop_level(levels[k]["payload"], levels[k]["origin"], proto) if crop else (levels[k]["payload"], levels[k]["origin"])
            out.update({pre + "L%d_origin" % k: np.array(org), pre + "L%d_scale" % k: np.array(levels[k]["scale"]),
                        pre + "L%d_payload" % k: pay})
        for s in m["sets"]:
            sp = "s%d_" % n_sets
            assert int(take(1)[0]) == len(RUNS)
            scan, cand, n_roots, one_sided = None, [], None, 0
            for r, run in enumerate(RUNS):
                if r == 0:
                    n = int(take(1)[0])
                    assert n == len(s["ranges"]), "filter_scan dropped a point"
                    scan = take(5 * n, (n, 5))
                roots, kept = (int(v) for v in take(2))
                best = float(take(1)[0])
                rec = take(9 * kept, (kept, 9))  # pose x, y, theta, bot, top, left, right, value, scale_id
                assert roots == 22 and np.all(np.isfinite(rec[:, 7])) and np.isfinite(best)
                rect = rec[:, 3:7]
                # the rotation the engine added to the heading: r with pose.theta + r == the theta it scored at, bit for bit
                rot = rec[:, 2] - s["pose"][2]
                for _ in range(4):
                    got = s["pose"][2] + rot
                    rot = np.where(got < rec[:, 2], np.nextafter(rot, np.inf), np.where(got > rec[:, 2], np.nextafter(rot, -np.inf), rot))
                assert np.array_equal(s["pose"][2] + rot, rec[:, 2])
                # ... and the pose is the base pose moved by LightWeightRectangle::center()
                assert np.array_equal(s["pose"][0] + (rect[:, 2] + (rect[:, 3] - rect[:, 2]) / 2), rec[:, 0])
                assert np.array_equal(s["pose"][1] + (rect[:, 0] + (rect[:, 1] - rect[:, 0]) / 2), rec[:, 1])
                # the root layer: per rotation the empty rectangle, then the entire one
                assert np.all(rect[0:roots:2] == 0) and np.all(rect[1:roots:2] == [-run[1], run[1], -run[0], run[0]])
                assert np.array_equal(rot[0:roots:2], rot[1:roots:2]) and len(set(rot[:roots].tolist())) == 11
                # a branch's parent: the latest earlier call at the same heading whose rectangle holds this one and has
                # twice or four times its area (the engine scores a branch's children right after it pops the parent)
                parent = np.full(kept, -1.0)
                area = (rect[:, 1] - rect[:, 0]) * (rect[:, 3] - rect[:, 2])
                for c in range(roots, kept):
                    for j in range(c - 1, -1, -1):
                        if (rec[j, 2] == rec[c, 2] and rect[j, 0] <= rect[c, 0] and rect[c, 1] <= rect[j, 1] and rect[j, 2] <= rect[c, 2]
                                and rect[c, 3] <= rect[j, 3] and area[c] > 0 and round(area[j] / area[c]) in (2, 4)
                                and abs(area[j] / area[c] - round(area[j] / area[c])) < 1e-9):
                            parent[c] = j + len(cand)
                            one_sided += round(area[j] / area[c]) == 2
                            break
                    assert parent[c] >= 0, "a branch without a parent among the recorded calls"
                if r == 0:
                    n_roots = roots
                cand += np.column_stack([rot, rect, parent, rec[:, 7], rec[:, 8], rec[:, 2]]).tolist()
            cand = np.asarray(cand)
            nc = len(cand)
            lv_scale = np.array([lv["scale"] for lv in levels])
            side = np.maximum(cand[:, 2] - cand[:, 1], cand[:, 4] - cand[:, 3])
            assert np.array_equal(cand[:, 7], [int(np.argmax(t <= lv_scale)) for t in side])
            kids = cand[:, 5] >= 0
            assert kids.sum() >= 60
            reached_fine += bool(m["scale"] < 1.0 and np.any(cand[kids, 7] == 0))
            assert np.all(cand[kids, 6] <= cand[cand[kids, 5].astype(int), 6] + 1e-5)
            n_one_sided += one_sided
            out.update({sp + "map": np.array(i), sp + "pose": s["pose"], sp + "scan": scan, sp + "limits": np.array(LIMITS), sp + "runs": np.array(RUNS, dtype=np.float64),
                        sp + "n_roots": np.array(n_roots), sp + "cand": cand})
            n_sets += 1
            n_cands += nc
    assert pos[0] == o.size
    out["n_sets"] = np.array(n_sets)
    return out, dict(sets=n_sets, cands=n_cands, extended=extended, one_sided=n_one_sided, reached_fine=reached_fine)


def main():
    if not os.path.isfile(os.path.join(REFERENCE, "src", "core", "scan_matchers", "m3rsm_engine.h")):
        sys.exit("reference tree not found at %s" % REFERENCE)
    exe = build()
    maps = make_maps(np.random.RandomState(20261018), SHAPES)
    out, c = run(exe, maps)
    n_sets, n_cands, extended, n_one_sided, reached_fine = c["sets"], c["cands"], c["extended"], c["one_sided"], c["reached_fine"]
    assert extended > 0, "no map made the reference add a level while it was filled"
    assert reached_fine >= 8, "hardly a branch that reached the fine map on a map finer than the rectangle"
    assert n_one_sided >= 10, "hardly a one-sided split (split_horz / split_vert) among the branches"
    path = os.path.join(GOLDEN_DIR, "pyramid.npz")
    np.savez_compressed(path, **out)
    print("wrote pyramid.npz: %d maps (%d with a level added during the fill), %d match sets, %d candidates, %d KiB"
          % (len(maps), extended, n_sets, n_cands, os.path.getsize(path) // 1024))


if __name__ == "__main__":
    main()
