"""Shared by tests/test_pyramid_host.py and tests/test_gpu_pyramid.py: the goldens of tests/golden/pyramid.npz
(make_golden_pyramid.py: levels and bounds of the compiled reference's M3RSMRescalableGridMap / Match) as objects, the
comparison of two windows of one level in EXTERNAL coordinates, and a brute-force statement of the level definition."""
import os
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "pyramid.npz"))
N_MAPS, N_SETS = int(G["n_maps"]), int(G["n_sets"])


def golden_map(i):
    pre = "m%d_" % i
    m = types.SimpleNamespace(cell_model=int(G[pre + "model"]), payload=G[pre + "payload"], origin=tuple(int(v) for v in G[pre + "origin"]),
                              scale=float(G[pre + "scale"]), unknown=G[pre + "unknown"], oie=int(G[pre + "oie"]), cls=str(G[pre + "cls"]))
    m.height, m.width = m.payload.shape[:2]
    m.levels = [dict(origin=tuple(int(v) for v in G[pre + "L%d_origin" % k]), scale=float(G[pre + "L%d_scale" % k]),
                     payload=G[pre + "L%d_payload" % k]) for k in range(1, int(G[pre + "n_levels"]) + 1)]
    return m


def golden_set(j):
    pre = "s%d_" % j
    return types.SimpleNamespace(map=int(G[pre + "map"]), pose=G[pre + "pose"], scan=G[pre + "scan"], limits=G[pre + "limits"],
                                 n_roots=int(G[pre + "n_roots"]), cand=G[pre + "cand"])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def assert_same_level(got_payload, got_origin, want_payload, want_origin, unknown, what=""):
    """two windows of one level hold the same cells: compared bit for bit over the union of the windows in external
    coordinates, a cell outside a window being the unknown payload (what Unbounded*GridMap::operator[] returns)"""
    def span(p, o):
        return -o[0], -o[1], p.shape[1] - o[0], p.shape[0] - o[1]
    a, b = span(got_payload, got_origin), span(want_payload, want_origin)
    x0, y0, x1, y1 = min(a[0], b[0]), min(a[1], b[1]), max(a[2], b[2]), max(a[3], b[3])

    def canvas(p, o):
        c = np.empty((y1 - y0, x1 - x0, p.shape[2]))
        c[...] = np.asarray(unknown)[:p.shape[2]]
        c[-o[1] - y0:-o[1] - y0 + p.shape[0], -o[0] - x0:-o[0] - x0 + p.shape[1]] = p
        return c
    np.testing.assert_array_equal(bits(canvas(got_payload, got_origin)), bits(canvas(want_payload, want_origin)), err_msg=what)


def brute_levels(payload, origin, unknown, impact):
    """The definition, cell by cell: per level k the external blocks floor(x / 2^k), floor(y / 2^k) of the known cells
    (payload not bit-equal to `unknown`), each holding the payload of the cell of largest impact(payload) -- smallest
    x, then y, among equals --; the last level is one block.  Returns [{(X, Y): payload}], level 1 first."""
    h, w, stride = payload.shape
    known = [(x - origin[0], y - origin[1], payload[y, x]) for y in range(h) for x in range(w)
             if not np.array_equal(bits(payload[y, x]), bits(np.asarray(unknown)[:stride]))]
    e = max(origin[0], w - origin[0], origin[1], h - origin[1])
    k_last = 0
    while 2 ** k_last < e:
        k_last += 1
    out = []
    for k in list(range(1, k_last + 1)) + [None]:
        blocks = {}
        for x, y, p in known:
            key = (0, 0) if k is None else (x >> k, y >> k)  # (Python's >> floors)
            cand = (-impact(p), x, y)
            if key not in blocks or cand < blocks[key][0]:
                blocks[key] = (cand, p)
        out.append({key: v[1] for key, v in blocks.items()})
    return out


def belief_impact(pkg, model, p):
    """the scorer's per-beam probability of a belief cell, restated (csrc/slamhip_internal.h)"""
    u, e, o, c = (float(v) for v in p)
    if model == pkg.CELL_CREDIBILIST:
        t0, t2 = u + e, o + c
        tot = ((t0 + 0.0) + t2) + 0.0
        return 1.0 - (1.0 - (0.0 if tot == 0.0 else t2 / tot))
    d_occ = abs(1.0 - o)
    t2, t3 = u + o, e + c
    tot = t2 + t3
    conflict = 0.0 if tot == 0.0 else t3 / tot
    unknown = u / 2.0
    return 1.0 - (unknown / 2 + (1 - unknown) * (conflict + d_occ) / 2.0)


def impact_of(pkg, m):
    """the impact brute_levels orders the cells of `m` by"""
    if m.cell_model == pkg.CELL_OCC:
        return (lambda p: 1.0 - abs(p[0] - 1.0)) if m.oie == pkg.OIE_DISCREPANCY else (lambda p: p[0])
    return lambda p: belief_impact(pkg, m.cell_model, p)


# ---- far from the world origin ------------------------------------------------------------------------------------------------
import placed_scenes as ps  # noqa: E402

FAR_MAPS = [64, 66, 67]  # 37 x 29, origin (11, 20), scale 0.1: GridCell, TBM, Credibilist
FAR_STATIONS = ps.ALL + ps.N_STATIONS
_far = {}


def moved_golden(i, station):
    """golden map i moved to a station of placed_scenes by placed_scenes.move_map's rule (a whole number of cells: the
    origin alone changes; these models hold no world coordinate in their payload), levels and all left behind"""
    m = golden_map(i)
    (kx, ky), _ = ps.station_entry(station)
    return types.SimpleNamespace(cell_model=m.cell_model, payload=m.payload, origin=(m.origin[0] - kx, m.origin[1] - ky), scale=m.scale,
                                 unknown=m.unknown, oie=m.oie, cls=m.cls, width=m.width, height=m.height)


def far_brute_levels(pkg, i, station):
    """brute_levels of moved_golden(i, station): made once, handed out unchanged"""
    if (i, station) not in _far:
        m = moved_golden(i, station)
        _far[(i, station)] = brute_levels(m.payload, m.origin, m.unknown, impact_of(pkg, m))
    return _far[(i, station)]


def expected_level_count(m):
    """ceil(log2(extent)) + 1, extent the largest distance in cells from the external axes to the window's far side"""
    extent = max(m.origin[0], m.width - m.origin[0], m.origin[1], m.height - m.origin[1])
    return (extent - 1).bit_length() + 1


# tests/golden/placed_pyramid.npz (make_golden_placed_pyramid.py): the compiled reference's levels and bounds at the N stations
_placed = None


def placed_golden():
    """placed_pyramid.npz, loaded when first asked for (the near-origin tests that import this module never do)"""
    global _placed
    if _placed is None:
        _placed = np.load(os.path.join(ROOT, "tests", "golden", "placed_pyramid.npz"))
    return _placed


def placed_counts():
    """(maps, bound sets) per station"""
    g = placed_golden()
    return int(g["N1_n_maps"]), int(g["N1_n_sets"])


def placed_lone_scene(station):
    """the whole match recorded at the station, as m3rsm_cases.golden_scene gives a scene of m3rsm.npz"""
    g, pre = placed_golden(), "lone_%s_" % station
    s = types.SimpleNamespace(name=str(g[pre + "name"]), cell_model=int(g[pre + "model"]), oie=int(g[pre + "oie"]), scale=float(g[pre + "scale"]),
                              origin=tuple(int(v) for v in g[pre + "origin"]), unknown=g[pre + "unknown"], payload=g[pre + "payload"],
                              pose=g[pre + "pose"], scan=g[pre + "scan"], limits=g[pre + "limits"], delta=g[pre + "delta"],
                              prob=float(g[pre + "prob"]), trace=g[pre + "trace"], station=station)
    s.height, s.width = s.payload.shape[:2]
    return s


def placed_raw_scene():
    """the edge scene matched under the reference's default (raw) trig provider at N1, as m3rsm_rawtrig_cases.golden_scene
    gives a scene of m3rsm_rawtrig.npz (without the cached provider's trace: its result and number of calls alone)"""
    g, pre = placed_golden(), "raw_"
    s = types.SimpleNamespace(name=str(g[pre + "name"]), cell_model=int(g[pre + "model"]), oie=int(g[pre + "oie"]), scale=float(g[pre + "scale"]),
                              origin=tuple(int(v) for v in g[pre + "origin"]), unknown=g[pre + "unknown"], payload=g[pre + "payload"],
                              pose=g[pre + "pose"], scan=g[pre + "scan"], angle=g[pre + "angle"], limits=g[pre + "limits"], delta=g[pre + "delta"],
                              prob=float(g[pre + "prob"]), trace=g[pre + "trace"], delta_cached=g[pre + "delta_cached"],
                              prob_cached=float(g[pre + "prob_cached"]), n_cached_calls=int(g[pre + "n_cached_calls"]),
                              libm_variant=int(g[pre + "libm_variant"]), station="N1")
    s.height, s.width = s.payload.shape[:2]
    return s


LONE_STATIONS = {"N1": "occ_square", "N2": "occ_1beam", "N3": "tbm_square"}


def placed_many_scene():
    """the many-to-many run whose requests stand at the origin, N1, N2 and N3, as m3rsm_many_cases.golden_scene gives a
    scene of m3rsm_many.npz: maps, requests (map, pose, scan), winner, delta, prob, trace, lone [K, 5]"""
    g = placed_golden()
    s = types.SimpleNamespace(name=str(g["many_name"]), oie=int(g["many_oie"]), limits=g["many_limits"], winner=int(g["many_winner"]),
                              delta=g["many_delta"], prob=float(g["many_prob"]), trace=g["many_trace"], lone=g["many_lone"], maps=[], requests=[])
    for j in range(int(g["many_n_maps"])):
        p = g["many_m%d_payload" % j]
        s.maps.append(types.SimpleNamespace(cell_model=int(g["many_model"]), payload=p, origin=tuple(int(v) for v in g["many_m%d_origin" % j]),
                                            scale=float(g["many_m%d_scale" % j]), unknown=g["many_m%d_unknown" % j], width=p.shape[1],
                                            height=p.shape[0]))
    for j in range(int(g["many_n_requests"])):
        s.requests.append(types.SimpleNamespace(map=int(g["many_r%d_map" % j]), pose=g["many_r%d_pose" % j], scan=g["many_r%d_scan" % j]))
    return s


def placed_golden_map(station, i):
    """golden_map for map i of a station of placed_pyramid.npz: the levels are the boxes the reference ever wrote"""
    PG = placed_golden()
    pre = "%s_m%d_" % (station, i)
    model, oie, scale, ox, oy, n = PG[pre + "meta"]
    m = types.SimpleNamespace(cell_model=int(model), payload=PG[pre + "payload"], origin=(int(ox), int(oy)), scale=float(scale),
                              unknown=PG[pre + "unknown"], oie=int(oie))
    m.height, m.width = m.payload.shape[:2]
    stride, at, m.levels = m.payload.shape[2], 0, []
    for (w, h, lox, loy), sc in zip(PG[pre + "Lgeo"], PG[pre + "Lscale"]):
        m.levels.append(dict(origin=(int(lox), int(loy)), scale=float(sc), payload=PG[pre + "Lflat"][at:at + w * h * stride].reshape(h, w, stride)))
        at += w * h * stride
    assert at == PG[pre + "Lflat"].size and len(m.levels) == int(n)
    return m


def placed_golden_set(station, j):
    PG = placed_golden()
    pre = "%s_s%d_" % (station, j)
    meta = PG[pre + "meta"]
    return types.SimpleNamespace(map=int(meta[0]), n_roots=int(meta[1]), pose=meta[2:5].copy(), limits=meta[5:10].copy(),
                                 scan=PG[pre + "scan"], cand=PG[pre + "cand"])


FAR_SET_OF = {64: 32, 66: 36, 67: 38}  # a golden match set (pose, 67-beam scan, 170 candidates with parents) per far map
ORACLE_MAPS = [64, 66]  # the cell models the oracle scores
_rows = {}


def moved_set(i, station):
    """(map, set): golden set FAR_SET_OF[i] at the station -- the base pose moved with the map, scan and candidates as
    they are"""
    s = golden_set(FAR_SET_OF[i])
    assert s.map == i
    m = moved_golden(i, station)
    s.pose = s.pose + ps.shift_m(station, m.scale)
    return m, s


def candidate_poses(base, rot, rect):
    """(x + c.x, y + c.y, rotation + theta) with c = LightWeightRectangle::center()"""
    cx = rect[:, 2] + (rect[:, 3] - rect[:, 2]) / 2
    cy = rect[:, 0] + (rect[:, 1] - rect[:, 0]) / 2
    return np.stack([base[0] + cx, base[1] + cy, rot + base[2]], axis=1)


def bound_probe_rows(pkg, po, oracle, i, station):
    """[9, 170]: the ORACLE's Max-OOPE score of every candidate of moved_set(i, station) on the level the candidate is
    scored on (the host build's, as a plain map of that scale and origin), at the candidate's pose and at its eight
    neighbours one ulp away in x and / or y -- placed_cases.probe, candidate by candidate since each has its own
    analysis area.  Row 0 is the strict-mode expectation; the rest measure the default mode's allowance.  Made once."""
    import placed_cases as pc
    if (i, station) not in _rows:
        m, s = moved_set(i, station)
        levels = [dict(origin=m.origin, scale=m.scale, payload=m.payload)] + pkg.pyramid_build_host(m, m.oie)
        plain = [po.GridMapData(m.cell_model, lv["payload"], lv["origin"], lv["scale"], m.unknown) for lv in levels]
        tab = po.ScanData(s.scan[:, 0], np.arange(s.scan.shape[0], dtype=np.float64), s.scan[:, 3], s.scan[:, 4], po.TRIG_CACHED, 0.0, 1.0,
                          np.ascontiguousarray(s.scan[:, 2]), np.ascontiguousarray(s.scan[:, 1]))
        rot, rect, level = s.cand[:, 0], s.cand[:, 1:5], s.cand[:, 7].astype(int)
        poses = candidate_poses(s.pose, rot, rect)
        cols = [pc.probe(oracle, plain[level[k]], tab, po.make_cfg(oope=po.OOPE_MAX, oie=m.oie, area=tuple(rect[k])), poses[k:k + 1])
                for k in range(len(rot))]
        _rows[(i, station)] = np.concatenate(cols, axis=1)
    return _rows[(i, station)]


def level_cells(level, unknown):
    """{(X, Y): payload} of the known cells of a level given as dict(origin, payload)"""
    p, o = level["payload"], level["origin"]
    stride = p.shape[2]
    return {(x - o[0], y - o[1]): p[y, x] for y in range(p.shape[0]) for x in range(p.shape[1])
            if not np.array_equal(bits(p[y, x]), bits(np.asarray(unknown)[:stride]))}


def assert_levels_are(levels, want, unknown):
    assert len(levels) == len(want)
    for lv, w in zip(levels, want):
        got = level_cells(lv, unknown)
        assert sorted(got) == sorted(w)
        for key in w:
            np.testing.assert_array_equal(bits(got[key]), bits(w[key]), err_msg=str(key))
