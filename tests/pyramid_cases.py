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
