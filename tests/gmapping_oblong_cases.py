"""Shared by tests/golden/make_golden_gmapping_oblong.py, tests/test_oracle_gmapping_oblong.py (CPU) and
tests/test_gpu_gmapping_oblong.py (GPU): tests/golden/gmapping_oblong.npz -- the GMapping scorer of the compiled
reference on two windows that are NO squares (77 x 45 and 45 x 77 cells, unequal origin components), with end cells on,
next to and beyond every rim and corner.

A GROUP is one pose sequence scored by ONE scorer object (one OOPE cache, Q19), per map and per scan.  The poses of a rim
group are made per scan: an ANCHOR beam's end point is put into a target cell, at (0.37, 0.61) of its extent.
  rim_<side>      end cells with ix0 = 0 / width - 1 / iy0 = 0 / height - 1
  corner_<which>  the four corner cells
  in1_<side>      one cell inside a rim: where the mask form starts
  out_<side>      one and two cells outside
  far             far outside (every score is 0: no RIM group)
  inner           around the robot and next to walls inside (no RIM group)
Internal cells here are (ix, iy) = external cell + origin; a map's payload is [iy, ix]."""
import os

import numpy as np
from pyoracle import CELL_GMAPPING, TRIG_CACHED, GridMapData, ScanData

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gmapping_oblong.npz")
SCALE = 0.1
MAPS = {"wide": (77, 45), "tall": (45, 77)}
# robot's internal cell: >= 1 m from the world origin in both coordinates, |x| != |y|
ROBOT_CELL = {"wide": (51, 10), "tall": (11, 53)}
ROBOT_THETA = {"wide": np.deg2rad(100.0), "tall": np.deg2rad(-20.0)}
SCAN_SIZES = (1, 64, 65, 257, 1080)
SCANS = tuple("s%d" % n for n in SCAN_SIZES) + ("s1080c",)  # (the last one: 1080 beams behind the cached trig provider)
SIDES = ("left", "right", "bottom", "top")
CORNERS = ("bl", "br", "tl", "tr")
RIM_GROUPS = tuple("rim_" + s for s in SIDES) + tuple("corner_" + c for c in CORNERS) + \
    tuple("in1_" + s for s in SIDES) + tuple("out_" + s for s in SIDES)
INNER_GROUPS = ("inner",)
GROUPS = RIM_GROUPS + ("far",) + INNER_GROUPS
FRAC = (0.37, 0.61)       # where in its cell an anchor beam's end point lies
MARGIN_CELLS = 1e-6       # no end point of the golden lies closer to a cell boundary
WALL = 3                  # the room's walls lie this many cells inside the rims
SHORT = 0.012             # range of the beams 61 .. 66 and 253 .. 258: one run of equal end cells across 63 -> 64, 255 -> 256


def along(W, H):
    """three cells along the x rims, three along the y rims (none on a tile-friendly position)"""
    return (6, W // 2 + 2, W - 8), (5, H // 2 + 1, H - 7)


def group_targets(W, H):
    """group -> internal end cells (ix0, iy0) an anchor beam is aimed at"""
    xs, ys = along(W, H)
    t = {"rim_left": [(0, y) for y in ys], "rim_right": [(W - 1, y) for y in ys],
         "rim_bottom": [(x, 0) for x in xs], "rim_top": [(x, H - 1) for x in xs],
         "corner_bl": [(0, 0)], "corner_br": [(W - 1, 0)], "corner_tl": [(0, H - 1)], "corner_tr": [(W - 1, H - 1)],
         "in1_left": [(1, y) for y in ys], "in1_right": [(W - 2, y) for y in ys],
         "in1_bottom": [(x, 1) for x in xs], "in1_top": [(x, H - 2) for x in xs],
         "out_left": [(-1, ys[0]), (-2, ys[1]), (-1, ys[2])], "out_right": [(W, ys[0]), (W + 1, ys[1]), (W, ys[2])],
         "out_bottom": [(xs[0], -1), (xs[1], -2), (xs[2], -1)], "out_top": [(xs[0], H), (xs[1], H + 1), (xs[2], H)],
         "far": [(-400, 300), (W + 500, -200)]}
    return t


def single_cells(W, H):
    """(ix, iy, full) written one by one (RefMapHandle.update): full cells in the corners, along every rim and one cell
    inside it, a free cell between two full ones, pairs of full cells that touch only diagonally"""
    xs, ys = along(W, H)
    full = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)]
    for y in ys:
        full += [(0, y), (0, y + 1), (W - 1, y), (W - 1, y - 1), (1, y - 1), (W - 2, y + 1)]
    for x in xs:
        full += [(x, 0), (x + 1, 0), (x, H - 1), (x - 1, H - 1), (x - 1, 1), (x + 1, H - 2)]
    cx, cy = W // 2 - 9, H // 2 + 5
    full += [(cx, cy), (cx + 2, cy)]                       # ... a free cell between them
    full += [(cx + 7, cy - 3), (cx + 8, cy - 2)]           # neighbours only diagonally
    full += [(cx - 4, cy - 6), (cx - 5, cy - 5)]           # ... and on the other diagonal
    out = [(x, y, True) for x, y in full] + [(cx + 1, cy, False)]
    assert len(set((x, y) for x, y, _ in out)) == len(out)
    return out


def obstacle_of(ix, iy, origin):
    """the obstacle mean a single full cell gets: in its cell, off the centre, another offset for every cell"""
    fx = 0.5 + 0.43 * np.sin(1.7 * ix + 0.9 * iy)
    fy = 0.5 + 0.43 * np.cos(0.6 * ix - 2.3 * iy)
    return ((ix - origin[0] + fx) * SCALE, (iy - origin[1] + fy) * SCALE)


def cell_centre_frac(ix, iy, origin, frac=FRAC):
    return ((ix - origin[0] + frac[0]) * SCALE, (iy - origin[1] + frac[1]) * SCALE)


def anchored_poses(scan_range, scan_angle, targets, origin, salt):
    """two poses per target: beam b's end point at the target, b and the heading another one for every pose"""
    n = scan_range.size
    usable = np.nonzero(scan_range > 5 * SHORT)[0]
    out, anchors = [], []
    for k, (ix, iy) in enumerate(targets):
        for v in range(2):
            j = (7 * k + 3 * v + salt) % 5
            b = int(usable[(j * (usable.size - 1)) // 4])
            theta = -2.6 + 1.13 * ((5 * k + 2 * v + salt) % 6)
            tx, ty = cell_centre_frac(ix, iy, origin)
            a = theta + scan_angle[b]
            out.append((tx - scan_range[b] * np.cos(a), ty - scan_range[b] * np.sin(a), theta))
            anchors.append(b)
    assert n >= 1
    return np.array(out), np.array(anchors)


def inner_poses(name, origin, seed):
    """around the robot (the first two equal), then four poses in cells that touch a wall of the room"""
    W, H = MAPS[name]
    rs = np.random.RandomState(seed)
    rx, ry = cell_centre_frac(*ROBOT_CELL[name], origin, (0.5, 0.5))
    base = np.array([rx, ry, ROBOT_THETA[name]])
    p = base + rs.randn(4, 3) * [0.05, 0.05, 0.02]
    p[0] = p[1] = base + [0.013, -0.021, 0.004]
    xs, ys = along(W, H)
    hug = [(WALL + 1, ys[1]), (W - 2 - WALL, ys[0]), (xs[1], WALL + 1), (xs[2], H - 2 - WALL)]
    q = [cell_centre_frac(ix, iy, origin, (0.5, 0.5)) + (0.7 * k - 1.0,) for k, (ix, iy) in enumerate(hug)]
    return np.concatenate([p, np.array(q)])


# ---- the golden as objects ---------------------------------------------------------------------------------------------
_golden = None


def golden():
    global _golden
    if _golden is None:
        _golden = dict(np.load(GOLDEN))
    return _golden


def golden_map(g, name, pre=None):
    pre = pre or name + "_map_"
    return GridMapData(CELL_GMAPPING, g[pre + "payload"], g[pre + "origin"], float(g[pre + "scale"]), g[pre + "unknown"],
                       False)


def golden_scan(g, name, key):
    """scan `key` of map `name`; what both maps share (angles, weights, the cached provider's table) is kept once"""
    raw = key[:-1] if key.endswith("c") else key
    rng, (ang, w, f) = g["%s_%s_range" % (name, raw)], [g["wide_%s_%s" % (raw, k)] for k in ("angle", "weight", "factor")]
    if key.endswith("c"):
        pre = "wide_%s_" % key
        return ScanData(rng, ang, w, f, TRIG_CACHED, float(g[pre + "a_min"]), float(g[pre + "a_inc"]), g[pre + "tab_sin"],
                        g[pre + "tab_cos"])
    return ScanData(rng, ang, w, f)


def hc_scan(g, name):
    """what skip_rate 3 leaves of the 1080-beam scan (the generator asserts that the reference's filter leaves the same)"""
    return ScanData(g[name + "_s1080_range"][::3].copy(), g["wide_s1080_angle"][::3].copy())


def group_slices(g):
    at, out = 0, {}
    for grp, n in zip(GROUPS, g["group_len"].tolist()):
        out[grp] = slice(at, at + n)
        at += n
    return out


def all_poses(g, name, key):
    """every group's poses of (map, scan), GROUPS order (the cached scan is the same scan: the same poses)"""
    return g["%s_%s_poses" % (name, key[:-1] if key.endswith("c") else key)]


def group_poses(g, name, key, group):
    return all_poses(g, name, key)[group_slices(g)[group]]


def group_scores(g, name, key, group, th=0.1):
    """Ref.score over the group's poses by ONE scorer object, fullness_th 0.1 or 0.5"""
    return g["%s_%s_scores" % (name, key)][{0.1: 0, 0.5: 1}[th], group_slices(g)[group]]


def cases():
    """every (map, scan, group)"""
    return [(name, key, grp) for name in MAPS for key in SCANS for grp in GROUPS]


def pf_step(g, k):
    pre = "pf_step%d_" % k
    return dict(range=g[pre + "range"], angle=g["pf_step0_angle"], delta=g[pre + "delta"],
                resampled=bool(int(g[pre + "resampled"])), poses=g[pre + "poses"], weights=g[pre + "weights"],
                master=g[pre + "master"])


# ---- what an input reaches ---------------------------------------------------------------------------------------------
def end_cells(scan, poses, origin):
    """internal end cell [n_poses, n_beams, 2] of every beam at every pose (host arithmetic), and the smallest distance
    of an end point's coordinate from a cell boundary, in cells"""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    a = poses[:, 2:3] + scan.angle[None, :]
    q = np.stack([(poses[:, 0:1] + scan.range[None, :] * np.cos(a)) / SCALE,
                  (poses[:, 1:2] + scan.range[None, :] * np.sin(a)) / SCALE], axis=2)
    margin = float(np.min(np.abs(q - np.round(q)))) if q.size else 1.0
    return np.floor(q).astype(np.int64) + np.asarray(origin, dtype=np.int64), margin


def reaches(group, W, H, ec):
    """whether the end cells `ec` [..., 2] hold what `group` is there for"""
    ix, iy = ec[..., 0].ravel(), ec[..., 1].ravel()
    inx, iny = (ix >= 0) & (ix < W), (iy >= 0) & (iy < H)
    kind, _, which = group.partition("_")
    if kind in ("rim", "in1"):
        d = 0 if kind == "rim" else 1
        return bool({"left": (ix == d) & iny, "right": (ix == W - 1 - d) & iny, "bottom": (iy == d) & inx,
                     "top": (iy == H - 1 - d) & inx}[which].any())
    if kind == "corner":
        cx, cy = {"bl": (0, 0), "br": (W - 1, 0), "tl": (0, H - 1), "tr": (W - 1, H - 1)}[which]
        return bool(((ix == cx) & (iy == cy)).any())
    if kind == "out":
        one, two = {"left": (ix == -1, ix == -2), "right": (ix == W, ix == W + 1), "bottom": (iy == -1, iy == -2),
                    "top": (iy == H, iy == H + 1)}[which]
        ok = iny if which in ("left", "right") else inx
        return bool((one & ok).any() and (two & ok).any())
    if kind == "far":
        return bool(((ix < -100) | (ix > W + 100)).all())
    return bool((inx & iny).any())


def run_spans(ec, full, first, W, H):
    """whether some pose has ONE run of equal end cells across beams first -> first + 1 that starts before `first`, in a
    cell whose 3 x 3 window holds a full cell: the run's value is not 0, and the beams behind its first one would each
    have another value of their own"""
    if ec.shape[1] <= first + 1:
        return False
    for p in range(ec.shape[0]):
        c = ec[p]
        if not ((c[first - 1] == c[first]).all() and (c[first] == c[first + 1]).all()):
            continue
        ix, iy = c[first]
        if 1 <= ix < W - 1 and 1 <= iy < H - 1 and full[iy - 1:iy + 2, ix - 1:ix + 2].any():
            return True
    return False


def transposed(m, how):
    """`m` as an exchange of x and y somewhere would see it.  payload: the cells transposed (width and height with them),
    the origin's components kept; origin: the origin's components exchanged, nothing else; binding: width and height
    exchanged, the cells' memory as it is (a row is `height` cells long)"""
    if how == "payload":
        return GridMapData(m.cell_model, np.ascontiguousarray(m.payload.transpose(1, 0, 2)), m.origin, m.scale, m.unknown)
    if how == "origin":
        return GridMapData(m.cell_model, m.payload, (m.origin[1], m.origin[0]), m.scale, m.unknown)
    assert how == "binding"
    return GridMapData(m.cell_model, m.payload.reshape(m.width, m.height, -1), m.origin, m.scale, m.unknown)
