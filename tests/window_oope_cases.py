"""Shared by tests/test_window_oope_golden.py, tests/test_gpu_window_oope.py and tests/golden/make_golden_window_oope.py:
tests/golden/window_oope.npz -- the window observation-probability estimators (max / mean / overlap) of the compiled
reference on oblong, off-centre, empty (line, point, underflowing) and rim-crossing analysis areas -- as objects, the
re-centring of an analysis area, and the margin of a coordinate from the nearest cell boundary."""
import os

import numpy as np
from pyoracle import TRIG_CACHED, TRIG_RAW, GridMapData, ScanData

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "window_oope.npz")
MAPS = ("occ10", "occ07", "tbm10")  # 23 x 17 cells, origin (11, 8): GridCell at 0.1 and 0.07, TBM at 0.1
SCAN_MAPS = ("occ10", "tbm10")
SCAN_SIZES = (1, 65, 257)
OOPES = (("max", 1), ("mean", 2), ("overlap", 3))  # OOPE_MAX, OOPE_MEAN, OOPE_OVERLAP
TRIGS = (("raw", TRIG_RAW), ("cached", TRIG_CACHED))
MARGIN_CELLS = 1e-9


def load_golden():
    return dict(np.load(GOLDEN))


def golden_map(g, name):
    pre = name + "_map_"
    return GridMapData(int(g[pre + "cell_model"]), g[pre + "payload"], g[pre + "origin"], float(g[pre + "scale"]),
                       g[pre + "unknown"], bool(int(g[pre + "bounded"])))


def golden_scan(g, n, trig):
    """the n-beam scan of the scan-level part behind the raw or the cached trig provider"""
    pre = "scan%d_" % n
    if trig == TRIG_CACHED:
        return ScanData(g[pre + "range"], g[pre + "angle"], g[pre + "weight"], g[pre + "factor"], TRIG_CACHED,
                        float(g[pre + "a_min"]), float(g[pre + "a_inc"]), g[pre + "tab_sin"], g[pre + "tab_cos"])
    return ScanData(g[pre + "range"], g[pre + "angle"], g[pre + "weight"], g[pre + "factor"])


def recentred(area, x, y):
    """LightWeightRectangle::move_center: (bot, top, left, right) of `area` around (x, y).  The half extents come from
    the un-centred area; re-centring a centred rectangle again differs in the last ulp."""
    half_v, half_h = (area[1] - area[0]) / 2, (area[3] - area[2]) / 2
    return np.array([y - half_v, y + half_v, x - half_h, x + half_h])


def boundary_margin(v, scale):
    """distance of the coordinates v from the nearest cell boundary, in cells"""
    q = np.asarray(v, dtype=np.float64) / scale
    return np.abs(q - np.round(q))


def area_margin(points, area, scale):
    """the smallest boundary_margin over the points' coordinates and the edges of `area` re-centred on each of them"""
    x, y = points[:, 0], points[:, 1]
    half_v, half_h = (area[1] - area[0]) / 2, (area[3] - area[2]) / 2
    edges = np.stack([x, y, x - half_h, x + half_h, y - half_v, y + half_v])
    return float(np.min(boundary_margin(edges, scale)))


def end_points(scan, poses):
    """[n_poses * n_beams, 2]: every beam's end point at every pose, in host arithmetic"""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    a = poses[:, 2:3] + scan.angle[None, :]
    x = poses[:, 0:1] + scan.range[None, :] * np.cos(a)
    y = poses[:, 1:2] + scan.range[None, :] * np.sin(a)
    return np.stack([x.ravel(), y.ravel()], axis=1)
