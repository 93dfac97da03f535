"""Scenes of tests/test_gpu_particle_score.py (slamhip_gmapping_particle_score_poses): a random GMAPPING map of 2 x 2
tiles whose full cells hold their obstacle mean at a seeded random point INSIDE the cell (the maps of
tests/scan_tiled_scenes.py have zero obstacle means: every value of the GMapping OOPE over them is exp(-|end point|^2 /
0.05)), its scans and poses, and a numpy restatement of what a 3 x 3 window sees, for the conditions that keep the
tests from passing vacuously.  (No test in here.)

Cells: occupied ones hold 0.6 .. 1.0, observed free ones 0 .. 0.05, the rest the never-observed -1; one quadrant is
never observed, so the pool points it at the shared unknown tile.  Thresholds: 0.1 (the filter's own: the tiles' masks
are valid for it; every occupied cell is full) and 0.8 (another one: the nine-cell path; about half of them are)."""
import types

import numpy as np

TILE = 128
W = H = 2 * TILE
SCALE = 0.05
UNKNOWN = np.array([-1.0, 0.0, 0.0])
CENTRE = (TILE, TILE)
UNKNOWN_QUADRANT = (1, 1)  # (tile x, tile y)
TH_FILTER, TH_OTHER = 0.1, 0.8
SEED_MAP, SEED_SCANS, SEED_POSES = 4711, 4712, 4713  # (picked so that the conditions check_conditions asserts hold)
SCAN_LENGTHS = (1, 90, 256, 257)  # 256 | 257: one block of 256 beams | two


def a_map(payload, origin):
    return types.SimpleNamespace(cell_model=2, payload=np.ascontiguousarray(payload), origin=tuple(int(v) for v in origin),
                                 scale=SCALE, unknown=UNKNOWN.copy(), width=payload.shape[1], height=payload.shape[0])


def window_map(payload3, x0, y0):
    """a downloaded EXTERNAL window [x0, ..) x [y0, ..) of a particle's map as a flat map"""
    return a_map(payload3, (-x0, -y0))


def gm_map(frac=0.15, origin=CENTRE):
    rs = np.random.RandomState(SEED_MAP)
    occ = rs.rand(H, W) < frac
    seen = rs.rand(H, W) < 0.7
    ys, xs = np.mgrid[0:H, 0:W]
    p = np.zeros((H, W, 3))
    p[..., 0] = np.where(occ, 0.6 + 0.4 * rs.rand(H, W), np.where(seen, 0.05 * rs.rand(H, W), -1.0))
    # the obstacle mean of a full cell: a point inside the cell, in world coordinates
    p[..., 1] = np.where(occ, (xs - origin[0] + 0.05 + 0.9 * rs.rand(H, W)) * SCALE, 0.0)
    p[..., 2] = np.where(occ, (ys - origin[1] + 0.05 + 0.9 * rs.rand(H, W)) * SCALE, 0.0)
    tx, ty = UNKNOWN_QUADRANT
    p[ty * TILE:(ty + 1) * TILE, tx * TILE:(tx + 1) * TILE] = UNKNOWN
    return a_map(p, origin)


def a_scan(rng, ang, weight, factor):
    f = lambda a: np.ascontiguousarray(a, dtype=np.float64)  # noqa: E731
    return types.SimpleNamespace(range=f(rng), angle=f(ang), weight=f(weight), factor=f(factor))


def scans():
    """one scan per length of SCAN_LENGTHS: points 0.3 .. 3 m away all around, uneven weights and factors"""
    rs = np.random.RandomState(SEED_SCANS)
    out = []
    for n in SCAN_LENGTHS:
        ang = np.linspace(-np.pi, np.pi, n, endpoint=False) + 0.01 * rs.rand(n)
        out.append(a_scan(0.3 + 2.7 * rs.rand(n), ang, 0.5 + rs.rand(n), 0.5 + 0.5 * rs.rand(n)))
    return out


def carry_scan(n=40):
    """a scan whose last point repeats its first point's range and angle: a pose's last beam ends where its first does"""
    rs = np.random.RandomState(SEED_SCANS + 1)
    ang = np.linspace(-np.pi, np.pi, n, endpoint=False)
    rng = 0.5 + 2.0 * rs.rand(n)
    ang[-1], rng[-1] = ang[0], rng[0]
    return a_scan(rng, ang, 0.5 + rs.rand(n), np.ones(n))


def random_poses(n, seed=SEED_POSES, reach=0.97):
    """anywhere over the 2 x 2 tiles (12.8 m a side): near the rim a scan's end points leave the extent"""
    rs = np.random.RandomState(seed)
    half = reach * TILE * SCALE
    return np.column_stack([(2 * rs.rand(n) - 1) * half, (2 * rs.rand(n) - 1) * half, rs.rand(n) * 6.3 - 3.15])


def seam_poses(scan, n, seed=SEED_POSES + 1):
    """poses whose FIRST end point lies within 2 cells of a tile seam (external x = 0 or y = 0), in the observed tiles"""
    rs = np.random.RandomState(seed)
    near = (rs.rand(n) * 4.0 - 2.0) * SCALE
    along = -(0.05 + 0.9 * rs.rand(n)) * TILE * SCALE  # (the negative side: away from the never-observed quadrant)
    on_x = np.arange(n) % 2 == 0
    ex, ey = np.where(on_x, near, along), np.where(on_x, along, near)
    th = rs.rand(n) * 6.3 - 3.15
    r, a = scan.range[0], scan.angle[0]
    return np.column_stack([ex - r * np.cos(th + a), ey - r * np.sin(th + a), th])


def poses_ending_at(scan, points, seed=SEED_POSES + 2):
    """poses, one per point (x, y), whose FIRST end point is that point"""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    th = np.random.RandomState(seed).rand(points.shape[0]) * 6.3 - 3.15
    r, a = scan.range[0], scan.angle[0]
    return np.column_stack([points[:, 0] - r * np.cos(th + a), points[:, 1] - r * np.sin(th + a), th])


def window_view(m, scan, poses, th, extent):
    """What the 3 x 3 window of every (pose, beam) sees in the flat map m, restated in numpy (statistics only: the last
    bit of an end point does not matter here).  extent: (x0, y0, x1, y1), the pool's extent in external cells.
    Returns (nonzero[P, B]: a full cell in the window, i.e. a value above 0; other_tile[P, B]: the best full cell lies in
    another tile than the centre cell; outside[P, B]: the end point's cell lies outside the extent)."""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    a = poses[:, 2:3] + scan.angle[None, :]
    wx = poses[:, 0:1] + scan.range[None, :] * np.cos(a)
    wy = poses[:, 1:2] + scan.range[None, :] * np.sin(a)
    cx, cy = np.floor(wx / SCALE).astype(np.int64), np.floor(wy / SCALE).astype(np.int64)
    best = np.full(wx.shape, np.inf)
    bdx, bdy = np.zeros(wx.shape, np.int64), np.zeros(wx.shape, np.int64)
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            ix, iy = cx + dx + m.origin[0], cy + dy + m.origin[1]
            inb = (ix >= 0) & (ix < m.width) & (iy >= 0) & (iy < m.height)
            cell = m.payload[np.clip(iy, 0, m.height - 1), np.clip(ix, 0, m.width - 1)]
            full = inb & (cell[..., 0] >= th)
            d2 = np.where(full, (cell[..., 1] - wx) ** 2 + (cell[..., 2] - wy) ** 2, np.inf)
            better = d2 < best
            best = np.where(better, d2, best)
            bdx, bdy = np.where(better, dx, bdx), np.where(better, dy, bdy)
    nonzero = np.isfinite(best)
    other_tile = nonzero & (((cx + bdx) // TILE != cx // TILE) | ((cy + bdy) // TILE != cy // TILE))
    x0, y0, x1, y1 = extent
    outside = (cx < x0) | (cx >= x1) | (cy < y0) | (cy >= y1)
    return nonzero, other_tile, outside


def check_conditions(views, what):
    """views: window_view results of every job of a scene -- at least 20 % of the (pose, beam) values above 0 and at
    least 20 % equal to 0, a best full cell across a tile seam, an end point outside the extent"""
    nz = np.concatenate([v[0].ravel() for v in views])
    assert nz.size > 0, what
    assert nz.mean() >= 0.2 and (~nz).mean() >= 0.2, (what, nz.mean())
    assert sum(int(v[1].sum()) for v in views) >= 1, what + ": no window whose best cell lies across a seam"
    assert sum(int(v[2].sum()) for v in views) >= 1, what + ": no end point outside the extent"
