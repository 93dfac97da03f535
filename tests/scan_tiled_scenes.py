"""Scenes shared by tests/test_scan_generate_tiled_host.py (no GPU) and tests/test_gpu_particle_scan_generate.py: a random
GMAPPING map of 2 x 2 tiles, its poses and beams, and the map cut into a tile pool in host memory.  (No test in here.)

The map recipe is random_map(model=2) of tests/test_gpu_scan_generate.py with the occupied fraction as a parameter:
occupied cells hold 0.6 .. 1.0, observed free ones 0 .. 0.2, the rest the never-observed -1."""
import types

import numpy as np

TILE = 128
W = H = 2 * TILE
SCALE = 0.05
UNKNOWN = np.array([-1.0, 0.0, 0.0])
CENTRE = (TILE, TILE)
UNKNOWN_QUADRANT = (1, 1)  # (tile x, tile y) left never observed: the pool points it at the shared unknown tile
SEED_DENSE, SEED_SPARSE = 411, 412  # (picked so that the conditions test_scan_generate_tiled_host.py asserts hold)


def a_map(payload, origin):
    return types.SimpleNamespace(cell_model=2, payload=payload, origin=tuple(int(v) for v in origin), scale=SCALE,
                                 unknown=UNKNOWN.copy(), width=payload.shape[1], height=payload.shape[0])


def gm_map(rs, frac, origin=CENTRE):
    occ = rs.rand(H, W) < frac
    seen = rs.rand(H, W) < 0.7
    p = np.zeros((H, W, 3))
    p[..., 0] = np.where(occ, 0.6 + 0.4 * rs.rand(H, W), np.where(seen, 0.2 * rs.rand(H, W), -1.0))
    tx, ty = UNKNOWN_QUADRANT
    p[ty * TILE:(ty + 1) * TILE, tx * TILE:(tx + 1) * TILE, 0] = -1.0
    return a_map(np.ascontiguousarray(p), origin)


def dense_scene(pkg):
    """(map, 24 poses, 90 angles, max_dist, thresholds): 10 % occupied; poses anywhere (some outside the extent), at cell
    centres (ties along axes and diagonals) and a hair beside them, as in tests/test_gpu_scan_generate.py"""
    rs = np.random.RandomState(SEED_DENSE)
    m = gm_map(rs, 0.10)
    ox, oy = m.origin
    poses = np.column_stack([(rs.rand(24) * 1.3 - 0.15) * W * SCALE - ox * SCALE, (rs.rand(24) * 1.3 - 0.15) * H * SCALE - oy * SCALE,
                             rs.rand(24) * 6.3 - 3.15])
    cells = np.floor(poses[8:, :2] / SCALE)
    poses[8:16, :2] = (cells[:8] + 0.5) * SCALE
    poses[8:16, 2] = np.arctan2(rs.randint(-3, 4, 8), rs.randint(1, 4, 8))
    poses[16:, :2] = (cells[8:] + 0.5) * SCALE + rs.choice([3e-8, -3e-8, 1e-9, -1e-7], (8, 2))
    poses[16:, 2] = np.arctan2(rs.randint(-3, 4, 8), rs.randint(1, 4, 8))
    _, inc, hs = pkg.to_lsp(0, 360, 90)
    # (0.8 lies inside the occupied cells' 0.6 .. 1.0; at 0.0 every observed cell is a candidate; at -2.0 every cell is,
    # those outside the extent too)
    return m, poses, pkg.scan_gen_angles(hs, inc)[:90], 4.0, (0.8, 0.0, -2.0)


def sparse_scene(pkg):
    """(map, 12 poses, 120 angles, max_dist, threshold): 0.2 % occupied, poses within 6 cells of the tile seams at
    virtual x = 128 or y = 128 (external 0); walks of up to ~250 cells that cross seams and leave the extent"""
    rs = np.random.RandomState(SEED_SPARSE)
    m = gm_map(rs, 0.002)
    near = (rs.rand(12) * 12.0 - 6.0) * SCALE   # within 6 cells of a seam
    along = (rs.rand(12) * 0.9 - 0.45) * W * SCALE  # anywhere along it
    on_x = np.arange(12) % 2 == 0
    poses = np.column_stack([np.where(on_x, near, along), np.where(on_x, along, near), rs.rand(12) * 6.3 - 3.15])
    _, inc, hs = pkg.to_lsp(0, 360, 120)
    return m, poses, pkg.scan_gen_angles(hs, inc)[:120], 9.0, 0.5


def cut_into_pool(m, rs):
    """The flat map as (pool[5, 16384, 4], table[2, 2]): tile 0 the unknown tile, tiles 1 .. 4 in a shuffled order; the
    never-observed quadrant points at tile 0 and the tile it would have had holds occupied cells nobody may read."""
    pool = np.zeros((5, TILE * TILE, 4))
    pool[0, :, 0] = UNKNOWN[0]
    table = np.zeros((2, 2), dtype=np.int32)
    ids = 1 + rs.permutation(4)
    for k, (ty, tx) in enumerate([(0, 0), (0, 1), (1, 0), (1, 1)]):
        if (tx, ty) == UNKNOWN_QUADRANT:
            pool[ids[k], :, 0] = 0.99
            continue
        pool[ids[k], :, :3] = m.payload[ty * TILE:(ty + 1) * TILE, tx * TILE:(tx + 1) * TILE].reshape(-1, 3)
        table[ty, tx] = ids[k]
    return pool, table


def window_map(payload3, x0, y0):
    """a downloaded EXTERNAL window [x0, ..) x [y0, ..) of a particle's map as the host routine's flat map"""
    return a_map(np.ascontiguousarray(payload3), (-x0, -y0))
