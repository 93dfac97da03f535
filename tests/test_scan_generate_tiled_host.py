"""CPU suite: scan generation over a tile table on the host (slamhip_scan_generate_host_tiled -- the per-beam routine of
csrc/scan_generate_device.h over an SgTiledMap, the map type the kernels of slamhip_gmapping_particle_generate_scans
read) against the same routine over the flat map (slamhip_scan_generate_host, held to the compiled reference's scans by
tests/test_scan_generate_host.py).  A random GMAPPING map of 2 x 2 tiles is cut into a pool -- tile 0 the unknown tile, the
private tiles in a shuffled order, one quadrant never observed and pointed at tile 0 while the tile it would have had
holds occupied cells -- and both must give the same status bytes and ranges, bit for bit, in both sincos variants.

The conditions the scenes have to meet are asserted on the FLAT map's results, so that a change of scene cannot hollow the
comparison out.  One of them cannot hold: with occ_threshold -2.0 EVERY cell is a candidate, the cells outside the extent
too, so the cell after the robot's own (whose bounds the ray meets once: a touch) is crossed by the ray and ends the beam
-- no beam has status 0 there, whatever the seed (none among 216 000 beams of 100 seeds).  At that threshold the test
asserts what it is run for instead: hits and no status 0, every beam decided within two cells, also from the poses that
stand outside the extent."""
import os

import numpy as np
import pytest
import scan_tiled_scenes as S

import __graft_entry__ as ge


@pytest.fixture(scope="module")
def pkg():
    p = ge.load_package()
    if not os.path.exists(p.LIB_PATH):
        p.build()
    return p


def same(got, want):
    np.testing.assert_array_equal(got[1], want[1])
    np.testing.assert_array_equal(got[0], want[0])


def tiled(pkg, m, pool, table, poses, angles, max_dist, thr, variant):
    return pkg.generate_scans_host_tiled(pool, table, m.origin, m.scale, poses, angles, max_dist, thr, m.unknown[0], variant)


@pytest.fixture(scope="module")
def dense(pkg):
    m, poses, angles, max_dist, thrs = S.dense_scene(pkg)
    pool, table = S.cut_into_pool(m, np.random.RandomState(7))
    flat = {(t, v): pkg.generate_scans_host(m, poses, angles, max_dist, t, 0, v) for t in thrs for v in (0, 1)}
    return m, poses, angles, max_dist, thrs, pool, table, flat


@pytest.fixture(scope="module")
def sparse(pkg):
    m, poses, angles, max_dist, thr = S.sparse_scene(pkg)
    pool, table = S.cut_into_pool(m, np.random.RandomState(8))
    flat = {v: pkg.generate_scans_host(m, poses, angles, max_dist, thr, 0, v) for v in (0, 1)}
    return m, poses, angles, max_dist, thr, pool, table, flat


def test_the_pool_is_the_cut_the_file_describes(dense):
    m, pool, table = dense[0], dense[5], dense[6]
    tx, ty = S.UNKNOWN_QUADRANT
    assert pool.shape == (5, 128 * 128, 4) and table.shape == (2, 2)
    assert table[ty, tx] == 0 and sorted(table.ravel()) != list(table.ravel())  # (shuffled: not in reading order)
    assert len(set(table.ravel())) == 4 and np.all(pool[0, :, 0] == -1.0)
    unused = (set(range(1, 5)) - set(table.ravel().tolist())).pop()
    assert np.all(pool[unused, :, 0] == 0.99)
    assert np.all(m.payload[ty * 128:(ty + 1) * 128, tx * 128:(tx + 1) * 128, 0] == -1.0)


def test_the_dense_scene_holds_its_cases(dense):
    m, poses, angles, max_dist, thrs, _, _, flat = dense
    assert poses.shape == (24, 3) and angles.size == 90 and max_dist == 4.0 and thrs == (0.8, 0.0, -2.0)
    occupied = m.payload[..., 0][m.payload[..., 0] >= 0.6]
    assert abs(occupied.size / (S.W * S.H) - 0.10 * 0.75) < 0.01 and occupied.min() < thrs[0] < occupied.max()
    cell = np.floor(poses[:, :2] / S.SCALE) + np.array(m.origin)
    outside = np.any((cell < 0) | (cell >= S.W), axis=1)
    assert 2 <= np.count_nonzero(outside) <= 12
    for (t, v), (rng, st) in flat.items():
        assert np.any(st == 1), (t, v)
        if t > -2.0:
            assert np.any(st == 0), (t, v)
        else:
            # (every cell is a candidate: see the file's docstring)
            assert not np.any(st == 0) and np.all(rng < 2 * S.SCALE) and np.all(np.any(st[outside] == 1, axis=1))


def test_the_sparse_scene_holds_its_cases(sparse):
    m, poses, angles, max_dist, thr, _, _, flat = sparse
    assert poses.shape == (12, 3) and angles.size == 120 and max_dist == 9.0
    seam = np.minimum(np.abs(poses[:, 0]), np.abs(poses[:, 1])) / S.SCALE
    assert np.all(seam <= 6.0)
    for v, (rng, st) in flat.items():
        hit = st == 1
        assert hit.mean() >= 0.10 and (~hit).mean() >= 0.10
        # the hit, or the end of a beam without one, more than 128 cells from the robot
        far = np.where(hit, rng / S.SCALE > 128, max_dist / S.SCALE > 128)
        assert far.mean() >= 0.20 and np.any(hit & (rng / S.SCALE > 128))
        a = angles[None, :] + poses[:, 2:3]
        hx, hy = poses[:, 0:1] + rng * np.cos(a), poses[:, 1:2] + rng * np.sin(a)

        def tile_of(x, y):
            return (np.floor(x / S.SCALE) + m.origin[0]) // 128 + 2 * ((np.floor(y / S.SCALE) + m.origin[1]) // 128)
        assert np.any(hit & (tile_of(hx, hy) != tile_of(poses[:, 0:1], poses[:, 1:2])))


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("thr", [0.8, 0.0, -2.0])
def test_tiled_equals_flat_on_the_dense_scene(pkg, dense, thr, variant):
    m, poses, angles, max_dist, _, pool, table, flat = dense
    same(tiled(pkg, m, pool, table, poses, angles, max_dist, thr, variant), flat[thr, variant])


@pytest.mark.parametrize("variant", [0, 1])
def test_tiled_equals_flat_on_the_sparse_scene(pkg, sparse, variant):
    m, poses, angles, max_dist, thr, pool, table, flat = sparse
    same(tiled(pkg, m, pool, table, poses, angles, max_dist, thr, variant), flat[variant])


def test_an_origin_other_than_the_centre(pkg, dense):
    m, poses, angles, max_dist, _, pool, table, _ = dense
    moved = S.a_map(m.payload, (100, 61))
    shift = (np.array(m.origin) - np.array(moved.origin)) * S.SCALE  # the same places of the map, other coordinates
    p = poses + np.array([shift[0], shift[1], 0.0])
    for thr in (0.8, -2.0):
        want = pkg.generate_scans_host(moved, p, angles, max_dist, thr, 0, 1)
        assert np.any(want[1] == 1)
        same(tiled(pkg, moved, pool, table, p, angles, max_dist, thr, 1), want)


def test_the_default_variant_is_this_hosts(pkg, sparse):
    m, poses, angles, max_dist, thr, pool, table, flat = sparse
    v = pkg.scan_gen_libm_variant(strict=False)
    if v >= 0:
        same(pkg.generate_scans_host_tiled(pool, table, m.origin, m.scale, poses[:2], angles, max_dist, thr),
             (flat[v][0][:2], flat[v][1][:2]))


def test_bad_calls_are_refused(pkg, dense):
    m, poses, angles, max_dist, _, pool, table, _ = dense
    for bad in (-1, 5):
        t = table.copy()
        t[1, 0] = bad
        with pytest.raises(pkg.SlamHipError, match="table entry"):
            tiled(pkg, m, pool, t, poses, angles, max_dist, 0.8, 0)
    with pytest.raises(pkg.SlamHipError, match="null pool"):
        tiled(pkg, m, None, table, poses, angles, max_dist, 0.8, 0)
    with pytest.raises(pkg.SlamHipError, match="null pool or table"):
        tiled(pkg, m, pool, None, poses, angles, max_dist, 0.8, 0)
    with pytest.raises(pkg.SlamHipError, match="variant"):
        tiled(pkg, m, pool, table, poses, angles, max_dist, 0.8, 2)
    # the flat entry's refusals: the opening assertion, a NaN angle, a beam longer than 2^20 cells
    with pytest.raises(pkg.SlamHipError, match="cell boundary"):
        tiled(pkg, m, pool, table, [[0.2, 0.13, 0.0]], angles, max_dist, 0.8, 0)
    with pytest.raises(pkg.SlamHipError):
        tiled(pkg, m, pool, table, poses, [0.0, np.nan], max_dist, 0.8, 0)
    with pytest.raises(pkg.SlamHipError):
        tiled(pkg, m, pool, table, poses, angles, 1e9, 0.8, 0)
    # ... and a valid call after them is served
    same(tiled(pkg, m, pool, table, poses[:1], angles, max_dist, 0.8, 0), pkg.generate_scans_host(m, poses[:1], angles, max_dist, 0.8, 0, 0))
    empty = tiled(pkg, m, pool, table, np.zeros((0, 3)), angles, max_dist, 0.8, 0)
    assert empty[0].shape == (0, 90)
