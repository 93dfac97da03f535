"""GPU suite: laser scans generated from resident maps (csrc/scan_generate.hip, slamhip_map_generate_scans).

Held to tests/golden/scan_generate.npz -- the scans of the compiled reference's LaserScanGenerator, with the libm variant
of the host that made them -- in both forms of the kernel (one wave per beam, one thread per beam), and to the host entry
generate_scans_host (the same per-beam routine, held to the same golden by tests/test_scan_generate_host.py) everywhere
else: a random map of every cell model, status-2 beams included; both libm variants; a map that a deferred update has
just changed.  Every comparison is exact."""
import os
import types

import numpy as np
import pytest

import __graft_entry__ as ge

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "scan_generate.npz"))
CALLS = [str(c) for c in G["calls"]]
VARIANT = int(G["sincos_variant"])  # (the build of sincos the generating host ran; its libm_variant is recorded too)
UNKNOWN = {0: [0.5], 1: [1.0, 0.0, 0.0, 0.0], 2: [-1.0, 0.0, 0.0], 3: [1.0, 0.0, 0.0, 0.0]}


@pytest.fixture(scope="module")
def pkg():
    return ge.load_package()


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def a_map(cell_model, payload, origin, scale, unknown):
    return types.SimpleNamespace(cell_model=cell_model, payload=payload, origin=tuple(int(v) for v in origin), scale=float(scale),
                                 unknown=np.asarray(unknown, dtype=np.float64), width=payload.shape[1], height=payload.shape[0])


def both_forms(ctx, map_id, *args, **kw):
    wave = ctx.generate_scans(map_id, *args, **kw)
    seq = ctx.generate_scans(map_id, *args, sequential=True, **kw)
    np.testing.assert_array_equal(wave[1], seq[1])
    np.testing.assert_array_equal(wave[0], seq[0])
    return wave


@pytest.mark.parametrize("c", CALLS)
def test_device_scans_equal_the_references(pkg, ctx, c):
    m = a_map(int(G[c + "_cell_model"]), G[c + "_payload"], G[c + "_origin"], G[c + "_scale"], G[c + "_unknown"])
    max_dist, fov, pts = G[c + "_lsp"]
    _, inc, hs = pkg.to_lsp(max_dist, fov, int(pts))
    angles = pkg.scan_gen_angles(hs, inc)
    ctx.upload_map(1, m)
    rng, status = both_forms(ctx, 1, G[c + "_poses"], angles, float(max_dist), float(G[c + "_threshold"]),
                             int(G[c + "_occ_kind"]), VARIANT)
    np.testing.assert_array_equal(status, G[c + "_status"])
    np.testing.assert_array_equal(rng, G[c + "_range"])
    ctx.map_release(1)


def random_map(rs, model, w, h):
    """10 % occupied cells, the rest free or never observed"""
    occ = rs.rand(h, w) < 0.10
    seen = rs.rand(h, w) < 0.7
    if model == 0:
        p = np.where(occ, 0.5 + 0.5 * rs.rand(h, w), np.where(seen, 0.3 * rs.rand(h, w), 0.5))[..., None]
    elif model == 2:
        p = np.zeros((h, w, 3))
        p[..., 0] = np.where(occ, 0.6 + 0.4 * rs.rand(h, w), np.where(seen, 0.2 * rs.rand(h, w), -1.0))
    else:
        o = np.where(occ, 0.5 + 0.5 * rs.rand(h, w), 0.1 * rs.rand(h, w))
        e = np.where(occ, 0.0, 0.8 * rs.rand(h, w))
        p = np.stack([1.0 - o - e, e, o, np.zeros((h, w))], axis=-1)
        p[~seen & ~occ] = [1.0, 0.0, 0.0, 0.0]
    return np.ascontiguousarray(p, dtype=np.float64)


# (model, occ_kind); 141 x 93 cells: rows that are no multiple of anything, walks of several 64-step rounds
@pytest.mark.parametrize("model,kind", [(0, 0), (1, 0), (1, 1), (2, 0), (3, 0)])
@pytest.mark.parametrize("variant", [0, 1])
def test_device_equals_the_host_routine_on_a_random_map(pkg, ctx, model, kind, variant):
    rs = np.random.RandomState(100 + 10 * model + kind)
    w, h, scale = 141, 93, 0.05
    m = a_map(model, random_map(rs, model, w, h), (50, 61), scale, UNKNOWN[model])
    ctx.upload_map(1, m)
    # poses anywhere (some outside the window), at cell centres (ties along axes and diagonals) and a hair beside them
    poses = np.column_stack([(rs.rand(24) * 1.3 - 0.15) * w * scale - 50 * scale, (rs.rand(24) * 1.3 - 0.15) * h * scale - 61 * scale,
                             rs.rand(24) * 6.3 - 3.15])
    cells = np.floor(poses[8:, :2] / scale)
    poses[8:16, :2] = (cells[:8] + 0.5) * scale
    poses[8:16, 2] = np.arctan2(rs.randint(-3, 4, 8), rs.randint(1, 4, 8))
    poses[16:, :2] = (cells[8:] + 0.5) * scale + rs.choice([3e-8, -3e-8, 1e-9, -1e-7], (8, 2))
    poses[16:, 2] = np.arctan2(rs.randint(-3, 4, 8), rs.randint(1, 4, 8))
    _, inc, hs = pkg.to_lsp(0, 360, 48)
    angles = pkg.scan_gen_angles(hs, inc)  # (starts at -pi: the robot's own heading is beam 24, the axes and diagonals are beams)
    for max_dist, thr in ((1.7, 0.5), (60.0, 0.55)):
        want = pkg.generate_scans_host(m, poses, angles, max_dist, thr, kind, variant)
        got = both_forms(ctx, 1, poses, angles, max_dist, thr, kind, variant)
        np.testing.assert_array_equal(got[1], want[1])
        np.testing.assert_array_equal(got[0], want[0])
        # (at threshold 0.5 a never-observed cell is a candidate: every beam ends in the robot's neighbourhood)
        assert np.any(want[1] == 1) and (thr == 0.5 or np.any(want[1] == 0))
    ctx.map_release(1)


def test_a_scan_generated_behind_a_deferred_update_sees_it(pkg, ctx):
    w, h, scale = 120, 120, 0.1
    m = a_map(0, np.full((h, w, 1), 0.5), (60, 60), scale, [0.5])
    ctx.upload_map(1, m)
    _, inc, hs = pkg.to_lsp(0, 270, 90)
    angles = pkg.scan_gen_angles(hs, inc)
    pose = np.array([0.053, 0.047, 0.2])
    before = ctx.generate_scans(1, [pose], angles, 30.0, 0.6, 0, VARIANT)
    assert not np.any(before[1] == 1)
    # a ring of obstacles 3 m away, appended without waiting for it
    c, s = pkg.beam_trig(angles)
    ctx.map_set_deferred(True)
    try:
        ctx.map_append_scan(1, pkg.RULE_MEAN, pose, np.full(angles.size, 3.0), c, s, None, quality=0.9)
        after = ctx.generate_scans(1, [pose], angles, 30.0, 0.6, 0, VARIANT)
        ctx.map_drain()
    finally:
        ctx.map_set_deferred(False)
    m.payload = ctx.map_download_window(1, 0, 0, w, h, 1)
    want = pkg.generate_scans_host(m, [pose], angles, 30.0, 0.6, 0, VARIANT)
    np.testing.assert_array_equal(after[1], want[1])
    np.testing.assert_array_equal(after[0], want[0])
    assert np.count_nonzero(after[1] == 1) > angles.size // 2
    ctx.map_release(1)


def test_bad_calls_are_refused_before_anything_is_launched(pkg, ctx):
    m = a_map(0, np.full((8, 8, 1), 0.5), (4, 4), 0.1, [0.5])
    ctx.upload_map(1, m)
    with pytest.raises(pkg.SlamHipError, match="cell boundary"):
        ctx.generate_scans(1, [[0.2, 0.13, 0.0]], [0.0], 1.0, 0.6, 0, VARIANT)
    with pytest.raises(pkg.SlamHipError):
        ctx.generate_scans(1, [[0.23, 0.13, 0.0]], [0.0], 1.0, 0.6, 1, VARIANT)
    with pytest.raises(pkg.SlamHipError):
        ctx.generate_scans(1, [[0.23, 0.13, 0.0]], [0.0], 1e9, 0.6, 0, VARIANT)
    with pytest.raises(pkg.SlamHipError):
        ctx.generate_scans(7, [[0.23, 0.13, 0.0]], [0.0], 1.0, 0.6, 0, VARIANT)
    ctx.map_release(1)
