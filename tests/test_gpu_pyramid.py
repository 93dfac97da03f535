"""GPU suite (-m gpu): the max-impact map pyramid and the per-candidate bound scorer on the device (csrc/map_pyramid.hip)
against the host build of the same definition, the goldens of the compiled reference (tests/golden/pyramid.npz) and
slamhip_score_poses on the levels' own map ids.  Levels, refreshes and bounds are compared bit for bit; the bounds agree
with the reference's Match::prob_upper_bound within the windowed-scorer parity bars of tests/test_gpu_parity.py."""
import numpy as np
import pytest
from pyramid_cases import N_MAPS, N_SETS, assert_same_level, bits, golden_map, golden_set

import __graft_entry__ as ge

pytestmark = pytest.mark.gpu

# tests/test_gpu_parity.py::test_window_oopes_vs_reference, `max` OOPE: beam-order sum + host pose trig is bit-exact with
# the reference, the default mode (canonical tree sum, device sincos) within 1e-12 relative
STRICT = dict(sum_order=1, pose_trig=1)
DEFAULT_RTOL = 1e-12
FINE, FIRST = 0, 1  # map ids: the fine map, the first level


@pytest.fixture(scope="module")
def pkg():
    return ge.load_package()


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def download_levels(ctx, pyr, stride):
    return [dict(origin=lv["origin"], scale=lv["scale"], map_id=lv["map_id"],
                 payload=ctx.map_download_window(lv["map_id"], 0, 0, lv["width"], lv["height"], stride)) for lv in pyr.info()]


def assert_levels_equal(a, b):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b), 1):
        assert x["origin"] == y["origin"] and x["scale"] == y["scale"], k
        np.testing.assert_array_equal(bits(x["payload"]), bits(y["payload"]), err_msg="level %d" % k)


def test_device_levels_equal_the_host_build_and_the_reference(pkg, ctx):
    for i in range(N_MAPS):
        m = golden_map(i)
        ctx.upload_map(FINE, m)
        pyr = pkg.Pyramid(ctx, FINE, m.oie, FIRST)
        got = download_levels(ctx, pyr, pkg.STRIDE[m.cell_model])
        host = pkg.pyramid_build_host(m, m.oie)
        assert [lv["map_id"] for lv in got] == list(range(FIRST, FIRST + len(host)))
        assert_levels_equal(got, host)  # geometry and payload, bit for bit
        assert len(got) == len(m.levels)
        for k, (lv, want) in enumerate(zip(got, m.levels), 1):
            assert lv["scale"] == want["scale"]
            assert_same_level(lv["payload"], lv["origin"], want["payload"], want["origin"], m.unknown, "map %d level %d" % (i, k))
            info = ctx.map_info(lv["map_id"])  # an ordinary bound map of the fine map's model
            assert info["cell_model"] == m.cell_model and info["scale"] == lv["scale"] and info["origin"] == lv["origin"]
        pyr.close()
        ctx.map_release(FINE)


@pytest.mark.parametrize("i", [64, 66, 67])  # 37 x 29, origin (11, 20), scale 0.1: GridCell, TBM, Credibilist
def test_refresh_of_a_window_equals_rebuild(pkg, ctx, i):
    m = golden_map(i)
    assert (m.width, m.height, m.origin) == (37, 29, (11, 20))
    stride = pkg.STRIDE[m.cell_model]
    ctx.upload_map(FINE, m)
    pyr = pkg.Pyramid(ctx, FINE, m.oie, FIRST)
    before = download_levels(ctx, pyr, stride)
    top = before[-1]["payload"][0, 0]
    # the cell the whole map's maximum comes from goes DOWN to the smallest known payload of the map; cells at block
    # corners of every level (external -16, -8, -1, 0, 7, 8, 15, 16), cells at negative external coordinates, a cell
    # that becomes unknown again
    known = ~np.all(bits(m.payload) == bits(m.unknown), axis=-1)
    donors = m.payload[known]
    low = np.array([1.0 / 1024]) if stride == 1 else np.array([0.1, 0.9, 0.0, 0.0])  # an impact below every donor's
    tops = [(int(x), int(y)) for y, x in np.argwhere(np.all(bits(m.payload) == bits(top), axis=-1))]
    ext = [(-8, -8), (-1, -1), (0, 0), (7, 7), (8, -16), (15, 0), (16, 7), (-11, -20), (-3, 5), (-9, -17)]
    coords = [(x + m.origin[0], y + m.origin[1]) for x, y in ext]
    vals = [donors[(7 * j + 3) % len(donors)] for j in range(len(ext))]
    coords.append((coords[4][0] + 1, coords[4][1]))  # a cell that becomes unknown again
    vals.append(np.asarray(m.unknown, dtype=np.float64)[:stride])
    for c in tops:  # (after the others: a later entry of the dirty log for the same cell would win)
        if c not in coords:
            coords.append(c)
            vals.append(low)
    ctx.map_apply_dirty(FINE, coords, np.asarray(vals))
    xs, ys = [c[0] for c in coords], [c[1] for c in coords]
    pyr.refresh(min(xs), min(ys), max(xs) - min(xs) + 1, max(ys) - min(ys) + 1)
    refreshed = download_levels(ctx, pyr, stride)
    pyr.rebuild()
    rebuilt = download_levels(ctx, pyr, stride)
    assert_levels_equal(refreshed, rebuilt)
    changed = m.payload.copy()
    for (x, y), v in zip(coords, vals):
        changed[y, x] = v
    m2 = type(m)(cell_model=m.cell_model, payload=changed, origin=m.origin, scale=m.scale, unknown=m.unknown)
    assert_levels_equal(rebuilt, pkg.pyramid_build_host(m2, m.oie))
    assert sum(not np.array_equal(bits(a["payload"]), bits(b["payload"])) for a, b in zip(before, rebuilt)) >= 3
    # one cell alone, at a corner of the window
    ctx.map_apply_dirty(FINE, [(0, 0)], np.asarray([donors[1]]))
    pyr.refresh(0, 0, 1, 1)
    changed[0, 0] = donors[1]
    m2.payload = changed
    assert_levels_equal(download_levels(ctx, pyr, stride), pkg.pyramid_build_host(m2, m.oie))
    # small windows that start INSIDE the map (the kernel's cell offset, the launcher's window arithmetic): 6 x 5 cells
    # in the middle, across the external axes; then 3 x 2 cells ending on the map's last column and row
    for x0, y0, w, h in ((8, 17, 6, 5), (34, 27, 3, 2)):
        cells = [(x0 + dx, y0 + dy) for dy in range(h) for dx in range(w)]
        new = [donors[(11 * j + 5) % len(donors)] for j in range(len(cells))]
        new[1] = np.asarray(m.unknown, dtype=np.float64)[:stride]
        ctx.map_apply_dirty(FINE, cells, np.asarray(new))
        pyr.refresh(x0, y0, w, h)
        for (x, y), v in zip(cells, new):
            changed[y, x] = v
        m2.payload = changed
        assert_levels_equal(download_levels(ctx, pyr, stride), pkg.pyramid_build_host(m2, m.oie))
    pyr.close()
    ctx.map_release(FINE)


def upload_set(pkg, ctx, s):
    m = golden_map(s.map)
    ctx.upload_map(FINE, m)
    ctx.scan_upload(s.scan[:, 0], s.scan[:, 1], s.scan[:, 2], s.scan[:, 3], s.scan[:, 4])
    return m, pkg.Pyramid(ctx, FINE, m.oie, FIRST)


def poses_of(base, rot, rect):
    """(x + c.x, y + c.y, rotation + theta) with c = LightWeightRectangle::center()"""
    cx = rect[:, 2] + (rect[:, 3] - rect[:, 2]) / 2
    cy = rect[:, 0] + (rect[:, 1] - rect[:, 0]) / 2
    return np.stack([base[0] + cx, base[1] + cy, rot + base[2]], axis=1)


@pytest.mark.parametrize("j,n", [(12, 1), (13, 63), (16, 65), (34, 206), (46, 206)])
def test_score_matches_equals_score_poses_on_the_level(pkg, ctx, j, n):
    s = golden_set(j)
    m, pyr = upload_set(pkg, ctx, s)
    # the golden candidates (roots and descendants: every level between the fine map and the rectangle's), then the
    # root layer of the documented limits (206 matches) to fill up
    rot206, rect206 = pkg.m3rsm_root_candidates((1.0, 1.0, 2 * 0.087), 0.0017)
    rot = np.concatenate([s.cand[s.n_roots - 2:, 0], rot206])[:n]
    rect = np.concatenate([s.cand[s.n_roots - 2:, 1:5], rect206])[:n]
    ids = pyr.level_map_ids()
    poses = poses_of(s.pose, rot, rect)
    seen_levels = set()
    for sum_order in (pkg.SUM_TREE256, pkg.SUM_SEQUENTIAL):
        for pose_trig in (pkg.POSE_TRIG_DEVICE, pkg.POSE_TRIG_HOST):
            mode = dict(sum_order=sum_order, pose_trig=pose_trig)
            got, level = pyr.score_matches(pkg.spe_cfg(oope=pkg.OOPE_MAX, oie=m.oie, area=(9, 9, 9, 9), **mode), s.pose, rot, rect)
            assert got.shape == (n,) and np.all((level >= 0) & (level < len(ids)))
            want = np.array([ctx.score_poses(ids[level[i]], pkg.spe_cfg(oope=pkg.OOPE_MAX, oie=m.oie, area=rect[i], **mode), poses[i:i + 1])[0]
                             for i in range(n)])
            np.testing.assert_array_equal(bits(got), bits(want), err_msg=str(mode))
            seen_levels |= set(level.tolist())
    if n > 1:
        assert len(seen_levels) >= 3  # mixed levels in one launch
    if n == 206:  # the other window OOPEs, default mode
        for oope in (pkg.OOPE_MEAN, pkg.OOPE_OVERLAP):
            got, level = pyr.score_matches(pkg.spe_cfg(oope=oope, oie=m.oie), s.pose, rot, rect)
            want = np.array([ctx.score_poses(ids[level[i]], pkg.spe_cfg(oope=oope, oie=m.oie, area=rect[i]), poses[i:i + 1])[0]
                             for i in range(n)])
            np.testing.assert_array_equal(bits(got), bits(want))
    pyr.close()
    ctx.map_release(FINE)


def test_bounds_equal_the_references(pkg, ctx):
    """every golden match set: level_out is the scale the reference's map was left at, the scores are
    Match::prob_upper_bound (bit-exact in the strict mode, 1e-12 in the default one), and no child exceeds its parent"""
    for j in range(N_SETS):
        s = golden_set(j)
        m, pyr = upload_set(pkg, ctx, s)
        rot, rect, parent, want, want_level = s.cand[:, 0], s.cand[:, 1:5], s.cand[:, 5].astype(int), s.cand[:, 6], s.cand[:, 7]
        strict, level = pyr.score_matches(pkg.spe_cfg(oope=pkg.OOPE_MAX, oie=m.oie, **STRICT), s.pose, rot, rect)
        np.testing.assert_array_equal(level, want_level, err_msg="set %d" % j)
        np.testing.assert_array_equal(strict, want, err_msg="set %d" % j)
        dflt, level = pyr.score_matches(pkg.spe_cfg(oope=pkg.OOPE_MAX, oie=m.oie), s.pose, rot, rect)
        np.testing.assert_array_equal(level, want_level)
        np.testing.assert_allclose(dflt, want, rtol=DEFAULT_RTOL, atol=0, err_msg="set %d" % j)
        kids = parent >= 0
        assert kids.sum() >= 30 and (m.scale == 1.0 or len(set(level[kids].tolist())) >= 2)
        for sc in (strict, dflt):  # the reference's own assertion (m3rsm_engine.h:352-354)
            assert np.all(sc[kids] <= sc[parent[kids]] + 1e-5), "set %d" % j
        pyr.close()
        ctx.map_release(FINE)


class DeviceArrays:
    """A few arrays in HBM for the `_device` entry, allocated by the HIP runtime THE LIBRARY is linked against (found among
    the process's mapped files: hipMalloc / hipMemcpy / hipFree through ctypes).  torch tensors would do elsewhere in
    this suite, but torch loads a HIP runtime of its own next to the library's; this test needs nothing of torch, and
    memory of the library's own runtime is what a C caller of the entry passes."""

    def __init__(self):
        import ctypes as C
        path = next(ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln)
        self.C, self.hip, self.ptrs = C, C.CDLL(path), []
        self.hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.hip.hipFree.argtypes = [C.c_void_p]

    def put(self, a):
        a = np.ascontiguousarray(a)
        p = self.C.c_void_p()
        assert self.hip.hipMalloc(self.C.byref(p), max(a.nbytes, 8)) == 0
        self.ptrs.append(p)
        assert self.hip.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0  # hipMemcpyHostToDevice
        return p.value

    def get(self, ptr, a):
        assert self.hip.hipMemcpy(a.ctypes.data, ptr, a.nbytes, 2) == 0  # hipMemcpyDeviceToHost
        return a

    def free(self):
        for p in self.ptrs:
            self.hip.hipFree(p)
        self.ptrs = []


def test_device_resident_candidates(pkg, ctx):
    s = golden_set(30)
    m, pyr = upload_set(pkg, ctx, s)
    rot, rect = s.cand[:, 0].copy(), s.cand[:, 1:5].copy()
    rect[3] = [0.2, 0.1, 0.0, 0.1]  # reversed: NaN and level -1 on the device-resident path
    rect[5, 1] = np.nan
    n = rot.size
    dev = DeviceArrays()
    d_rot, d_rect = dev.put(rot), dev.put(rect)
    d_score, d_level = dev.put(np.zeros(n)), dev.put(np.zeros(n, np.int32))
    cfg = pkg.spe_cfg(oope=pkg.OOPE_MAX, oie=m.oie)
    pyr.score_matches_device(cfg, s.pose, n, d_rot, d_rect, d_score, d_level)
    ctx.synchronize()
    got, level = dev.get(d_score, np.zeros(n)), dev.get(d_level, np.zeros(n, np.int32))
    ok = np.ones(n, bool)
    ok[[3, 5]] = False
    want, want_level = pyr.score_matches(cfg, s.pose, rot[ok], rect[ok])
    np.testing.assert_array_equal(bits(got[ok]), bits(want))
    np.testing.assert_array_equal(level[ok], want_level)
    assert np.all(np.isnan(got[~ok])) and np.all(level[~ok] == -1)
    with pytest.raises(pkg.SlamHipError, match="-1"):  # the host entry refuses such a batch as a whole
        pyr.score_matches(cfg, s.pose, rot, rect)
    with pytest.raises(pkg.SlamHipError, match="-1"):
        pyr.score_matches_device(pkg.spe_cfg(oope=pkg.OOPE_MAX, oie=m.oie, pose_trig=pkg.POSE_TRIG_HOST), s.pose, n, d_rot, d_rect,
                                 d_score, d_level)
    dev.free()
    pyr.close()
    ctx.map_release(FINE)


def test_a_level_is_an_ordinary_map(pkg, ctx):
    m = golden_map(64)  # GridCell, 37 x 29, scale 0.1
    ctx.upload_map(FINE, m)
    pyr = pkg.Pyramid(ctx, FINE, m.oie, FIRST)
    host = pkg.pyramid_build_host(m, m.oie)
    for lv, h in zip(pyr.info(), host):
        img = ctx.map_render(lv["map_id"], pkg.RENDER_OCCGRID)
        np.testing.assert_array_equal(img, pkg.render_cells(m.cell_model, h["payload"], pkg.RENDER_OCCGRID))
        pgm = ctx.map_render(lv["map_id"], pkg.RENDER_PGM)
        np.testing.assert_array_equal(pgm, pkg.render_cells(m.cell_model, h["payload"], pkg.RENDER_PGM)[::-1])
    lv, h = pyr.info()[1], host[1]
    win = ctx.map_download_window(lv["map_id"], 1, 2, lv["width"] - 2, lv["height"] - 3, 1)
    np.testing.assert_array_equal(bits(win), bits(h["payload"][2:lv["height"] - 1, 1:lv["width"] - 1]))
    pyr.close()
    ctx.map_release(FINE)


def test_ids_errors_and_a_fine_map_that_moves(pkg, ctx):
    m = golden_map(60)  # 37 x 29, scale 1.0, GridCell
    ctx.upload_map(FINE, m)
    pyr = pkg.Pyramid.create(ctx, FINE, m.oie, FIRST)
    ids = [lv["map_id"] for lv in pyr.info()]
    with pytest.raises(pkg.SlamHipError, match="-1"):  # the ids are taken
        pkg.Pyramid(ctx, FINE, m.oie, ids[-1])
    with pytest.raises(pkg.SlamHipError, match="-1"):
        pkg.Pyramid(ctx, FINE, m.oie, 4095)  # ... and must lie in [0, 4095]
    with pytest.raises(pkg.SlamHipError, match="-1"):
        pkg.Pyramid(ctx, FINE, 2, 100)
    with pytest.raises(pkg.SlamHipError, match="-1"):
        pkg.Pyramid(ctx, 77, m.oie, 100)  # unbound fine map
    with pytest.raises(pkg.SlamHipError, match="-1"):
        pyr.refresh(30, 0, 8, 4)  # outside the fine map
    ctx.scan_upload([1.0], [1.0], [0.0], [1.0])
    with pytest.raises(pkg.SlamHipError, match="-1"):
        pyr.score_matches(pkg.spe_cfg(oope=pkg.OOPE_OBSTACLE, oie=m.oie), [0, 0, 0], [0.0], [[0, 0, 0, 0]])
    with pytest.raises(pkg.SlamHipError, match="-1"):
        pyr.score_matches(pkg.spe_cfg(oope=pkg.OOPE_MAX, oie=1 - m.oie), [0, 0, 0], [0.0], [[0, 0, 0, 0]])
    with pytest.raises(pkg.SlamHipError, match="-1"):
        pyr.score_matches(pkg.spe_cfg(oope=pkg.OOPE_MAX, oie=m.oie), [0, np.inf, 0], [0.0], [[0, 0, 0, 0]])
    pyr.close()
    for i in ids:  # destroy released them ...
        with pytest.raises(pkg.SlamHipError):
            ctx.map_info(i)
    pyr = pkg.Pyramid(ctx, FINE, m.oie, FIRST)  # ... and a second create on them succeeds
    assert [lv["map_id"] for lv in pyr.info()] == ids
    # the fine map grows (a re-bind that keeps the cells at their external coordinates): refresh and the scorer say so,
    # rebuild plans the levels anew under the same ids
    ctx.map_bind(FINE, m.cell_model, 70, 40, (40, 25), m.scale, m.unknown)
    with pytest.raises(pkg.SlamHipError, match="-4"):
        pyr.refresh(0, 0, 1, 1)
    with pytest.raises(pkg.SlamHipError, match="-4"):
        pyr.score_matches(pkg.spe_cfg(oope=pkg.OOPE_MAX, oie=m.oie), [0, 0, 0], [0.0], [[0, 0, 0, 0]])
    pyr.rebuild()
    grown = ctx.map_download_window(FINE, 0, 0, 70, 40, 1)
    m2 = type(m)(cell_model=m.cell_model, payload=grown, origin=(40, 25), scale=m.scale, unknown=m.unknown)
    assert_levels_equal(download_levels(ctx, pyr, 1), pkg.pyramid_build_host(m2, m.oie))
    np.testing.assert_array_equal(bits(grown[25 - 20:25 - 20 + 29, 40 - 11:40 - 11 + 37]), bits(m.payload))
    pyr.close()
    # models the pyramid does not take
    ctx.map_bind(FINE, pkg.CELL_GMAPPING, 8, 8, (4, 4), 0.1, [-1.0, 0.0, 0.0])
    with pytest.raises(pkg.SlamHipError, match="-1"):
        pkg.Pyramid(ctx, FINE, pkg.OIE_DISCREPANCY, FIRST)
    t = golden_map(66)  # TBM
    ctx.upload_map(FINE, t)
    with pytest.raises(pkg.SlamHipError, match="-1"):
        pkg.Pyramid(ctx, FINE, pkg.OIE_OCCUPANCY, FIRST)  # belief cells: the discrepancy OIE only
    with pytest.raises(pkg.SlamHipError):
        ctx.map_info(FIRST)  # a failed create leaves no level behind
    ctx.map_release(FINE)
