"""GPU suite: the raw scan's way into HBM (slamhip_scan_filter_upload -> k_scan_assemble).  The call stages what is new
with a scan -- kept ranges, kept indices where a beam was dropped, factors / ahr weights where there are any -- and a
kernel assembles the scan block from that and the per-beam tables (cos, sin, viny factor) resident in HBM.  The block must
hold, double for double, what the packed upload (slamhip_scan_upload -> k_scan_pull) of the same scan filtered step by
step on the host leaves there: both are read back (slamhip_scan_download) and compared as bit patterns, and a handful
of poses scored in beam order must come out bit for bit the same.  For the viny weighting this is also the proof that
the device's double sqrt and the one multiplication return the host's bits on these inputs.

Shapes: raw beam counts around the workgroup size (1, 2, 255, 256, 257) and the headline's 1080; every way of keeping
beams (all, every 2nd / 3rd, first only, last only, a random half, a range cut); three weightings x factor or none x
raw / cached beam trig.  Sequences: the tables go up once per angle array / trig mode and not with new ranges; an empty
result in between; a bounded map; RAW_EXACT scoring after a default call (the kept angles are written out on demand);
two contexts with tables of their own."""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as ge
from synth import MapData

pytestmark = pytest.mark.gpu

_dp = C.POINTER(C.c_double)
SIZE, SCALE = 320, 0.1  # a 32 m window around the origin: beams of up to 12 m from poses near it stay inside
INC = np.deg2rad(270.0) / 1080
A_MIN = -np.deg2rad(135.0)


@pytest.fixture(scope="module")
def pkg():
    return ge.load_package()


@pytest.fixture(scope="module")
def gmap():
    rs = np.random.RandomState(3)
    return MapData(0, rs.rand(SIZE, SIZE, 1), (SIZE // 2, SIZE // 2), SCALE, [0.5])


@pytest.fixture(scope="module")
def ctx(pkg, gmap):
    c = pkg.Context(0)
    c.upload_map(0, gmap)
    yield c
    c.close()


@pytest.fixture(scope="module")
def poses():
    return np.random.RandomState(4).randn(6, 3) * [0.5, 0.5, 0.3]


def angles(n, shift=0.0):
    """the cached provider's own angles (its accumulating loop), so that every table index is exact"""
    a_max = A_MIN + INC * n + INC
    acc, a = [], A_MIN
    while a < a_max:
        acc.append(a)
        a += INC
    return np.array(acc[:n]) + shift, a_max


def table_uploads(ctx):
    n = C.c_longlong(-1)
    ctx.L.slamhip_scan_table_uploads.argtypes = [C.c_void_p, C.POINTER(C.c_longlong)]
    assert ctx.L.slamhip_scan_table_uploads(ctx.h, C.byref(n)) == 0
    return n.value


def download(ctx):
    """the current scan's five arrays as bit patterns [5, n]"""
    fn = ctx.L.slamhip_scan_download
    fn.argtypes = [C.c_void_p, C.c_int, _dp, C.POINTER(C.c_int)]
    n = C.c_int(-1)
    assert fn(ctx.h, 0, None, C.byref(n)) == 0
    out = np.full((5, max(n.value, 1)), np.nan)
    assert fn(ctx.h, out.shape[1], out.ctypes.data_as(_dp), C.byref(n)) == 0
    return out[:, :n.value].view(np.uint64)


def both_ways(pkg, ctx, gmap, poses, rng, ang, a_max, occ, fac, trig, weighting, skip=0, max_range=-1.0, bounded=False,
              pose=(0.1, -0.2, 0.3)):
    """The same raw scan through the separate steps + packed upload and through the one call; returns the number kept."""
    tm = pkg.TRIG_CACHED if trig == "cached" else pkg.TRIG_RAW
    cfg = pkg.spe_cfg(sum_order=pkg.SUM_SEQUENTIAL, pose_trig=pkg.POSE_TRIG_HOST)
    geom = dict(width=gmap.width, height=gmap.height, origin=gmap.origin, scale=gmap.scale, bounded=bounded)
    tab = pkg.beam_trig(ang, tm, A_MIN, a_max, INC)
    kept = pkg.filter_scan(rng, ang, occ, pose, geom, skip_rate=skip, max_range=max_range, trig_mode=tm, a_min=A_MIN,
                           a_delta=INC, tab_sin=tab[1] if trig == "cached" else None,
                           tab_cos=tab[0] if trig == "cached" else None)
    got_kept = ctx.scan_filter_upload(0, rng, ang, pose, is_occ=occ, factor=fac, trig_mode=tm, a_min=A_MIN, a_max=a_max,
                                      a_inc=INC, skip_rate=skip, max_range=max_range, bounded=bounded, weighting=weighting)
    np.testing.assert_array_equal(got_kept, kept)
    if kept.size == 0:
        assert download(ctx).shape[1] == 0
        return 0
    got, got_scores = download(ctx), ctx.score_poses(0, cfg, poses)
    w = pkg.scan_weights(weighting, rng[kept], ang[kept])
    ctx.scan_upload(rng[kept], tab[0][kept], tab[1][kept], w, fac[kept] if fac is not None else None)
    want, want_scores = download(ctx), ctx.score_poses(0, cfg, poses)
    for row, name in enumerate(["range", "cos", "sin", "weight", "factor"]):
        np.testing.assert_array_equal(got[row], want[row], err_msg=name)
    np.testing.assert_array_equal(got_scores.view(np.uint64), want_scores.view(np.uint64))
    return kept.size


def keep_case(keep, n, rs, rng):
    """(is_occ, skip_rate, max_range) of a way of keeping beams"""
    if keep == "all":
        return None, 0, -1.0
    if keep in ("skip2", "skip3"):
        return None, int(keep[-1]), -1.0
    if keep == "range_cut":  # drops the longer half (the only beam of a 1-beam scan stays)
        return None, 0, float(np.median(rng)) + 1e-9
    occ = np.zeros(n, np.int32)
    if keep == "first":
        occ[0] = 1
    elif keep == "last":
        occ[-1] = 1
    else:
        occ[:] = rs.rand(n) < 0.5
        occ[rs.randint(n)] = 1
    return occ, 0, -1.0


@pytest.mark.parametrize("keep", ["all", "skip2", "skip3", "first", "last", "half", "range_cut"])
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 1080])
def test_assembled_scan_equals_the_packed_upload(pkg, ctx, gmap, poses, n, keep):
    rs = np.random.RandomState(1000 + n)
    ang, a_max = angles(n)
    for weighting in ("even", "viny", "ahr"):
        for with_factor in (False, True):
            for trig in ("raw", "cached"):
                rng = 0.5 + 11.5 * rs.rand(n)
                fac = 0.5 + rs.rand(n) if with_factor else None
                occ, skip, max_range = keep_case(keep, n, rs, rng)
                k = both_ways(pkg, ctx, gmap, poses, rng, ang, a_max, occ, fac, trig, weighting, skip, max_range)
                assert k == n if keep == "all" else 0 < k <= n


def test_tables_go_up_with_the_angles_and_not_with_the_ranges(pkg, gmap, poses):
    ctx = pkg.Context(0)
    try:
        ctx.upload_map(0, gmap)
        rs = np.random.RandomState(7)
        n = 257
        ang, a_max = angles(n)
        tab = pkg.beam_trig(ang)
        ctx.scan_upload(1.0 + rs.rand(n), tab[0], tab[1], np.full(n, 1.0 / n))
        assert table_uploads(ctx) == 0  # a context that is given filtered scans only has no tables

        def scan(ang, a_max, trig="raw", weighting="viny", occ="half", bounded=False, lo=0.5, hi=12.0):
            m = ang.size
            o = (rs.rand(m) < 0.5).astype(np.int32) if isinstance(occ, str) else occ
            return both_ways(pkg, ctx, gmap, poses, lo + (hi - lo) * rs.rand(m), ang, a_max, o, 0.5 + rs.rand(m), trig,
                             weighting, bounded=bounded)

        for _ in range(3):  # same angles, new ranges (and masks, and weightings)
            assert scan(ang, a_max) > 0
            assert table_uploads(ctx) == 1
        assert scan(ang, a_max, weighting="even") > 0 and scan(ang, a_max, weighting="ahr") > 0
        assert table_uploads(ctx) == 1
        assert scan(ang + 1e-3, a_max) > 0  # another angle array of the same length
        assert table_uploads(ctx) == 2
        ang2, a_max2 = angles(300)  # another length
        assert scan(ang2, a_max2) > 0
        assert table_uploads(ctx) == 3
        assert scan(ang2, a_max2, trig="cached") > 0  # the same angles through the other trig provider
        assert table_uploads(ctx) == 4
        # nothing kept, then something again
        assert scan(ang2, a_max2, trig="cached", occ=np.zeros(300, np.int32)) == 0
        with pytest.raises(pkg.SlamHipError):
            ctx.score_poses(0, pkg.spe_cfg(), poses)
        assert scan(ang2, a_max2, trig="cached") > 0
        # a bounded map drops the beams that leave the 32 m window
        k = scan(ang2, a_max2, trig="cached", occ=np.ones(300, np.int32), bounded=True, lo=10.0, hi=30.0)
        assert 0 < k < 300
        assert table_uploads(ctx) == 4
        ang3, a_max3 = angles(5000)  # more beams than the tables' first allocation holds
        assert scan(ang3, a_max3) > 0
        assert table_uploads(ctx) == 5
    finally:
        ctx.close()


def test_raw_exact_scoring_after_a_default_call_finds_the_kept_angles(pkg, gmap, poses):
    """The kept points' angles are no longer written out with every scan: an exact call after a default one gets them
    on demand, and scores what the packed upload + slamhip_scan_set_angles of the same points scores."""
    ctx = pkg.Context(0)
    try:
        ctx.upload_map(0, gmap)
        rs = np.random.RandomState(9)
        n = 257
        ang, a_max = angles(n)
        exact = pkg.spe_cfg(sum_order=pkg.SUM_SEQUENTIAL, pose_trig=pkg.POSE_TRIG_RAW_EXACT)
        for rep in range(3):
            rng, occ = 0.5 + 11.5 * rs.rand(n), (rs.rand(n) < 0.6).astype(np.int32)
            if rep == 2:
                ang = ang + 2e-3  # the angle array changes under a scan whose angles were never asked for
            kept = ctx.scan_filter_upload(0, rng, ang, (0.0, 0.0, 0.0), is_occ=occ, weighting="viny")
            ctx.score_poses(0, pkg.spe_cfg(), poses)
            if pkg.libm_variant() < 0:  # no exact modes on this host: both ways refuse
                with pytest.raises(pkg.SlamHipError):
                    ctx.score_poses(0, exact, poses)
                return
            got = ctx.score_poses(0, exact, poses)
            if rep == 1:  # ... and explicit angles replace the lazy ones
                ctx.scan_set_angles(ang[kept] + 0.25)
                moved = ctx.score_poses(0, exact, poses)
                assert not np.array_equal(moved, got)
            tab = pkg.beam_trig(ang)
            ctx.scan_upload(rng[kept], tab[0][kept], tab[1][kept], pkg.scan_weights("viny", rng[kept], ang[kept]))
            with pytest.raises(pkg.SlamHipError):  # the packed upload knows no angles
                ctx.score_poses(0, exact, poses)
            ctx.scan_set_angles(ang[kept])
            want = ctx.score_poses(0, exact, poses)
            np.testing.assert_array_equal(got.view(np.uint64), want.view(np.uint64))
    finally:
        ctx.close()


def test_two_contexts_keep_tables_of_their_own(pkg, gmap, poses):
    a, b = pkg.Context(0), pkg.Context(0)
    try:
        rs = np.random.RandomState(11)
        for c in (a, b):
            c.upload_map(0, gmap)
        ang_a, max_a = angles(257)
        ang_b, max_b = angles(1080, shift=0.01)
        for _ in range(2):
            for c, ang, a_max, trig in ((a, ang_a, max_a, "cached"), (b, ang_b, max_b, "raw")):
                m = ang.size
                assert both_ways(pkg, c, gmap, poses, 0.5 + 11.5 * rs.rand(m), ang, a_max,
                                 (rs.rand(m) < 0.7).astype(np.int32), None, trig, "viny") > 0
        assert table_uploads(a) == 1 and table_uploads(b) == 1
    finally:
        a.close()
        b.close()
