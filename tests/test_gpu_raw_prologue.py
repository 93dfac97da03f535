"""GPU suite: slamhip_matcher_process_raw_scan with the lone co-resident hill-climbing chain assembling the raw scan in
its own prologue (SLAMHIP_OPT_RAW_PROLOGUE 1, the default; csrc/hc_resident.hip, RAW) against the assembly kernel in
front of the chain (0).  No tolerance anywhere: the scan block the chain leaves in HBM (slamhip_scan_download, five
rows), the points kept, pose delta, probability and the scorer calls are compared as bit patterns / integers.

Shapes: kept beams around every workgroup size (1, 2, 255, 256, 257, 1023, 1024, 1025, 1080) crossed with workgroups
of 256 / 512 / 1024 threads -- a thread's first beam in registers, the further ones in LDS, none at all --; every way
of keeping beams; three weightings x factor or none x raw / cached beam trig.  Sequences: scans of different lengths in
a row (the staging buffers' turns, the pads of a shorter scan behind a longer one), an empty filter result in between,
matches on the scan the chain left behind (the chain of kernels, a Monte-Carlo matcher), the paths that assemble in
front of the match (a chain of kernels, the beam-order sum, a second context on the device), two contexts."""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as ge
from synth import cast_scan, make_scene

pytestmark = pytest.mark.gpu

_dp = C.POINTER(C.c_double)
N_RAW = 1080
INC = np.deg2rad(270.0) / N_RAW
A_MIN = -np.deg2rad(135.0)
HC = [40, 0.1, 0.1]


@pytest.fixture(scope="module")
def pkg():
    return ge.load_package()


@pytest.fixture(scope="module")
def scene():
    """a 200 x 200 map and raw scans of every length from one ray cast (the first n beams of its 1080)"""
    sc = make_scene(cell_model=0, size=200, scale=0.1, n_beams=N_RAW, seed=31)
    rng, _, _ = cast_scan(sc["gt"], sc["map"].scale, sc["true_pose"], N_RAW, seed=5, raw=True)
    acc, a = [], A_MIN  # the cached provider's own angles (its accumulating loop): every table index is exact
    while len(acc) < N_RAW:
        acc.append(a)
        a += INC
    sc["raw_range"], sc["raw_angle"] = np.minimum(rng, 25.0), np.array(acc)
    return sc


@pytest.fixture(scope="module")
def ctx(pkg, scene):
    c = pkg.Context(0)
    c.upload_map(0, scene["map"])
    yield c
    c.close()


@pytest.fixture(scope="module")
def matchers(pkg, ctx):
    """one hill-climbing matcher per workgroup size and option setting (a matcher adapts to the matches it has seen:
    both settings see the same ones)"""
    ms = {}
    for nt in (256, 512, 1024):
        for opt in (1, 0):
            m = pkg.Matcher(ctx, "HC", pkg.spe_cfg(), HC)
            m.set_device_chain(2, nt)
            ms[nt, opt] = m
    yield ms
    for m in ms.values():
        m.close()


def download(ctx):
    """the current scan's five arrays as bit patterns [5, n]"""
    fn = ctx.L.slamhip_scan_download
    fn.argtypes = [C.c_void_p, C.c_int, _dp, C.POINTER(C.c_int)]
    n = C.c_int(-1)
    assert fn(ctx.h, 0, None, C.byref(n)) == 0
    out = np.full((5, max(n.value, 1)), np.nan)
    assert fn(ctx.h, out.shape[1], out.ctypes.data_as(_dp), C.byref(n)) == 0
    return out[:, :n.value].view(np.uint64)


def table_uploads(ctx):
    n = C.c_longlong(-1)
    ctx.L.slamhip_scan_table_uploads.argtypes = [C.c_void_p, C.POINTER(C.c_longlong)]
    assert ctx.L.slamhip_scan_table_uploads(ctx.h, C.byref(n)) == 0
    return n.value


def keep_mask(keep, n, k, rs, rng):
    """(is_occ, skip_rate, max_range) of a way of keeping k (or, for the data-dependent ways, some) of n raw beams"""
    if keep == "all":
        return None, 0, -1.0
    if keep == "skip2":
        return None, 2, -1.0
    if keep == "range_cut":  # drops the longer half
        return None, 0, float(np.median(rng[:n])) + 1e-9
    occ = np.zeros(n, np.int32)
    if keep == "first":
        occ[0] = 1
    elif keep == "last":
        occ[-1] = 1
    elif keep == "half":
        occ[:] = rs.rand(n) < 0.5
        occ[rs.randint(n)] = 1
    else:  # "pick": exactly k of the n beams, at random places
        occ[rs.choice(n, k, replace=False)] = 1
    return occ, 0, -1.0


def one_match(pkg, ctx, m, opt, scene, n, occ, skip, max_range, fac, trig, weighting, pose, dl=True):
    ctx.set_option(pkg.OPT_RAW_PROLOGUE, opt)
    a_max = A_MIN + INC * n + INC
    match = m.make_raw_process_scan(0, scene["raw_range"][:n], scene["raw_angle"][:n], is_occ=occ, factor=fac,
                                    trig_mode=pkg.TRIG_CACHED if trig == "cached" else pkg.TRIG_RAW, a_min=A_MIN,
                                    a_max=a_max, a_inc=INC, skip_rate=skip, max_range=max_range, weighting=weighting)
    kept, prob = match(pose)
    return dict(kept=kept, prob=np.float64(prob).view(np.uint64), delta=np.array(list(match.delta)).view(np.uint64),
                scan=download(ctx) if dl else None, calls=m.stats()["scorer_calls"])


def both(pkg, ctx, matchers, nt, scene, n, occ=None, skip=0, max_range=-1.0, fac=None, trig="raw", weighting="even",
         pose=None, fused=True):
    """the same raw scan with the chain assembling it and behind the assembly kernel: everything equal, bit for bit;
    `fused`: the first of the two must have gone through the chain's own prologue (None: not looked at)"""
    pose = scene["init_pose"] if pose is None else pose
    before = ctx.get_option(pkg.OPT_RAW_PROLOGUE_MATCHES)
    on = one_match(pkg, ctx, matchers[nt, 1], 1, scene, n, occ, skip, max_range, fac, trig, weighting, pose)
    mid = ctx.get_option(pkg.OPT_RAW_PROLOGUE_MATCHES)
    uploads = table_uploads(ctx)
    off = one_match(pkg, ctx, matchers[nt, 0], 0, scene, n, occ, skip, max_range, fac, trig, weighting, pose)
    assert ctx.get_option(pkg.OPT_RAW_PROLOGUE_MATCHES) == mid  # (0: the assembly kernel)
    assert table_uploads(ctx) == uploads  # (the same angles: the tables stay, whoever reads them)
    if fused is not None and on["kept"] > 0:
        assert mid - before == (1 if fused else 0)
    assert on["kept"] == off["kept"]
    for row, name in enumerate(["range", "cos", "sin", "weight", "factor"]):
        np.testing.assert_array_equal(on["scan"][row], off["scan"][row], err_msg=name)
    assert on["prob"] == off["prob"] and np.array_equal(on["delta"], off["delta"])
    assert on["calls"] == off["calls"]
    for opt in (1, 0):
        assert matchers[nt, opt].resident_stats()["gave_up"] == 0
    return on


@pytest.mark.parametrize("nt", [256, 512, 1024])
@pytest.mark.parametrize("k", [1, 2, 255, 256, 257, 1023, 1024, 1025, 1080])
def test_kept_beams_around_the_workgroup_sizes(pkg, ctx, matchers, scene, nt, k):
    """k beams kept: all of a k-beam scan (no index row), and k picked out of 1080 (index row)"""
    rs = np.random.RandomState(100 + k)
    assert both(pkg, ctx, matchers, nt, scene, k)["kept"] == k
    occ, skip, max_range = keep_mask("pick", N_RAW, k, rs, scene["raw_range"])
    on = both(pkg, ctx, matchers, nt, scene, N_RAW, occ, skip, max_range, fac=0.5 + rs.rand(N_RAW), weighting="viny")
    assert on["kept"] == k


@pytest.mark.parametrize("keep", ["all", "skip2", "first", "last", "half", "range_cut"])
@pytest.mark.parametrize("n", [257, 1080])
def test_filters_weightings_factors_and_trig(pkg, ctx, matchers, scene, n, keep):
    rs = np.random.RandomState(7 * n)
    for weighting in ("even", "viny", "ahr"):
        for with_factor in (False, True):
            for trig in ("raw", "cached"):
                occ, skip, max_range = keep_mask(keep, n, 0, rs, scene["raw_range"])
                fac = 0.5 + rs.rand(n) if with_factor else None
                nt = (256, 512, 1024)[rs.randint(3)]
                before = table_uploads(ctx)
                on = both(pkg, ctx, matchers, nt, scene, n, occ, skip, max_range, fac, trig, weighting)
                assert 0 < on["kept"] <= n
                # the tables go up with a new angle array / trig mode (the first of the two matches at most), never with
                # the option's setting (both())
                assert table_uploads(ctx) - before <= 1


def test_scans_of_different_lengths_in_a_row_and_an_empty_one(pkg, ctx, matchers, scene):
    """the staging buffers take turns whoever reads them, and the pads of a shorter scan behind a longer one are zero
    in both blocks (the rows are compared up to the scan's own length; the next longer scan reads what lies behind)"""
    rs = np.random.RandomState(5)
    for nt in (1024, 256):
        for n in (1080, 300, 1025, 2, 1080, 1, 700):
            both(pkg, ctx, matchers, nt, scene, n, pose=scene["init_pose"] + rs.randn(3) * [0.05, 0.05, 0.02])
        # ... with the option on throughout (no assembly kernel between two chains), lengths going down and up
        ctx.set_option(pkg.OPT_RAW_PROLOGUE, 1)
        seen = []
        for n in (1080, 513, 1080, 64, 1024):
            seen.append(one_match(pkg, ctx, matchers[nt, 1], 1, scene, n, None, 0, -1.0, None, "raw", "viny", scene["init_pose"]))
        ctx.set_option(pkg.OPT_RAW_PROLOGUE, 0)
        for n, on in zip((1080, 513, 1080, 64, 1024), seen):
            off = one_match(pkg, ctx, matchers[nt, 0], 0, scene, n, None, 0, -1.0, None, "raw", "viny", scene["init_pose"])
            assert np.array_equal(on["scan"], off["scan"]) and on["prob"] == off["prob"] and on["calls"] == off["calls"]
            assert np.array_equal(on["delta"], off["delta"])
        # nothing kept: NaN and a zero delta, no current scan; then something again
        for opt in (1, 0):
            r = one_match(pkg, ctx, matchers[nt, opt], opt, scene, 400, np.zeros(400, np.int32), 0, -1.0, None, "raw", "even",
                          scene["init_pose"])
            assert r["kept"] == 0 and np.isnan(r["prob"].view(np.float64)) and r["scan"].shape[1] == 0
        both(pkg, ctx, matchers, nt, scene, 1080)
        assert matchers[nt, 1].resident_stats()["gave_up"] == 0


def test_later_matches_find_the_scan_the_chain_left(pkg, ctx, matchers, scene):
    """a match on the current scan, without a new upload, behind a chain that assembled it itself: the chain of kernels
    and a Monte-Carlo matcher read the block the bookkeeping workgroup wrote"""
    rs = np.random.RandomState(9)
    # (one pair of followers per setting, made alike and given the same calls: a Monte-Carlo matcher's random stream
    # runs on from match to match)
    chain = {opt: pkg.Matcher(ctx, "HC", pkg.spe_cfg(), HC) for opt in (1, 0)}
    mc = {opt: pkg.Matcher(ctx, "MC", pkg.spe_cfg(), [7, 0.2, 0.1, 20, 100]) for opt in (1, 0)}
    try:
        for m in chain.values():
            m.set_device_chain(1)
        for n, weighting in ((1080, "viny"), (257, "even"), (1025, "ahr")):
            occ = (rs.rand(n) < 0.8).astype(np.int32)
            res = {}
            for opt in (1, 0):
                before = ctx.get_option(pkg.OPT_RAW_PROLOGUE_MATCHES)
                first = one_match(pkg, ctx, matchers[1024, opt], opt, scene, n, occ, 0, -1.0, 0.5 + np.arange(n) / n, "cached",
                                  weighting, scene["init_pose"], dl=False)  # (nothing between the match and its followers)
                assert ctx.get_option(pkg.OPT_RAW_PROLOGUE_MATCHES) - before == opt
                r1 = chain[opt].process_scan(0, scene["init_pose"])
                r2 = mc[opt].process_scan(0, scene["init_pose"])
                res[opt] = dict(kept=first["kept"], prob=first["prob"], scan=download(ctx), hc_prob=np.float64(r1["prob"]).view(np.uint64),
                                mc_prob=np.float64(r2["prob"]).view(np.uint64), hc_delta=r1["delta"].view(np.uint64),
                                mc_delta=r2["delta"].view(np.uint64), hc_calls=chain[opt].stats()["scorer_calls"],
                                mc_calls=mc[opt].stats()["scorer_calls"])
            for key in res[1]:
                assert np.array_equal(res[1][key], res[0][key]), key
    finally:
        for m in list(chain.values()) + list(mc.values()):
            m.close()


def test_paths_that_assemble_in_front_of_the_match(pkg, ctx, matchers, scene):
    """a chain of kernels, the beam-order sum, a window OOPE and a Monte-Carlo matcher behind process_raw_scan: the
    assembly kernel runs first whatever the option says -- the fail-over of a co-resident chain goes through the same
    function --, and the results do not depend on the option"""
    kinds = [("HC", pkg.spe_cfg(), HC, 1), ("HC", pkg.spe_cfg(sum_order=pkg.SUM_SEQUENTIAL), HC, 2),
             ("MC", pkg.spe_cfg(), [7, 0.2, 0.1, 20, 100], None),
             ("HC", pkg.spe_cfg(oope=pkg.OOPE_MAX, area=(-0.1, 0.1, -0.1, 0.1)), HC, 2)]
    for kind, cfg, prm, mode in kinds:
        ms = {opt: pkg.Matcher(ctx, kind, cfg, prm) for opt in (1, 0)}
        try:
            for n in (1080, 257):
                out = {}
                for opt in (1, 0):
                    if mode is not None:
                        ms[opt].set_device_chain(mode)
                    before = ctx.get_option(pkg.OPT_RAW_PROLOGUE_MATCHES)
                    out[opt] = one_match(pkg, ctx, ms[opt], opt, scene, n, None, 2, -1.0, None, "raw", "viny", scene["init_pose"])
                    assert ctx.get_option(pkg.OPT_RAW_PROLOGUE_MATCHES) == before
                assert out[1]["kept"] == out[0]["kept"] > 0 and np.array_equal(out[1]["scan"], out[0]["scan"])
                assert out[1]["prob"] == out[0]["prob"] and np.array_equal(out[1]["delta"], out[0]["delta"])
                assert out[1]["calls"] == out[0]["calls"]
        finally:
            for m in ms.values():
                m.close()


def test_two_contexts_on_one_device(pkg, scene):
    """each context stages, assembles and keeps count for itself; matches alternate between them"""
    a, b = pkg.Context(0), pkg.Context(0)
    ms = {}
    try:
        for c in (a, b):
            c.upload_map(0, scene["map"])
            for opt in (1, 0):
                ms[c, opt] = pkg.Matcher(c, "HC", pkg.spe_cfg(), HC)
        rs = np.random.RandomState(13)
        for n_a, n_b in ((1080, 257), (513, 1080), (1080, 1080)):
            for c, n, weighting in ((a, n_a, "viny"), (b, n_b, "even")):
                occ = (rs.rand(n) < 0.7).astype(np.int32)
                two = {(1024, opt): ms[c, opt] for opt in (1, 0)}
                both(pkg, c, two, 1024, scene, n, occ, weighting=weighting)
        assert a.get_option(pkg.OPT_RAW_PROLOGUE_MATCHES) == 3 and b.get_option(pkg.OPT_RAW_PROLOGUE_MATCHES) == 3
        assert table_uploads(a) == 3 and table_uploads(b) == 2  # (per angle array, as without the option)
    finally:
        for m in ms.values():
            m.close()
        a.close()
        b.close()
