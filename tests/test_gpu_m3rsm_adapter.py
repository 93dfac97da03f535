"""GPU suite: the BF_M3RSM host adapter as a maintainer of the reference would include it -- HipM3rsmMap and HipM3rsmEngine
(slam-constructor_amd/host/slamhip_m3rsm_map.h), the BF_M3RSM branch of init_hip_scan_matcher
(host/slamhip_init_scan_matching.h) and HipGridScanMatcher over a resident map -- next to the compiled reference over a
loop of scans (oracle/ref_m3rsm_adapter_harness.cpp).  Per scan: the fine map HipM3rsmMap::append_scan wrote against the
reference's scan adder, the levels it rebuilt or refreshed against the tight twin of the reference's map and against a
pyramid built from scratch, and one match through the two factories.  The matcher's limits and accuracies are all
non-default and no two alike, so a swap in the factory moves the result.
The scenes themselves are checked on the reference alone by tests/test_m3rsm_adapter_reference.py.

The `tbm_viny` cases hold the one place where BF_M3RSM's weights are not the scan's own.  The reference's matcher hands
its estimator PREROTATED scans (prerotate_scan = true, bf_multi_res_scan_matcher.h:42-43): Cartesian points in the world's
orientation, and VinySlamSPW::weight reads a point's angle() -- beam angle + candidate rotation + heading -- so its
weights turn with the candidate.  Weighing the polar points once, in the sensor's frame, is the reference's engine with
prerotate_scan = false and another match: on the first step of tbm_viny-blur delta (-0.1125, 0.025, -0.0174533),
0.50571739, 545 calls against the matcher's (-0.1125, -0.1, -0.0349066), 0.506099, 550 calls.  The adapter stores one
scan per root rotation with the reference's own weighting applied to the reference's own turned scan
(hip_store_rotation_scans, slamhip_matcher_set_m3rsm_rotation_slots).
Built by oracle/Makefile where the reference tree exists; skipped when the prebuilt harness is absent."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SO = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref",
                  "libslamref_m3rsm_adapter.so")
N_STEPS = 9
DEFAULT_RTOL = 1e-12  # tests/test_gpu_m3rsm.py::test_default_mode_finds_the_references_match
SCENES = {0: "occ", 1: "tbm_viny", 2: "tbm_even"}  # cells and scan point weighting
VARIANTS = {0: "blur", 1: "dynamic_blur", 2: "max_range", 3: "no_return"}
# (strict, hip/trig_cache): the reference's bits under the cached and under the raw provider, and the default mode
MODES = {(1, 1): "strict_cached", (1, 0): "strict_raw", (0, 0): "default"}


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(SO):
        pytest.skip("oracle/_ref/libslamref_m3rsm_adapter.so not present")
    L = C.CDLL(SO)
    L.refm3_loop.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]
    L.refm3_engine.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]
    L.refm3_edge.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_double)]
    return L


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("mode", sorted(MODES, reverse=True), ids=lambda m: MODES[m])
@pytest.mark.parametrize("variant", sorted(VARIANTS), ids=lambda v: VARIANTS[v])
@pytest.mark.parametrize("scene", sorted(SCENES), ids=lambda s: SCENES[s])
def test_loop_through_the_adapter_equals_the_reference(lib, scene, variant, mode):
    strict, trig_cache = mode
    k = lib.refm3_row_doubles()
    rows = (C.c_double * (k * N_STEPS))()
    rc = lib.refm3_loop(scene, variant, strict, trig_cache, N_STEPS, rows)
    assert rc == 0, "harness error %d (2: the twin is not tight)" % rc
    r = np.array(list(rows)).reshape(N_STEPS, k)
    print("branch", r[:, 1], "fine", r[:, 0], "view", r[:, 22], "levels", r[:, 2], r[:, 3], "geom", r[:, 4], "twin", r[:, 5],
          "fresh", r[:, 6], "calls", r[:, 15], r[:, 16], "events", r[:, 17], r[:, 18])
    print("ref", r[:, 7:11], "hip", r[:, 11:15])
    # 1. the fine map, payload for payload and as a map consumer reads it
    assert (r[:, 0] == 0).all() and (r[:, 22] == 0).all(), "fine cells differ: %s / %s" % (r[:, 0], r[:, 22])
    # 3. the levels: against the tight twin and against a pyramid built from scratch; both branches were taken
    assert (r[:, 2] == r[:, 3]).all(), "levels: %s, the twin's %s" % (r[:, 2], r[:, 3])
    assert (r[:, 4] == 0).all(), "level geometry: %s" % r[:, 4]
    assert (r[:, 5] == 0).all(), "level cells differ from the twin's: %s" % r[:, 5]
    assert (r[:, 6] == 0).all(), "level cells differ from a fresh pyramid's: %s" % r[:, 6]
    assert (r[:, 1] == 1).any() and (r[:, 1] == 0).any()
    # 4. the match through the factories
    assert (r[:, 20] == 1).all() and (r[:, 17] == 1).all()
    assert (r[:, 18] == 1).all(), "the adapter's observer events: %s" % r[:, 18]
    np.testing.assert_array_equal(bits(r[:, 11:14]), bits(r[:, 7:10]), err_msg="delta")
    if strict:
        np.testing.assert_array_equal(bits(r[:, 14]), bits(r[:, 10]), err_msg="probability")
        np.testing.assert_array_equal(r[:, 16], r[:, 15], err_msg="scorer calls")
    else:
        assert (np.abs(r[:, 14] - r[:, 10]) <= DEFAULT_RTOL * np.abs(r[:, 10])).all(), r[:, 14] - r[:, 10]


@pytest.mark.parametrize("mode", sorted(MODES, reverse=True), ids=lambda m: MODES[m])
@pytest.mark.parametrize("scene", sorted(SCENES), ids=lambda s: SCENES[s])
def test_engine_requests_equal_the_reference(lib, scene, mode):
    """HipM3rsmEngine: three requests over two HipM3rsmMaps of one context (two of them on the same map).  best_match()
    against the reference's M3RSMEngine with the same three requests on the twins; match_each() against three lone
    process_scan calls of the matcher the factory makes.  Under the raw provider the harness first asks for one bound
    on every request: return code 3 means a slot came without its angles."""
    strict, trig_cache = mode
    out = (C.c_double * 34)()
    rc = lib.refm3_engine(scene, strict, trig_cache, 4, out)
    assert rc == 0, "harness error %d (2 twin, 3 a request's slot has no angles, 4 the reference found no match)" % rc
    o = np.array(list(out))
    print("winner", o[0], o[1], "hip", o[2:6], "ref", o[6:10], "each", o[10:22], "lone", o[22:34])
    assert o[0] == o[1] and o[0] >= 0
    np.testing.assert_array_equal(bits(o[2:5]), bits(o[6:9]), err_msg="delta")
    if strict:
        assert bits(o[5]) == bits(o[9])
    else:
        assert abs(o[5] - o[9]) <= DEFAULT_RTOL * abs(o[9])
    # match_each = the lone calls, bit for bit in both modes
    np.testing.assert_array_equal(bits(o[10:22]), bits(o[22:34]))
    # ... and the request that won the shared search is the best of the lone ones
    lone = o[22:34].reshape(3, 4)
    assert lone[int(o[0]), 3] == lone[:, 3].max() and bits(lone[int(o[0]), 3]) == bits(o[5])


@pytest.mark.parametrize("trig_cache", [0, 1], ids=["strict_raw", "strict_cached"])
def test_edge_scene_through_the_factories(lib, trig_cache):
    """End points exactly ON cell edges (33 x 33 cells of 1/8 m, robot on a cell centre, ranges odd multiples of 1/16,
    angles, heading and rotation step multiples of 1/64): on the room scenes the raw and the cached provider give the
    same match, here the reference makes 1260 scorer calls under the raw provider and 1264 under the cached one
    (tests/test_m3rsm_adapter_reference.py asserts that they differ).  A factory that hands the matcher
    SLAMHIP_POSE_TRIG_HOST where `hip/strict` without `hip/trig_cache` asks for RAW_EXACT, or the other way round, fails
    here and nowhere else."""
    out = (C.c_double * 16)()
    assert lib.refm3_edge(trig_cache, 1, out) == 0
    o = np.array(list(out))
    print("ref", o[:6], "hip", o[6:12])
    assert o[5] == 1 and o[11] == 1
    np.testing.assert_array_equal(bits(o[6:10]), bits(o[0:4]), err_msg="delta, probability")
    assert o[10] == o[4], "scorer calls"


def test_rotation_slots_at_the_c_abi():
    """slamhip_matcher_set_m3rsm_rotation_slots without the reference: what the adapter's per-rotation weights stand on.
    A request's scan_slot is the first of one slot per root rotation.  (1) With the request's own scan in every one of them
    the search is the plain one, call for call.  (2) With other weights in ONE rotation's slot the root bounds of that
    rotation move and no other's.  (3) The lone current-scan match is refused while on, a request whose slots are not all
    there is refused before anything runs, and switching off gives the plain search back."""
    import __graft_entry__ as ge
    from m3rsm_many_cases import golden_scene
    from test_gpu_m3rsm_many import Scene

    pkg = ge.load_package()
    ctx = pkg.Context(0)
    sc = Scene(pkg, ctx, golden_scene(0))
    try:
        m = sc.matcher(strict=True)
        want, want_trace, want_calls = m.m3rsm_match_many(sc.table), m.m3rsm_trace_many(), m.stats()["scorer_calls"]
        want_each = m.m3rsm_match_each(sc.table)
        rots = m.m3rsm_rotations()
        R = len(rots)
        # the root layer's order: 0, -s, +s, -2 s, +2 s, ...
        assert R >= 3 and R % 2 == 1 and rots[0] == 0 and (rots[1::2] < 0).all() and (rots[2::2] == -rots[1::2]).all()
        assert (np.diff(rots[2::2]) > 0).all()
        reqs = sc.s.requests
        for k, r in enumerate(reqs):
            for j in range(R):
                ctx.scan_store(100 + k * R + j, r.scan[:, 0], r.scan[:, 1], r.scan[:, 2], r.scan[:, 3], r.scan[:, 4])
        table = [(sc.pyr[r.map], 100 + k * R, r.pose) for k, r in enumerate(reqs)]
        m.set_m3rsm_rotation_slots(True)
        got = m.m3rsm_match_many(table)
        assert got["request"] == want["request"] and bits([got["prob"]]) == bits([want["prob"]])
        np.testing.assert_array_equal(bits(got["delta"]), bits(want["delta"]))
        np.testing.assert_array_equal(bits(m.m3rsm_trace_many()), bits(want_trace))
        assert m.stats()["scorer_calls"] == want_calls
        for a, b in zip(m.m3rsm_match_each(table), want_each):
            np.testing.assert_array_equal(bits(list(a["delta"]) + [a["prob"]]), bits(list(b["delta"]) + [b["prob"]]))
        # (2) rotation 3 of request 0 weighs beam 0 alone
        n_root = 2 * R * len(reqs)  # (empty, entire) per rotation and request, request by request
        r0 = reqs[0]
        w = np.zeros(len(r0.scan))
        w[0] = 1.0
        ctx.scan_store(100 + 3, r0.scan[:, 0], r0.scan[:, 1], r0.scan[:, 2], w, r0.scan[:, 4])
        m.m3rsm_match_many(table)
        root, plain = m.m3rsm_trace_many()[:n_root], want_trace[:n_root]
        np.testing.assert_array_equal(bits(root[:, :6]), bits(plain[:, :6]))
        moved = bits(root[:, 6]) != bits(plain[:, 6])
        touched = (root[:, 0] == 0) & (bits(root[:, 1]) == bits([rots[3]])[0])
        assert touched.sum() == 2 and moved[touched].any() and not moved[~touched].any()
        # (3)
        with pytest.raises(pkg.SlamHipError, match="error -1"):
            sc.lone(m, 0)
        with pytest.raises(pkg.SlamHipError, match="error -1"):
            m.m3rsm_match_many([(sc.pyr[reqs[0].map], 100 + len(reqs) * R - 1, reqs[0].pose)])  # only its first slot holds a scan
        m.set_m3rsm_rotation_slots(False)
        np.testing.assert_array_equal(bits(m.m3rsm_match_many(sc.table)["delta"]), bits(want["delta"]))
        np.testing.assert_array_equal(bits(m.m3rsm_trace_many()), bits(want_trace))
    finally:
        sc.close()
        ctx.close()
