"""GPU suite: the host adapters that had only been through a syntax check, RUN next to the compiled reference -- as a
maintainer of the reference would include them (slam-constructor_amd/host/):
  HipLaserScanGenerator, HipResidentMapView::generate_scans / operator[]     slamhip_scan_generator.h, slamhip_reference_adapter.h
  HipGridMapToPgmDumper, hip_occupancy_grid, HipResidentMapView::render      slamhip_map_observers.h
  HipScanProbabilityEstimator, hip_process_raw_scans / HipRawScanJob         slamhip_reference_adapter.h
  init_hip_resident_credibilist_slam, init_hip_credibilist_scan_matcher, slamhip_credibilist_belief   slamhip_credibilist_slam.h
The harnesses are oracle/ref_consumers_harness.cpp and oracle/ref_credibilist_harness.cpp over the scenes of
oracle/ref_adapter_scenes.h: a hand-made 77 x 45 cecum map with its origin off the centre, and one SLAM-built map per
cell class the resident factories produce, each grown while it was built, each with hand-made TBM beliefs a scan cannot
leave behind.  Every map is copied into HBM (slamhip_map_bind + slamhip_map_upload_window) under a HipResidentMapView of
the matching tbm_kind.  Everything is bit for bit unless a bar is named.  The scenes themselves -- that they run through
the reference without an assertion and contain what they are meant to -- are checked on the reference alone by
tests/test_adapter_scenes_reference.py.
Built by oracle/Makefile where the reference tree exists; skipped when the prebuilt harness is absent."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REF = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref")
SO_CONSUMERS = os.path.join(REF, "libslamref_consumers.so")
SO_CREDIBILIST = os.path.join(REF, "libslamref_credibilist.so")
CLASSES = {0: "cecum_mock", 1: "mean_probability", 2: "affine_quality_merge", 3: "tbm_consistent", 4: "tbm_unknown_even_occ",
           5: "credibilist"}
DEFAULT_RTOL = 1e-12  # tests/test_gpu_parity.py: the default sum against the reference's
D = C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def consumers():
    if not os.path.exists(SO_CONSUMERS):
        pytest.skip("oracle/_ref/libslamref_consumers.so not present")
    L = C.CDLL(SO_CONSUMERS)
    L.refc_scan_generator.argtypes = [C.c_int, D]
    L.refc_angles.argtypes = [D]
    L.refc_observers.argtypes = [C.c_int, C.c_char_p, D]
    L.refc_spe.argtypes = [C.c_int] * 7 + [D]
    L.refc_raw_batch.argtypes = [C.c_int, C.c_int, D]
    return L


@pytest.fixture(scope="module")
def credibilist():
    if not os.path.exists(SO_CREDIBILIST):
        pytest.skip("oracle/_ref/libslamref_credibilist.so not present")
    L = C.CDLL(SO_CREDIBILIST)
    L.refcred_loop.argtypes = [C.c_int] * 5 + [D, D, D]
    L.refcred_host_matcher.argtypes = [C.c_int] * 4 + [D]
    return L


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("cls", sorted(CLASSES), ids=lambda c: CLASSES[c])
def test_scan_generator_over_the_view_equals_the_reference(consumers, cls):
    """Seven poses (the middle, one outside the window, the far corner for hits beyond 64 cells, a cell centre whose
    middle beam runs through grid vertices, one looking out of the open end, one at a wall): (a) the reference's generator
    over the host map = (b) the reference's generator over the view = (c) HipLaserScanGenerator over the view, lone and all
    poses in one call -- number of points, range and angle bits, is_occupied, the provider's dynamic type.  A pose with a
    status-2 beam, found with the library's host routine, must throw std::logic_error from (c).  Then one scan more
    through K6 into a window K6 built, invalidate(), and (c) again against (a) over the reference's updated map."""
    out = (C.c_double * 16)()
    assert consumers.refc_scan_generator(cls, out) == 0
    o = list(out)
    print(CLASSES[cls], "poses", o[0], "points", o[1], "view", o[2], "device", o[3], "batch", o[4], "assert pose tries", o[5],
          "threw", o[6], "clean", o[7], "after update: points", o[8], "mismatches", o[9], "geometry", o[10], "changed", o[11],
          "before", o[12])
    assert o[0] >= 6 and o[1] > 100 and o[7] == 1
    assert o[2] == 0, "the reference's generator over the view"
    assert o[3] == 0, "HipLaserScanGenerator::laser_scan_2D"
    assert o[4] == 0, "laser_scans_2D against the lone calls"
    assert o[5] >= 1 and o[6] == 1, "status 2 must throw std::logic_error"
    if cls != 0:
        assert o[12] == 0 and o[8] > 100 and o[11] >= 1
        assert o[10] == 1, "the view's geometry after invalidate()"
        assert o[9] == 0, "after the K6 update"


def test_scan_generator_angles_equal_the_references_loop(consumers):
    out = (C.c_double * 12)()
    assert consumers.refc_angles(out) == 0
    o = np.array(list(out)).reshape(4, 3)
    print(o)
    assert list(o[:, 0]) == [37, 90, 1001, 4] or list(o[:, 0]) == [37, 90, 1000, 4]  # (the default: cut short by the 2 pi break)
    assert (o[:, 0] == o[:, 1]).all() and (o[:, 2] == 0).all()


@pytest.mark.parametrize("cls", sorted(CLASSES), ids=lambda c: CLASSES[c])
def test_map_observers_equal_the_references(consumers, cls, tmp_path):
    """PGM: four dumps equal as byte strings, header included; three on_map_update through GridMapToPgmDumber and
    HipGridMapToPgmDumper with the same prefix scheme, the map changing and growing in between: same names, same bytes.
    Occupancy grid: hip_occupancy_grid over the view and over the host map against the publisher's cell loop."""
    out = (C.c_double * 24)()
    assert consumers.refc_observers(cls, str(tmp_path).encode(), out) == 0
    o = list(out)
    print(CLASSES[cls], "pgm bytes", o[0], "differ", o[1:4], "updates", o[4:13], "changed", o[13], "grew", o[14], "grid cells", o[15],
          "view", o[16], "host", o[17], "geometry", o[18], "not finite", o[19], "greys", o[20])
    assert o[0] > 3000
    assert o[1] == 0, "GridMapToPgmDumber over the view"
    assert o[2] == 0, "HipGridMapToPgmDumper over the view"
    assert o[3] == 0, "HipGridMapToPgmDumper over the host map"
    for k in range(3):
        assert o[4 + 3 * k] == 1, "file names of update %d" % k
        assert o[5 + 3 * k] == 1, "file bytes of update %d" % k
    assert o[21] == 1 and o[13] == 1 and o[14] >= 1 and o[12] > o[6]
    assert o[15] > 3000 and 0 < o[0] - o[15] < 20  # (one byte per cell behind the PGM header)
    assert o[16] == 0, "hip_occupancy_grid over the view"
    assert o[17] == 0, "hip_occupancy_grid over the host map"
    assert o[18] == 1
    if cls == 3:
        assert o[19] >= 1  # o / (o + e) of the hand-made cells without either mass: -1 in the grid
    if cls != 0:
        assert o[20] > 100


# (cell class, oope 0 obstacle 1 max 2 mean 3 overlap, oie 0 discrepancy 1 occupancy, weighting 0 even 1 viny, cached provider)
SPE_CASES = [(1, 0, 0, 0, 0), (1, 1, 1, 1, 1), (2, 2, 0, 0, 0), (2, 3, 1, 1, 0), (3, 3, 0, 1, 0), (4, 1, 0, 0, 1), (3, 0, 0, 1, 1),
             (4, 2, 0, 1, 0)]


@pytest.mark.parametrize("strict", [1, 0], ids=["sequential", "default_sum"])
@pytest.mark.parametrize("case", SPE_CASES, ids=lambda c: "-".join(map(str, c)))
def test_scan_probability_estimator_equals_the_references(consumers, case, strict):
    """filter_scan + estimate_scan_probability against WeightedMeanPointProbabilitySPE on one scan, one map and 16 poses;
    the window estimators under the area bot -0.17, top 0.09, left -0.06, right 0.23.  Two filter_scans in a row with
    different scans must score the second."""
    cls, oope, oie, weighting, cached = case
    out = (C.c_double * 40)()
    assert consumers.refc_spe(cls, oope, oie, weighting, cached, strict, 1, out) == 0
    o = np.array(list(out))
    print(case, "ref", o[:16], "hip", o[16:32], "points", o[32], "filtered differ", o[33], "second", o[34], o[35])
    assert o[32] >= 50 and o[33] == 0
    if strict:
        np.testing.assert_array_equal(bits(o[16:32]), bits(o[:16]))
        assert bits(o[35]) == bits(o[34]), "the second filter_scan's scan"
    else:
        assert (np.abs(o[16:32] - o[:16]) <= DEFAULT_RTOL * np.abs(o[:16])).all(), o[16:32] - o[:16]
        assert abs(o[35] - o[34]) <= DEFAULT_RTOL * abs(o[34]), "the second filter_scan's scan"


def same(a, b):
    """bit for bit; a result the reference reports as NaN is any NaN"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


@pytest.mark.parametrize("strict", [1, 0], ids=["strict", "default"])
def test_raw_scan_batch_equals_its_owners_and_the_reference(consumers, strict):
    """hip_process_raw_scans: three matchers on one context, each with its own map, scanner and pose (two cell classes
    of one cell model -- the library refuses a batch over maps of different models --, one with viny weights, sp_skip_rate
    and sp_max_usable_range).  Every job = its owner's own process_scan, bit for bit in both modes;
    = the reference's GridScanMatcher::process_scan bit for bit in strict mode.  Rounds: all three; one job without
    points; one job whose scan filters to nothing; K = 1."""
    out = (C.c_double * 160)()
    assert consumers.refc_raw_batch(strict, 1, out) == 0
    o = np.array(list(out))
    r = o[:156].reshape(4, 3, 13)
    print("job", r[:, :, 0:4], "owner", r[:, :, 4:8], "reference", r[:, :, 8:12])
    ran = r[:, :, 12] == 1
    assert ran.sum() == 10
    for rnd in range(4):
        for rob in range(3):
            if not ran[rnd, rob]:
                continue
            job, owner, ref = r[rnd, rob, 0:4], r[rnd, rob, 4:8], r[rnd, rob, 8:12]
            assert same(job, owner), "round %d robot %d: job %s, its owner's process_scan %s" % (rnd, rob, job, owner)
            if strict:
                assert same(job, ref), "round %d robot %d: job %s, the reference %s" % (rnd, rob, job, ref)
    assert list(r[1, 1, 0:3]) == [0, 0, 0] and np.isnan(r[1, 1, 3]), "a job without points"
    assert list(r[2, 2, 0:3]) == [0, 0, 0] and np.isnan(r[2, 2, 3]), "a job whose scan filters to nothing"
    assert o[156] == 1, "the callers' scans and maps were changed"


# (matcher 0 MC / 1 HC, strict, hip/trig_cache)
CRED_MODES = {(1, 1, 1): "hc_strict_cached", (0, 1, 1): "mc_strict_cached", (1, 1, 0): "hc_strict_raw", (1, 0, 0): "hc_default"}


@pytest.mark.parametrize("mode", sorted(CRED_MODES, reverse=True), ids=lambda m: CRED_MODES[m])
def test_credibilist_factory_loop_equals_the_reference_world(credibilist, mode):
    """init_credibilist_slam(props) next to init_hip_resident_credibilist_slam(props) over nine generated scans with
    odometry error, the window growing.  Poses after every scan bit-equal -- in the default mode too, the bar
    tests/test_gpu_world.py holds the resident TBM world to --, the final beliefs mass by mass over the reference's extent,
    the scan qualities the worlds chose (0.9 and 0.6 both occur), world->map() through the view cell by cell."""
    matcher, strict, trig_cache = mode
    n = 9
    poses, q, out = (C.c_double * (6 * n))(), (C.c_double * (2 * n))(), (C.c_double * 16)()
    assert credibilist.refcred_loop(matcher, strict, trig_cache, n, 1, poses, q, out) == 0
    o, p, quality = list(out), np.array(list(poses)).reshape(n, 6), np.array(list(q)).reshape(n, 2)
    print(CRED_MODES[mode], "pose mismatches", o[0], "worst", o[1], "cells", o[2], "belief mismatches", o[3], "worst", o[4],
          "tests", o[5], o[6], "accepted", o[7], o[8], "grown", o[9], "map", o[10], o[11], "view", o[12], "qualities", quality.T)
    np.testing.assert_array_equal(bits(p[:, 3:6]), bits(p[:, 0:3]), err_msg="poses")
    np.testing.assert_array_equal(quality[:, 1], quality[:, 0], err_msg="scan qualities")
    assert set(quality[:, 0]) == {0.9, 0.6}
    assert o[9] >= 1 and o[13] == 1 and o[2] == o[10] * o[11]
    assert o[3] == 0, "final beliefs differ in %d cells (max %g)" % (o[3], o[4])
    assert o[12] == 0, "world->map() through the view"
    assert o[5] == o[6] and o[7] == o[8], "scorer calls"


@pytest.mark.parametrize("mode", sorted(CRED_MODES, reverse=True), ids=lambda m: CRED_MODES[m])
def test_credibilist_matcher_over_a_host_map_equals_the_reference(credibilist, mode):
    """init_hip_credibilist_scan_matcher over a HOST map of CredibilistCell, mirrored through slamhip_credibilist_belief:
    one process_scan beside the reference's matcher on the same map."""
    matcher, strict, trig_cache = mode
    out = (C.c_double * 16)()
    assert credibilist.refcred_host_matcher(matcher, strict, trig_cache, 1, out) == 0
    o = np.array(list(out))
    print(CRED_MODES[mode], "ref", o[:6], "hip", o[6:12], "full uploads", o[12])
    np.testing.assert_array_equal(bits(o[6:9]), bits(o[0:3]), err_msg="delta")
    if strict:
        assert bits(o[9]) == bits(o[3]), "probability"
    else:
        assert abs(o[9] - o[3]) <= DEFAULT_RTOL * abs(o[3])
    assert o[10] == o[4] and o[11] == o[5], "scorer calls"
    assert o[12] == 1
