"""The scenes of tests/test_gpu_host_adapters.py on the REFERENCE alone (no GPU): the reference-alone entry points of
oracle/ref_consumers_harness.cpp and oracle/ref_credibilist_harness.cpp.  The reference's generator ends the process where
one of its assertions fails, so every pose a scene uses goes through the library's host routine first (refc_pose_check, no
device): a pose with a status-2 beam, or one the library refuses, fails here as a plain assert.  What the GPU tests rely on
is asserted here as counts, where a wrong scene costs no GPU time.
Built by oracle/Makefile where the reference tree exists; skipped when the harnesses are absent."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

REF = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref")
SO_CONSUMERS = os.path.join(REF, "libslamref_consumers.so")
SO_CREDIBILIST = os.path.join(REF, "libslamref_credibilist.so")
CLASSES = {0: "cecum_mock", 1: "mean_probability", 2: "affine_quality_merge", 3: "tbm_consistent", 4: "tbm_unknown_even_occ",
           5: "credibilist"}
D = C.POINTER(C.c_double)
STATS = ["w", "h", "ox", "oy", "grown", "cells", "never_observed", "greys", "points", "hit_early", "hit_late", "miss",
         "leaves_window", "tie", "robot_outside", "unknown_lt_1_no_mass", "conflict", "not_finite", "assert_pose_tries",
         "grown_in_updates", "beams"]


@pytest.fixture(scope="module")
def consumers():
    if not os.path.exists(SO_CONSUMERS):
        pytest.skip("oracle/_ref/libslamref_consumers.so not present")
    L = C.CDLL(SO_CONSUMERS)
    L.refc_pose_check.argtypes = [C.c_int, C.c_int, D]
    L.refc_scene_stats.argtypes = [C.c_int, D]
    L.refc_spe.argtypes = [C.c_int] * 7 + [D]
    L.refc_raw_batch.argtypes = [C.c_int, C.c_int, D]
    # the poses the maps are built and updated from, before anything is built from them
    out = (C.c_double * 32)()
    n = L.refc_pose_check(0, 0, out)
    assert n >= 8 and list(out)[:n] == [0.0] * n, "a build pose trips the reference's generator: %s" % list(out)[:n]
    return L


@pytest.fixture(scope="module")
def credibilist():
    if not os.path.exists(SO_CREDIBILIST):
        pytest.skip("oracle/_ref/libslamref_credibilist.so not present")
    L = C.CDLL(SO_CREDIBILIST)
    L.refcred_loop.argtypes = [C.c_int] * 5 + [D, D, D]
    L.refcred_host_matcher.argtypes = [C.c_int] * 4 + [D]
    return L


@pytest.mark.parametrize("cls", sorted(CLASSES), ids=lambda c: CLASSES[c])
def test_map_scene_on_the_reference_alone(consumers, cls):
    out = (C.c_double * 32)()
    for phase in (1, 2):  # the map as built, and after the update of the generator scene
        n = consumers.refc_pose_check(cls, phase, out)
        assert n >= 6 and list(out)[:n] == [0.0] * n, "a generator pose trips the reference's generator: %s" % list(out)[:n]
    out = (C.c_double * 24)()
    assert consumers.refc_scene_stats(cls, out) == 0
    s = dict(zip(STATS, list(out)))
    print(CLASSES[cls], s)
    if cls == 0:  # the hand-made map: oblong, origin off the centre in both axes
        assert (s["w"], s["h"], s["ox"], s["oy"]) == (77, 45, 45, 26)
    else:
        assert s["w"] != s["h"] and (s["ox"], s["oy"]) != (s["w"] // 2, s["h"] // 2)
        assert s["greys"] > 100
        assert s["grown_in_updates"] == 2, "the observers' scene: the map must grow in both updates"
    assert s["grown"] >= 1
    assert 0.25 * s["cells"] <= s["never_observed"] <= 0.45 * s["cells"]
    assert 37 * 6 <= s["beams"] <= 90 * 7
    assert s["hit_early"] >= 100 and s["hit_late"] >= 5 and s["miss"] >= 50 and s["points"] == s["hit_early"] + s["hit_late"]
    assert s["leaves_window"] >= 100 and s["tie"] >= 1 and s["robot_outside"] == 1
    assert s["assert_pose_tries"] >= 1, "no pose on which the library's host routine reports status 2"
    if cls >= 3:
        assert s["unknown_lt_1_no_mass"] >= 1 and s["conflict"] >= 2
    if cls == 3:  # o / (o + e) of a cell without either mass
        assert s["not_finite"] >= 1


# (cell class, oope, oie, weighting, cached): tests/test_gpu_host_adapters.py runs the same list
SPE_CASES = [(1, 0, 0, 0, 0), (1, 1, 1, 1, 1), (2, 2, 0, 0, 0), (2, 3, 1, 1, 0), (3, 3, 0, 1, 0), (4, 1, 0, 0, 1), (3, 0, 0, 1, 1),
             (4, 2, 0, 1, 0)]


@pytest.mark.parametrize("case", SPE_CASES, ids=lambda c: "-".join(map(str, c)))
def test_estimator_scene_on_the_reference_alone(consumers, case):
    cls, oope, oie, weighting, cached = case
    out = (C.c_double * 40)()
    assert consumers.refc_spe(cls, oope, oie, weighting, cached, 1, 0, out) == 0
    o = np.array(list(out))
    print(case, "points", o[32], "probabilities", o[:16], "second scan", o[34], "bot/left exchanged", o[36])
    assert o[32] >= 50
    # (the `max` estimator has plateaus: two poses may see the same cells)
    assert np.isfinite(o[:16]).all() and len(set(o[:16])) >= 12, "16 poses must score differently"
    assert np.isfinite(o[34]) and o[34] != o[0], "the second scan must score differently"
    if oope != 0:  # a permuted analysis area must move the result
        assert o[36] != o[0]


def test_batch_scene_on_the_reference_alone(consumers):
    out = (C.c_double * 160)()
    assert consumers.refc_raw_batch(1, 0, out) == 0
    r = np.array(list(out))[:156].reshape(4, 3, 13)
    print(r[:, :, 8:])
    assert (r[:3, :, 12] == 1).all() and list(r[3, :, 12]) == [0, 1, 0]
    full = r[0, :, 8:12]
    assert np.isfinite(full).all() and (np.abs(full[:, :3]).sum(axis=1) > 0).all(), "every robot's match corrects its pose"
    assert len({tuple(x) for x in full}) == 3
    # an empty job, and a job whose scan filters to nothing: no correction, the unknown probability
    assert list(r[1, 1, 8:11]) == [0, 0, 0] and np.isnan(r[1, 1, 11])
    assert list(r[2, 2, 8:11]) == [0, 0, 0] and np.isnan(r[2, 2, 11])
    # the others are what they were
    np.testing.assert_array_equal(r[1, [0, 2], 8:12], full[[0, 2]])
    np.testing.assert_array_equal(r[2, [0, 1], 8:12], full[[0, 1]])
    np.testing.assert_array_equal(r[3, 1, 8:12], full[1])


# (matcher 0 MC / 1 HC, strict, hip/trig_cache)
CRED_MODES = [(1, 1, 1), (0, 1, 1), (1, 1, 0), (1, 0, 0)]


@pytest.mark.parametrize("mode", CRED_MODES, ids=lambda m: "-".join(map(str, m)))
def test_credibilist_loop_on_the_reference_alone(credibilist, mode):
    matcher, strict, trig_cache = mode
    n = 9
    poses, q, out = (C.c_double * (6 * n))(), (C.c_double * (2 * n))(), (C.c_double * 16)()
    assert credibilist.refcred_loop(matcher, strict, trig_cache, n, 0, poses, q, out) == 0
    o, quality = list(out), list(q)[::2]
    print(mode, "tests", o[5], "accepted", o[7], "map", o[10], o[11], "known", o[14], "qualities", quality)
    assert o[13] == 1 and o[10] != o[11], "the reference's map must grow"
    assert o[5] > 100 and o[7] >= 5 and o[14] > 2000
    assert set(quality) == {0.9, 0.6}, "both scan qualities must occur"
    out = (C.c_double * 16)()
    assert credibilist.refcred_host_matcher(matcher, strict, trig_cache, 0, out) == 0
    o = list(out)
    print("host map: delta", o[:3], "probability", o[3], "tests", o[4], "accepted", o[5])
    assert o[3] == o[3] and o[4] > 50 and o[5] >= 3 and o[13] > 1500


def test_credibilist_matcher_refuses_the_occupancy_oie_in_a_child_process():
    """init_hip_credibilist_scan_matcher with oie/type = occupancy prints its message and ends the process before it
    touches a device: run in a child, which must not come back."""
    if not os.path.exists(SO_CREDIBILIST):
        pytest.skip("oracle/_ref/libslamref_credibilist.so not present")
    code = "import ctypes, sys; sys.exit(100 + ctypes.CDLL(%r).refcred_refusal())" % SO_CREDIBILIST
    r = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=60)
    assert r.returncode == 255, (r.returncode, r.stderr)  # std::exit(-1)
    assert "credibilist cells score through the discrepancy OIE on the HIP path" in r.stderr
    assert "[slamhip]" not in r.stderr, "a library call was reached: %s" % r.stderr
