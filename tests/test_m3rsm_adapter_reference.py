"""The scenes of tests/test_gpu_m3rsm_adapter.py on the REFERENCE alone (no GPU): oracle/ref_m3rsm_adapter_harness.cpp's
refm3_reference_selfcheck runs the loop -- the reference's scan adder into M3RSMRescalableGridMap<UnboundedPlainGridMap>,
the tight twin of that map, the reference's BF_M3RSM matcher on the twin -- without calling into the device library.
What the GPU test relies on is asserted here, where a wrong scene costs no GPU time: the twin is tight at every step, the
reference's match is valid and stays under the golden generator's cap on scorer calls, the run rebuilds and refreshes,
and the twin is needed at all (the loop map's coarse cells do sit above the tight maximum).
Built by oracle/Makefile where the reference tree exists; skipped when the harness is absent."""
import ctypes as C
import os

import numpy as np
import pytest

SO = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref",
                  "libslamref_m3rsm_adapter.so")
N_STEPS = 9
MAX_CALLS = 4500  # tests/golden/make_golden_m3rsm.py's own cap
SCENES = {0: "occ", 1: "tbm_viny", 2: "tbm_even"}  # cells and scan point weighting
VARIANTS = {0: "blur", 1: "dynamic_blur", 2: "max_range", 3: "no_return"}


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(SO):
        pytest.skip("oracle/_ref/libslamref_m3rsm_adapter.so not present")
    L = C.CDLL(SO)
    L.refm3_reference_selfcheck.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]
    L.refm3_edge.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_double)]
    return L


@pytest.mark.parametrize("variant", sorted(VARIANTS), ids=lambda v: VARIANTS[v])
@pytest.mark.parametrize("scene", sorted(SCENES), ids=lambda s: SCENES[s])
def test_scene_on_the_reference_alone(lib, scene, variant):
    k = lib.refm3_row_doubles()
    rows = (C.c_double * (k * N_STEPS))()
    rc = lib.refm3_reference_selfcheck(scene, variant, N_STEPS, rows)
    assert rc == 0, "the twin is not tight (harness error %d)" % rc
    r = np.array(list(rows)).reshape(N_STEPS, k)
    assert (r[:, 20] == 1).all(), "the reference's match on the twin is not valid"
    assert (r[:, 17] == 1).all(), "on_matching_start / on_matching_end: not once each, or not with the result"
    assert 0 < r[:, 15].min() and r[:, 15].max() <= MAX_CALLS, r[:, 15]
    assert (r[:, 1] == 1).sum() >= 1 and (r[:, 1] == 0).sum() >= 5, "window grew at steps %s" % r[:, 1]
    assert r[:, 19].max() > 0, "no coarse cell of the loop map is looser than the twin's"
    assert (r[:, 21] > 100).all()  # a map was built
    print("scene %s variant %s: rebuilds %d, refreshes %d, calls <= %d, loop map above the twin by up to %.3g"
          % (SCENES[scene], VARIANTS[variant], (r[:, 1] == 1).sum(), (r[:, 1] == 0).sum(), r[:, 15].max(), r[:, 19].max()))


def test_edge_scene_tells_the_providers_apart(lib):
    """The edge scene (end points exactly ON cell edges under the raw provider) is what tells SLAMHIP_POSE_TRIG_RAW_EXACT
    from HOST in the GPU test: the reference itself must answer differently under its two providers there."""
    res = []
    for trig_cache in (0, 1):
        out = (C.c_double * 16)()
        assert lib.refm3_edge(trig_cache, 0, out) == 0
        o = np.array(list(out))
        assert o[3] == o[3] and o[5] == 1 and 0 < o[4] <= MAX_CALLS
        res.append(o[:5])
    print("raw", res[0], "cached", res[1])
    assert (res[0].view(np.uint64) != res[1].view(np.uint64)).any()
