"""CPU suite: tests/golden/m3rsm_rawtrig.npz (make_golden_m3rsm_rawtrig.py) is what the GPU suite needs it to be -- whole
matches of the compiled reference under its DEFAULT trig provider with their traces, and enough calls in them that the
cached provider scores differently: without those the fixture could not tell SLAMHIP_POSE_TRIG_RAW_EXACT from HOST."""
import os

import numpy as np
import pytest
from m3rsm_rawtrig_cases import EDGE_NAMES, G, LIBM_VARIANT, N_SCENES, PER_SCENE, ROOT, SCENE_NAMES, bits, golden_scene, n_bitwise_different

import __graft_entry__ as ge


def test_structure():
    assert N_SCENES == 6 and SCENE_NAMES == ["occ_square", "occ_1beam", "tbm_square", "cred_square", "edge_occ", "edge_tbm"]
    assert EDGE_NAMES == ["edge_occ", "edge_tbm"] and LIBM_VARIANT in (0, 1)
    assert set(G.files) == {"n_scenes", "libm_variant"} | {"s%d_%s" % (i, k) for i in range(N_SCENES) for k in PER_SCENE}
    size = os.path.getsize(os.path.join(ROOT, "tests", "golden", "m3rsm_rawtrig.npz"))
    assert size <= 930 * 1024
    beams = {"occ_square": 67, "occ_1beam": 1, "tbm_square": 67, "cred_square": 67, "edge_occ": 67, "edge_tbm": 67}
    shape = {"occ_1beam": (29, 37)}
    for name in SCENE_NAMES:
        s = golden_scene(name)
        n = beams[name]
        stride = {0: 1, 1: 4, 3: 4}[s.cell_model]
        assert s.scan.shape == (n, 5) and s.angle.shape == (n,) and s.trig.shape == (3,) and s.limits.shape == (5,)
        assert s.payload.shape == shape.get(name, (33, 33)) + (stride,) and s.unknown.shape == (stride,)
        for t in (s.trace, s.trace_cached):
            assert t.ndim == 2 and t.shape[1] == 7 and 0 < len(t) <= 4500 and np.all(np.isfinite(t))
        assert s.delta.shape == (3,) and s.delta_cached.shape == (3,) and np.isfinite(s.prob) and np.isfinite(s.prob_cached)
        # the scan's cos / sin columns are the raw provider's at base angle 0, the angles lie on the cached provider's grid
        np.testing.assert_allclose(s.scan[:, 1], np.cos(s.angle), rtol=0, atol=1e-15)
        np.testing.assert_allclose(s.scan[:, 2], np.sin(s.angle), rtol=0, atol=1e-15)
        k = (s.angle - s.trig[0]) / s.trig[2]
        np.testing.assert_allclose(k, np.round(k), rtol=0, atol=1e-9)
        assert np.all(s.scan[:, 4] == 1.0) and np.all(s.scan[:, 3] == s.scan[0, 3])


@pytest.mark.parametrize("name", ["edge_occ", "edge_tbm"])
def test_edge_scenes_are_made_of_exact_binary_fractions(name):
    s = golden_scene(name)
    assert s.edge and s.scale == 0.125
    on_centre = s.pose[:2] * 16
    assert np.all(on_centre == np.round(on_centre)) and np.all(np.round(on_centre) % 2 == 1)  # a cell centre
    r16 = s.scan[:, 0] * 16
    assert np.all(r16 == np.round(r16)) and np.all(np.round(r16) % 2 == 1)  # centre + range along an axis: a cell edge
    assert np.all(s.angle * 32 == np.round(s.angle * 32)) and s.pose[2] * 64 == round(s.pose[2] * 64)
    assert np.all(s.limits * 64 == np.round(s.limits * 64))
    rots = np.unique(s.trace[:, 0])
    assert np.all(rots * 64 == np.round(rots * 64))
    # heading + rotation + angle is exactly 0 for a beam of some rotation: the raw provider's direction is (1, 0) there
    assert np.any((s.pose[2] + rots)[:, None] + s.angle[None, :] == 0.0)


def test_the_providers_are_told_apart():
    total, moved = 0, []
    for name in SCENE_NAMES:
        s = golden_scene(name)
        n = n_bitwise_different(s.trace, s.trace_cached)
        total += n
        if s.edge:
            assert n >= 1, name
        if len(s.trace) != len(s.trace_cached) or not np.array_equal(bits(s.delta), bits(s.delta_cached)):
            moved.append(name)
    assert total >= 10
    assert moved, "in no scene does the provider change the number of calls or the delta"


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_every_level_follows_from_its_rectangle_and_the_roots_are_the_root_layer(name):
    pkg = ge.load_package()
    s = golden_scene(name)
    levels = pkg.pyramid_build_host(s, s.oie)
    lv_scale = np.array([s.scale] + [lv["scale"] for lv in levels])
    for t in (s.trace, s.trace_cached):
        side = np.maximum(t[:, 2] - t[:, 1], t[:, 4] - t[:, 3])
        assert np.all(side >= 0)
        np.testing.assert_array_equal(t[:, 6], [int(np.argmax(v <= lv_scale)) for v in side])
        rot, rect = pkg.m3rsm_root_candidates((s.limits[0], s.limits[1], 2 * s.limits[2]), s.limits[3])
        np.testing.assert_array_equal(bits(t[:len(rot), 0]), bits(rot))
        np.testing.assert_array_equal(bits(t[:len(rot), 1:5]), bits(rect))
    # the result is a point of the trace
    win = (s.trace[:, 0] == s.delta[2]) & (s.trace[:, 3] == s.delta[0]) & (s.trace[:, 4] == s.delta[0]) \
        & (s.trace[:, 1] == s.delta[1]) & (s.trace[:, 2] == s.delta[1])
    assert np.any(s.trace[win, 5] == s.prob)
