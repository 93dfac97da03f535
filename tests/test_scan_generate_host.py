"""CPU suite: scan generation on the host (slamhip_scan_gen_angles, slamhip_scan_generate_host -- the per-beam routine
the kernels of csrc/scan_generate.hip run, csrc/scan_generate_device.h) against tests/golden/scan_generate.npz, the scans
and angle lists of the compiled reference's LaserScanGenerator (tests/golden/make_golden_scan_generate.py): bit for bit."""
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest

import __graft_entry__ as ge

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "scan_generate.npz"))
CALLS = [str(c) for c in G["calls"]]
VARIANT = int(G["sincos_variant"])  # (the build of sincos the generating host ran; its libm_variant is recorded too)


@pytest.fixture(scope="module")
def pkg():
    p = ge.load_package()
    if not os.path.exists(p.LIB_PATH):
        p.build()
    return p


def golden_map(c):
    return types.SimpleNamespace(cell_model=int(G[c + "_cell_model"]), payload=G[c + "_payload"], origin=tuple(G[c + "_origin"]),
                                 scale=float(G[c + "_scale"]), unknown=G[c + "_unknown"], width=G[c + "_payload"].shape[1],
                                 height=G[c + "_payload"].shape[0])


def golden_call(pkg, c):
    max_dist, fov, pts = G[c + "_lsp"]
    _, inc, hs = pkg.to_lsp(max_dist, fov, int(pts))
    return golden_map(c), G[c + "_poses"], pkg.scan_gen_angles(hs, inc), float(max_dist), float(G[c + "_threshold"])


@pytest.mark.parametrize("k", range(4))
def test_angle_lists_are_the_references(pkg, k):
    max_dist, fov, pts = G["angles_%d_params" % k]
    _, inc, hs = pkg.to_lsp(max_dist, fov, int(pts))
    np.testing.assert_array_equal(pkg.scan_gen_angles(hs, inc), G["angles_%d" % k])


def test_the_two_pi_break_and_the_full_circle(pkg):
    # the default LaserScannerParams (15, 90 deg, half sector pi) stop at the 2 pi break: 4 angles, not 5
    assert pkg.scan_gen_angles(np.pi, 90 * np.pi / 180).size == 4
    assert G["angles_2"].size == 4 and G["angles_3"].size == 60


@pytest.mark.parametrize("c", CALLS)
def test_host_scans_equal_the_references(pkg, c):
    m, poses, angles, max_dist, thr = golden_call(pkg, c)
    rng, status = pkg.generate_scans_host(m, poses, angles, max_dist, thr, int(G[c + "_occ_kind"]), VARIANT)
    np.testing.assert_array_equal(status, G[c + "_status"])
    np.testing.assert_array_equal(rng, G[c + "_range"])
    for k, scan in enumerate(pkg.compact_scans(rng, status, angles)):
        hit = G[c + "_status"][k] == 1
        np.testing.assert_array_equal(scan[0], G[c + "_range"][k][hit])
        np.testing.assert_array_equal(scan[1], angles[hit])
        assert scan[2].all() and scan[2].size == int(hit.sum())


def test_the_golden_holds_the_cases(pkg):
    steps = np.concatenate([G[c + "_hit_step"].ravel() for c in CALLS])
    assert np.any(steps < 0) and np.any((steps >= 0) & (steps < 64)) and np.any(steps >= 64)
    assert {int(G[c + "_cell_model"]) for c in CALLS} >= {pkg.CELL_OCC, pkg.CELL_TBM, pkg.CELL_GMAPPING}
    assert {float(G[c + "_scale"]) for c in CALLS} == {0.1, 0.05}


# ---- far from the world origin: tests/golden/placed_generate.npz (make_golden_placed_generate.py), the reference's scans on
# windows 1000 ... 2000 m out, one station per quadrant
P = np.load(os.path.join(ROOT, "tests", "golden", "placed_generate.npz"))
P_CALLS = [str(c) for c in P["calls"]]
P_VARIANT = int(P["sincos_variant"])


def placed_map(name):
    return types.SimpleNamespace(cell_model=int(P[name + "_cell_model"]), payload=P[name + "_payload"],
                                 origin=tuple(int(v) for v in P[name + "_origin"]), scale=float(P[name + "_scale"]),
                                 unknown=P[name + "_unknown"], width=P[name + "_payload"].shape[1], height=P[name + "_payload"].shape[0])


def placed_call(pkg, c):
    max_dist, fov, pts = P[c + "_lsp"]
    _, inc, hs = pkg.to_lsp(max_dist, fov, int(pts))
    return placed_map(str(P[c + "_map"])), P[c + "_poses"], pkg.scan_gen_angles(hs, inc), float(max_dist), float(P[c + "_threshold"])


@pytest.mark.parametrize("c", P_CALLS)
def test_host_scans_equal_the_references_far_from_the_origin(pkg, c):
    m, poses, angles, max_dist, thr = placed_call(pkg, c)
    assert 37 <= angles.size <= 90
    rng, status = pkg.generate_scans_host(m, poses, angles, max_dist, thr, int(P[c + "_occ_kind"]), P_VARIANT)
    np.testing.assert_array_equal(status, P[c + "_status"])
    np.testing.assert_array_equal(rng, P[c + "_range"])


def test_the_far_golden_holds_the_cases(pkg):
    import placed_scenes as ps
    keys = [str(k) for k in P["stat_keys"]]
    for st in ps.Q_STATIONS:
        (kx, ky), _ = ps.STATIONS[st]
        s = dict(zip(keys, P[st + "_stats"]))
        for k in ("robot_outside", "tie", "astray", "touch", "leaves_window", "hit_early", "hit_late", "no_hit", "short_walks"):
            assert s[k] > 0, (st, k)
        assert s["max_cells"] > 1000
        models = set()
        for name in ("cecum", "mean", "tbm", "gmapping"):
            m = placed_map("%s_%s" % (st, name))
            models.add(m.cell_model)
            assert not (0 <= m.origin[0] < m.width) and not (0 <= m.origin[1] < m.height)  # (0, 0) is no cell of the window
            assert (m.width // 2 - m.origin[0], m.height // 2 - m.origin[1]) == (kx, ky)
        assert models == {pkg.CELL_OCC, pkg.CELL_TBM, pkg.CELL_GMAPPING}
        steps = np.concatenate([P[c + "_hit_step"].ravel() for c in P_CALLS if c.startswith(st)])
        assert np.any(steps == -1) and np.any((steps >= 0) & (steps < 64)) and np.any(steps >= 64)
    # the scenes are one scene moved by whole cells, and still no two stations' ranges are the same doubles
    a, b = P["Q1_cecum_long_range"], P["Q3_cecum_long_range"]
    assert np.array_equal(a != 0, b != 0) and not np.array_equal(a, b)
    np.testing.assert_allclose(a, b, rtol=0, atol=1e-3)


def test_robot_on_a_cell_boundary_is_invalid(pkg):
    m, poses, angles, max_dist, thr = golden_call(pkg, "cecum_short")
    for bad in ([0.2, 0.123, 0.0], [0.123, -0.2, 0.0], [0.2 + 1e-9, 0.123, 0.0]):  # (floor(x / scale) * scale is x)
        with pytest.raises(pkg.SlamHipError, match="cell boundary"):
            pkg.generate_scans_host(m, [poses[0], bad], angles, max_dist, thr, 0, VARIANT)
    with pytest.raises(pkg.SlamHipError):
        pkg.generate_scans_host(m, [[np.nan, 0.1, 0.0]], angles, max_dist, thr, 0, VARIANT)
    with pytest.raises(pkg.SlamHipError):
        pkg.generate_scans_host(m, poses, angles, max_dist, thr, 1, VARIANT)  # occ_kind 1 on an OCC map


def test_a_status_2_pose_has_no_compact_scan(pkg):
    out = pkg.compact_scans(np.array([[1.0, 0.0], [2.0, 3.0]]), np.array([[1, 2], [1, 1]], np.uint8), [0.1, 0.2])
    assert out[0] is None and out[1][0].tolist() == [2.0, 3.0]


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_per_beam_routine_under_sanitizers(tmp_path):
    """tests/native/scan_generate_test.cpp under -fsanitize=address,undefined: the host routine over random maps, walks of
    every kind (ties, astray walks, beams that leave the window); the kernel's wave form emulated lane after lane with
    the functions the kernel calls -- every beam it settles equals the sequential routine, and it settles at least 80 %
    of them; the restated sincos against the running libm's over 2e6 arguments."""
    hip_inc = "/opt/rocm/include"
    if not os.path.exists(os.path.join(hip_inc, "hip", "hip_runtime.h")):
        pytest.skip("HIP headers not found")
    exe = str(tmp_path / "scan_generate_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__", "-I" + hip_inc, "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "slam-constructor_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "scan_generate_test.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok wave form settled ")
    fma, plain = (int(v) for v in re.search(r"sincos mismatches fma (\d+) plain (\d+)", r.stdout).groups())
    want = ge.load_package().scan_gen_libm_variant(strict=False)
    # the build the library's probe names equals the running libm everywhere (a libm that is neither: nothing to hold)
    assert want == -1 or (fma, plain)[1 - want] == 0, r.stdout
