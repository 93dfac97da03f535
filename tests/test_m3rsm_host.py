"""CPU suite: the best-first engine of the multi-resolution matcher (csrc/m3rsm_engine.cpp, host C++ without HIP) replayed
against tests/golden/m3rsm.npz -- whole matches of the compiled reference's BruteForceMultiResolutionScanMatcher with the
full trace of its scorer calls (tests/golden/make_golden_m3rsm.py) -- through tests/native/m3rsm_engine_test.cpp, plainly
and under -fsanitize=address,undefined; what the golden holds; the reference-side adapter headers against the reference."""
import os
import shutil
import subprocess

import numpy as np
import pytest
from m3rsm_cases import N_SCENES, SCENE_NAMES, children, golden_scene, host_slots

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "slam-constructor_amd", "csrc")
REFERENCE = os.environ.get("REFERENCE", "/root/reference")


def scenes_file(path):
    flat = [float(N_SCENES)]
    for i in range(N_SCENES):
        s = golden_scene(i)
        flat += [*s.limits, *s.delta, s.prob, float(len(s.trace)), *s.trace.ravel()]
    np.asarray(flat, dtype=np.float64).tofile(path)
    return path


def run_engine_test(tmp_path, extra):
    exe = str(tmp_path / "m3rsm_engine_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", *extra, "-I" + CSRC,
           os.path.join(ROOT, "tests", "native", "m3rsm_engine_test.cpp"), os.path.join(CSRC, "m3rsm_engine.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300)
    r = subprocess.run([exe, scenes_file(str(tmp_path / "scenes.bin"))], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok %d scenes" % N_SCENES), r.stdout


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_engine_replays_the_reference_for_every_width_and_depth(tmp_path):
    run_engine_test(tmp_path, [])


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_engine_under_asan_and_ubsan(tmp_path):
    run_engine_test(tmp_path, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])


def test_the_golden_holds_the_cases():
    sc = [golden_scene(i) for i in range(N_SCENES)]
    assert SCENE_NAMES == ["occ_square", "occ_oblong", "occ_step07", "occ_1beam", "tbm_square", "cred_square"]
    assert {(s.cell_model, s.oie) for s in sc} == {(0, 0), (1, 0), (3, 0)}
    by = {s.name: s for s in sc}
    assert by["occ_oblong"].limits[0] != by["occ_oblong"].limits[1]
    assert tuple(by["occ_step07"].limits[[0, 1, 4]]) == (0.3, 0.45, 0.07)
    one = by["occ_1beam"]
    assert len(one.scan) == 1 and (one.width, one.height, one.origin, one.scale) == (37, 29, (11, 20), 0.05)
    one_sided, five, levels = 0, 0, set()
    for s in sc:
        assert 40 <= len(s.trace) <= 4500 and np.all(np.isfinite(s.trace))
        assert np.all(s.scan[:, 3] == s.scan[0, 3]) and np.all(s.scan[:, 4] == 1.0)  # even weights
        levels |= set(s.trace[:, 6].astype(int).tolist())
        # every call is a root or a child, by the rule, of an earlier call at the same rotation
        seen = {}
        n_roots = 2 * len(set(s.trace[:, 0].tolist()))
        for j, row in enumerate(s.trace):
            k = row[:5].tobytes()
            if j < n_roots:
                assert np.all(row[1:5] == 0) or np.array_equal(row[1:5], [-s.limits[1], s.limits[1], -s.limits[0], s.limits[0]])
            else:
                assert k in seen, "%s: call %d has no parent on record" % (s.name, j)
                one_sided += seen[k] == (2, 0)
                five += seen[k] == (5, 4)
            kids = children(row[1:5], s.limits[4])
            for c, kid in enumerate(kids):
                seen[np.asarray([row[0], *kid]).tobytes()] = (len(kids), c)
        # the result is the bound of a point on record
        pts = s.trace[(s.trace[:, 1] == s.trace[:, 2]) & (s.trace[:, 3] == s.trace[:, 4])]
        hit = (pts[:, 3] == s.delta[0]) & (pts[:, 1] == s.delta[1]) & (pts[:, 0] == s.delta[2]) & (pts[:, 5] == s.prob)
        assert hit.any()
    assert one_sided >= 10 and five >= 50 and len(levels) >= 4
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "m3rsm.npz")) <= 930 * 1024


def test_host_slot_layout():
    """the numpy restatement the GPU tests compare the expand kernel with: breadth first, five slots per node"""
    s = host_slots((0.0, 0.4, 0.0, 0.2), 0.05, 2)
    assert s.shape == (30, 4) and np.all(np.isfinite(s[:4])) and np.all(np.isnan(s[4]))
    assert np.array_equal(s[0], [0.0, 0.2, 0.0, 0.1]) and np.array_equal(s[5 + 5 * 0 + 1], [0.1, 0.2, 0.0, 0.05])
    assert np.all(np.isnan(s[5 + 5 * 4:]))  # the fifth child slot is empty, and so are its children
    p = host_slots((0.0, 0.04, 0.0, 0.04), 0.05, 3)
    assert np.all(np.isfinite(p[:5])) and np.all(np.isnan(p[5:]))  # five points, which have no children
    assert np.all(np.isnan(host_slots((0.3, 0.1, 0.0, 1.0), 0.05, 1)))  # reversed: no children


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_adapter_headers_compile_against_the_reference(tmp_path):
    if not os.path.isfile(os.path.join(REFERENCE, "src", "utils", "init_scan_matching.h")):
        pytest.skip("the reference tree is not present")
    src = tmp_path / "adapter_check.cpp"
    src.write_text('#include "slamhip_init_scan_matching.h"\n#include "slamhip_m3rsm_map.h"\nint main() { return 0; }\n')
    cmd = ["g++", "-std=c++14", "-fsyntax-only", "-w", "-I" + os.path.join(REFERENCE, "src"), "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "slam-constructor_amd", "host"), str(src)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
