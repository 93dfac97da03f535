"""CPU suite: the planning of slamhip_score_poses_batch (csrc/score_batch_plan.h, plain C++ without HIP) through
tests/native/score_batch_plan_test.cpp -- every workgroup of the flat scoring grid inside one job, every pose covered
once, offsets summing to the totals, empty jobs, the ragged totals 1023 / 1024 / 2048 / 8192 under every
poses-per-workgroup value, the beam-order budget's routing at the budget and one term beyond -- built and run as a
stand-alone native program, plainly and under -fsanitize=address,undefined."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "slam-constructor_amd", "csrc")
NATIVE = os.path.join(ROOT, "tests", "native")
ASAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]

needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")


@needs_gxx
@pytest.mark.parametrize("extra", [[], ASAN], ids=["plain", "asan_ubsan"])
def test_block_table_offsets_and_routing(tmp_path, extra):
    exe = str(tmp_path / "score_batch_plan_test")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *extra, "-I" + CSRC,
                        os.path.join(NATIVE, "score_batch_plan_test.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert r.stdout.splitlines()[-1] == "ok score batch plan", r.stdout


def test_the_header_is_free_of_hip():
    text = open(os.path.join(CSRC, "score_batch_plan.h")).read()
    assert "#include <hip" not in text and "slamhip_internal.h" not in text and '#include "slamhip' not in text


def test_the_restated_poses_per_block_thresholds_are_the_launchers():
    """the native test restates pick_poses_per_block (csrc/kernel_pick.h includes the HIP runtime's header): both texts
    carry the same three thresholds"""
    pick = open(os.path.join(CSRC, "kernel_pick.h")).read()
    test = open(os.path.join(NATIVE, "score_batch_plan_test.cpp")).read()
    for needle in ("n_poses >= 8192) return 8", "n_poses >= 2048) return 4", "n_poses >= 1024) return 2"):
        assert needle in pick, needle
    assert "n >= 8192 ? 8 : (n >= 2048 ? 4 : (n >= 1024 ? 2 : 1))" in test
