"""CPU suite: the walk that carries the GMapping OOPE's run cache from pose to pose (csrc/gm_carry.h, plain C++ without
HIP: the text k_gm_carry_jobs of csrc/gm_score_batch.hip runs, one lane per job) through tests/native/gm_carry_test.cpp
-- against a plain per-beam simulation of the reference's cache over seeded random cell sequences: runs that span a pose
boundary, runs that cover a whole pose (the carried value handed through), tot_w == 0, single-beam scans, the empty-cache
start, pose counts around the walk's chunk -- built and run as a stand-alone native program, plainly and under
-fsanitize=address,undefined."""
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
def test_the_walk_equals_the_per_beam_cache(tmp_path, extra):
    exe = str(tmp_path / "gm_carry_test")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror", *extra, "-I" + CSRC,
                        os.path.join(NATIVE, "gm_carry_test.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert r.stdout.splitlines()[-1] == "ok gm carry", r.stdout


def test_the_header_is_free_of_hip_and_the_kernel_runs_its_text():
    text = open(os.path.join(CSRC, "gm_carry.h")).read()
    assert "#include" not in text
    kernel = open(os.path.join(CSRC, "gm_score_batch.hip")).read()
    assert "gm_carry_walk(" in kernel and "gm_carry_empty()" in kernel
    assert '#include "gm_carry.h"' in open(os.path.join(CSRC, "slamhip_internal.h")).read()
