"""CPU suite: the planning of slamhip_pyramid_refresh_batch (csrc/pyr_refresh_batch_plan.h, plain C++ without HIP)
through tests/native/pyr_refresh_batch_plan_test.cpp -- every coarse cell whose block meets a job's window assigned
exactly once, to a flat launch or to the tail; the tail from the first level of at most 256 cells to the top; block
offsets that partition each flat grid; equal pyramids never in one round; a refused call leaving the plan as it was --
built and run as a stand-alone native program, plainly and under -fsanitize=address,undefined.  A second program,
tests/native/raw_stage_six_rows_test.cpp, drives RawBatchStage (csrc/scan_filter.cpp) with the six-row block layout of
slamhip_matcher_m3rsm_match_each_raw for requests that keep 0, 1 and 257 points, the same two ways."""
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
def test_plan(tmp_path, extra):
    exe = str(tmp_path / "pyr_refresh_batch_plan_test")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *extra, "-I" + CSRC,
                        os.path.join(NATIVE, "pyr_refresh_batch_plan_test.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert r.stdout.splitlines()[-1] == "ok pyr refresh batch plan", r.stdout


@needs_gxx
@pytest.mark.parametrize("extra", [[], ASAN], ids=["plain", "asan_ubsan"])
def test_raw_stage_with_a_six_row_layout(tmp_path, extra):
    exe = str(tmp_path / "raw_stage_six_rows_test")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", *extra, "-I" + CSRC,
                        os.path.join(NATIVE, "raw_stage_six_rows_test.cpp"), os.path.join(CSRC, "scan_filter.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert r.stdout.splitlines()[-1] == "ok raw stage six rows", r.stdout


def test_the_header_is_free_of_hip():
    text = open(os.path.join(CSRC, "pyr_refresh_batch_plan.h")).read()
    assert "#include <hip" not in text and "slamhip_internal.h" not in text and '#include "map_pyramid' not in text
