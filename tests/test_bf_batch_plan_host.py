"""CPU suite: the bookkeeping of K brute-force enumerator streams on one matcher (csrc/bf_batch_plan.h, plain C++ without
HIP) through tests/native/bf_batch_plan_test.cpp -- latching over several calls, identity and explicit job mappings, every
refusal leaving the state as it was, an empty raw job that does not latch, reset keeping the bases -- built and run as a
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
def test_stream_bookkeeping(tmp_path, extra):
    exe = str(tmp_path / "bf_batch_plan_test")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *extra, "-I" + CSRC,
                        os.path.join(NATIVE, "bf_batch_plan_test.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert r.stdout.splitlines()[-1] == "ok bf batch plan", r.stdout


def test_the_header_is_free_of_hip():
    text = open(os.path.join(CSRC, "bf_batch_plan.h")).read()
    assert "#include <hip" not in text and "slamhip_internal.h" not in text
