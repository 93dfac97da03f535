"""CPU suite of the batched Monte-Carlo matching (slamhip_matcher_set_mc_streams): the lock-step logic of K chains on K
engine streams against K plain accept loops (tests/native/mc_batch_test.cpp, a stand-alone program: optimised and under
ASan / UBSan), the new entry points in the package's export list and in the header, and the reference-side adapter with
set_mc_streams compiled against the unmodified reference headers."""
import os
import shutil
import subprocess

import pytest

import __graft_entry__ as ge

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = os.environ.get("REFERENCE", "/root/reference")
HIP_INC = "/opt/rocm/include"
NEW = ["slamhip_matcher_set_mc_streams", "slamhip_matcher_set_mc_job_streams", "slamhip_matcher_mc_stream_info"]


@pytest.fixture(scope="module")
def sources():
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    if not os.path.exists(os.path.join(HIP_INC, "hip", "hip_runtime.h")):
        pytest.skip("HIP headers not found")
    return ["-std=c++17", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I" + HIP_INC, "-I" + os.path.join(ROOT, "include"),
            "-I" + os.path.join(ROOT, "slam-constructor_amd", "csrc"), os.path.join(ROOT, "tests", "native", "mc_batch_test.cpp"),
            os.path.join(ROOT, "slam-constructor_amd", "csrc", "mt_block.cpp")]


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                             "-fno-omit-frame-pointer"]], ids=["O2", "asan_ubsan"])
def test_interleaved_chains_equal_the_plain_loops(tmp_path, sources, flags):
    """K in {1, 2, 5, 20} chains in lock-step, S in {1, 2, 7, 20, 511} candidates per chain and super-step, limits from
    1/5 to 600/1200, quantised scores (ties), three consecutive calls per set of streams: 5040 matches, each equal to
    its plain loop in trace, final pose, pairs consumed and enumerator state."""
    exe = str(tmp_path / "mc_batch_test")
    subprocess.run(["g++"] + flags + sources + ["-o", exe], check=True, capture_output=True, text=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok 5040 matches"), r.stdout


def test_the_new_entry_points_are_exported_and_declared():
    pkg = ge.load_package()
    assert not [s for s in NEW if s not in pkg.EXPORTS]
    header = open(os.path.join(ROOT, "include", "slamhip.h")).read()
    assert not [s for s in NEW if "int %s(" % s not in header]
    for testing in (False, True):
        lib = pkg.load(testing)
        assert not [s for s in NEW if not hasattr(lib, s)]
    # the speculation-width hook is the testing library's alone
    assert hasattr(pkg.load(True), "slamhip_matcher_testing_mc_batch_slots")
    assert not hasattr(pkg.load(False), "slamhip_matcher_testing_mc_batch_slots")
    for name in ("set_mc_streams", "set_mc_job_streams", "mc_stream_info"):
        assert callable(getattr(pkg.Matcher, name))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_the_adapter_with_engine_streams_compiles_against_the_reference(tmp_path):
    if not os.path.isfile(os.path.join(REFERENCE, "src", "core", "scan_matchers", "grid_scan_matcher.h")):
        pytest.skip("reference tree not present")
    tu = tmp_path / "tu.cpp"
    tu.write_text('#include "slamhip_reference_adapter.h"\n'
                  "double use(HipGridScanMatcher &a, HipGridScanMatcher &b, const TransformedLaserScan &s, const RobotPose &p,\n"
                  "           const GridMap &m) {\n"
                  "  a.set_mc_streams(std::vector<unsigned>{7u, 11u});\n"
                  "  std::vector<HipRawScanJob> jobs;\n"
                  "  jobs.push_back(HipRawScanJob{&a, &s, &p, &m, RobotPoseDelta{}, 0.0});\n"
                  "  jobs.push_back(HipRawScanJob{&b, &s, &p, &m, RobotPoseDelta{}, 0.0});\n"
                  "  hip_process_raw_scans(a, jobs);\n"
                  "  a.set_mc_streams({});\n"
                  "  return jobs[0].prob + jobs[1].pose_delta.x;\n}\n")
    cmd = ["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-I" + os.path.join(REFERENCE, "src"),
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "slam-constructor_amd", "host"), str(tu)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "slamhip_reference_adapter.h" not in r.stderr, r.stderr[-4000:]  # (no warning from the adapter itself)
