"""CPU suite: K independent multi-resolution searches in lock-step (m3rsm::run_each, csrc/m3rsm_each.cpp over the resumable
Search of csrc/m3rsm_engine.cpp, host C++ without HIP) replayed against tests/golden/m3rsm.npz -- all lone scenes of the
compiled reference in ONE batch, each with its own limits -- through tests/native/m3rsm_each_engine_test.cpp: plainly,
under -fsanitize=address,undefined and, where the host compiler has the runtime, under -fsanitize=thread.  The two
earlier native programs (run, run_many) are built and run again the same way: both drive the same resumable object."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import m3rsm_cases as lone_cases
import m3rsm_many_cases as many_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "slam-constructor_amd", "csrc")
NATIVE = os.path.join(ROOT, "tests", "native")
ENGINE = [os.path.join(CSRC, "m3rsm_engine.cpp"), os.path.join(CSRC, "m3rsm_each.cpp")]
ASAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
TSAN = ["-fsanitize=thread", "-fno-omit-frame-pointer"]

needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")


def lone_file(path):
    flat = [float(lone_cases.N_SCENES)]
    for i in range(lone_cases.N_SCENES):
        s = lone_cases.golden_scene(i)
        flat += [*s.limits, *s.delta, s.prob, float(len(s.trace)), *s.trace.ravel()]
    np.asarray(flat, dtype=np.float64).tofile(path)
    return path


def many_file(path):
    flat = [float(many_cases.N_SCENES)]
    for i in range(many_cases.N_SCENES):
        s = many_cases.golden_scene(i)
        flat += [*s.limits, float(len(s.requests)), float(s.winner), *s.delta, s.prob, float(len(s.trace)), *s.trace.ravel()]
    np.asarray(flat, dtype=np.float64).tofile(path)
    return path


def build(tmp_path, program, sources, extra):
    exe = str(tmp_path / program)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-pthread", *extra, "-I" + CSRC,
           os.path.join(NATIVE, program + ".cpp"), *sources, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    return exe, r


def run_each_test(tmp_path, extra):
    exe, r = build(tmp_path, "m3rsm_each_engine_test", ENGINE, extra)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe, lone_file(str(tmp_path / "lone.bin"))], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert r.stdout.splitlines()[-1].startswith("ok %d jobs in a batch" % lone_cases.N_SCENES), r.stdout


@needs_gxx
def test_lock_step_searches_replay_every_lone_match(tmp_path):
    run_each_test(tmp_path, [])


@needs_gxx
def test_lock_step_searches_under_asan_and_ubsan(tmp_path):
    run_each_test(tmp_path, ASAN)


@needs_gxx
def test_lock_step_searches_under_tsan(tmp_path):
    probe = tmp_path / "probe.cpp"
    probe.write_text("#include <thread>\nint main() { std::thread t([] {}); t.join(); return 0; }\n")
    exe = str(tmp_path / "probe")
    r = subprocess.run(["g++", "-std=c++17", "-pthread", *TSAN, str(probe), "-o", exe], capture_output=True, text=True, timeout=300)
    if r.returncode != 0 or subprocess.run([exe], capture_output=True, timeout=60).returncode != 0:
        pytest.skip("the host compiler has no thread sanitizer runtime that runs here")
    run_each_test(tmp_path, TSAN)


@needs_gxx
@pytest.mark.parametrize("extra", [[], ASAN], ids=["plain", "asan_ubsan"])
def test_run_and_run_many_still_give_their_goldens(tmp_path, extra):
    # the two earlier programs, over the engine as the library builds it (m3rsm_each.cpp beside it)
    exe, r = build(tmp_path, "m3rsm_engine_test", ENGINE, extra)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe, lone_file(str(tmp_path / "lone.bin"))], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok %d scenes" % lone_cases.N_SCENES), r.stdout + r.stderr
    exe, r = build(tmp_path, "m3rsm_many_engine_test", ENGINE, extra)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe, many_file(str(tmp_path / "many.bin")), str(tmp_path / "lone.bin")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok %d + %d scenes" % (many_cases.N_SCENES, lone_cases.N_SCENES)), r.stdout


def test_the_batch_holds_scenes_with_different_limits():
    limits = {tuple(lone_cases.golden_scene(i).limits) for i in range(lone_cases.N_SCENES)}
    assert lone_cases.N_SCENES == 6 and len(limits) >= 3
