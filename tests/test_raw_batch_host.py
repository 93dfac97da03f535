"""CPU suite: the host half of slamhip_matcher_process_raw_scan_batch.  tests/native/raw_batch_stage_test.cpp compiles
csrc/scan_filter.cpp (RawBatchStage: per job the lone call's filter and rows, the scanners' tables, the layout of the
one pinned arena) into a stand-alone program and holds it to the library's public host functions -- kept indices, kept
ranges, factors, ahr weights and the weight sums as bytes, rows 16-byte aligned and disjoint, one table per distinct
scanner, a job that keeps nothing, a map's rim that drops points -- once at -O2 and once under ASan / UBSan.  The new
symbols and the ctypes layout of slamhip_raw_match_job are held to a small C program's sizeof / offsetof."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

import __graft_entry__ as ge

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "slam-constructor_amd", "csrc")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")


@pytest.fixture(scope="module")
def pkg():
    p = ge.load_package()
    if not os.path.exists(p.LIB_PATH):
        p.build()
    return p


def _build(pkg, tmp_path, name, flags):
    exe = str(tmp_path / name)
    libdir = os.path.dirname(pkg.LIB_PATH)
    cmd = ["g++", "-std=c++17", "-ffp-contract=off", "-I" + CSRC, "-I" + os.path.join(ROOT, "include")] + flags + [
        os.path.join(ROOT, "tests", "native", "raw_batch_stage_test.cpp"), os.path.join(CSRC, "scan_filter.cpp"),
        "-L" + libdir, "-lslamhip", "-Wl,-rpath," + libdir, "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=600)
    return exe


def test_stage_equals_the_public_host_functions(pkg, tmp_path):
    r = subprocess.run([_build(pkg, tmp_path, "raw_batch_stage_test", ["-O2"])], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok ") and int(r.stdout.split()[1]) >= 500, r.stdout


def test_stage_under_sanitizers(pkg, tmp_path):
    """The same stand-alone program under ASan / UBSan: the arena is a heap block of exactly arena_bytes."""
    exe = _build(pkg, tmp_path, "raw_batch_stage_test_san", ["-O1", "-g", "-fsanitize=address,undefined",
                                                             "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok ") and int(r.stdout.split()[1]) >= 500, r.stdout


def test_new_symbols_and_the_layout_of_a_raw_match_job(pkg, tmp_path):
    lib = pkg.load()
    for sym in ("slamhip_matcher_process_raw_scan_batch", "slamhip_matcher_batch_scan_download"):
        assert sym in pkg.EXPORTS and hasattr(lib, sym), sym
    src = tmp_path / "layout.c"
    src.write_text("""#include <stddef.h>
#include <stdio.h>
#include "slamhip.h"
int main(void) {
  printf("%zu %zu %zu %zu\\n", sizeof(slamhip_raw_match_job), offsetof(slamhip_raw_match_job, map_id),
         offsetof(slamhip_raw_match_job, scan), offsetof(slamhip_raw_match_job, init_pose));
  printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(slamhip_raw_scan), offsetof(slamhip_raw_scan, range),
         offsetof(slamhip_raw_scan, is_occ), offsetof(slamhip_raw_scan, trig_mode), offsetof(slamhip_raw_scan, skip_rate),
         offsetof(slamhip_raw_scan, max_range), offsetof(slamhip_raw_scan, weighting));
  return 0;
}
""")
    exe = str(tmp_path / "layout")
    cc = shutil.which("gcc") or "g++"
    subprocess.run([cc] + (["-x", "c"] if cc == "g++" else []) + ["-I" + os.path.join(ROOT, "include"), str(src), "-o", exe],
                   check=True, capture_output=True, text=True, timeout=120)
    job, scan = [[int(v) for v in ln.split()] for ln in subprocess.run([exe], capture_output=True, text=True,
                                                                       check=True).stdout.splitlines()]
    J, S = pkg.RawMatchJob, pkg.RawScan
    assert job == [C.sizeof(J), J.map_id.offset, J.scan.offset, J.init_pose.offset]
    assert scan == [C.sizeof(S), S.range.offset, S.is_occ.offset, S.trig_mode.offset, S.skip_rate.offset, S.max_range.offset,
                    S.weighting.offset]
    # make_raw_batch needs no GPU: the block it makes carries the jobs' values
    import numpy as np
    blk = pkg.Matcher.make_raw_batch(None, [dict(map_id=3, range=np.ones(5), angle=np.arange(5.0), init_pose=(1, 2, 3),
                                                 weighting="ahr", skip_rate=2, bounded=True, trig_mode=pkg.TRIG_CACHED,
                                                 a_min=-1.0, a_max=1.0, a_inc=0.5)])
    a = blk["raw_arr"][0]
    assert (a.map_id, a.scan.n, a.scan.weighting, a.scan.skip_rate, a.scan.bounded, a.scan.trig_mode) == (3, 5, 2, 2, 1, 1)
    assert list(a.init_pose) == [1.0, 2.0, 3.0] and a.scan.a_inc == 0.5 and a.scan.range[4] == 1.0
