"""CPU suite: the reference-side surface of the batched scorer (host/slamhip_reference_adapter.h) --
hip_estimate_scan_probabilities: K (filtered LaserScan2D, GridMap, pose list) triples through ONE
slamhip_score_poses_batch call -- compiled against the reference's headers where they are present (-fsyntax-only:
nothing of the reference is linked or run), and the ctypes layout of slamhip_score_job against a small C program's
sizeof / offsetof."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

import __graft_entry__ as ge

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = os.environ.get("REFERENCE", "/root/reference")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_the_batch_scorer_adapter_compiles_against_the_reference(tmp_path):
    if not os.path.isfile(os.path.join(REFERENCE, "src", "core", "scan_matchers", "grid_scan_matcher.h")):
        pytest.skip("the reference tree is not present")
    src = tmp_path / "adapter_check.cpp"
    src.write_text('''#include "slamhip_reference_adapter.h"
std::vector<std::vector<double>> use(slamhip_ctx *ctx, const slamhip_spe_cfg &cfg, const ScanProbabilityEstimator::SPEParams &params,
                                     const LaserScan2D &a, const LaserScan2D &b, const GridMap &map, HipMapMirror &mirror,
                                     const RobotPose &p) {
  std::vector<HipScoreJob> jobs = {HipScoreJob{&a, &map, &mirror, {p, p, p}}, HipScoreJob{&b, &map, &mirror, {p}}};
  HipScanTrig cached;
  cached.mode = SLAMHIP_TRIG_CACHED;
  std::vector<std::vector<double>> s = hip_estimate_scan_probabilities(ctx, cfg, params, jobs, 1, cached, 8);
  std::vector<std::vector<double>> t = hip_estimate_scan_probabilities(ctx, cfg, params, jobs, 0);
  s.insert(s.end(), t.begin(), t.end());
  return s;
}
int main() { return 0; }
''')
    cmd = ["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-I" + os.path.join(REFERENCE, "src"), "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "slam-constructor_amd", "host"), str(src)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]


@pytest.mark.skipif(shutil.which("g++") is None and shutil.which("gcc") is None, reason="no host compiler")
def test_new_symbols_and_the_layout_of_the_score_job(tmp_path):
    pkg = ge.load_package()
    for sym in ("slamhip_score_poses_batch", "slamhip_score_poses_batch_stats"):
        assert sym in pkg.EXPORTS, sym
    assert hasattr(pkg.Context, "score_poses_batch") and hasattr(pkg.Context, "score_poses_batch_stats")
    src = tmp_path / "layout.c"
    src.write_text("""#include <stddef.h>
#include <stdio.h>
#include "slamhip.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu\\n", sizeof(slamhip_score_job), offsetof(slamhip_score_job, map_id),
         offsetof(slamhip_score_job, scan_slot), offsetof(slamhip_score_job, n_poses), offsetof(slamhip_score_job, poses_xyt));
  return 0;
}
""")
    exe = str(tmp_path / "layout")
    cc = shutil.which("gcc") or "g++"
    subprocess.run([cc] + (["-x", "c"] if cc == "g++" else []) + ["-I" + os.path.join(ROOT, "include"), str(src), "-o", exe],
                   check=True, capture_output=True, text=True, timeout=120)
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    J = pkg.ScoreJob
    assert got == [C.sizeof(J), J.map_id.offset, J.scan_slot.offset, J.n_poses.offset, J.poses_xyt.offset]
