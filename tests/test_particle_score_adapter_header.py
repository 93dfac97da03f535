"""CPU suite: host/slamhip_gmapping_adapter.h compiles against the unmodified reference headers with
hip_estimate_particle_scan_probabilities instantiated (slamhip_gmapping_particle_score_poses: pose sets scored over a
GMapping filter's per-particle maps), alone and beside host/slamhip_reference_adapter.h."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = os.environ.get("REFERENCE", "/root/reference")

USE = ("std::vector<std::vector<double>> use(slamhip_ctx *ctx, slamhip_gmapping *filter, const LaserScan2D &scan,\n"
       "                                     const LaserScan2D &other, const RobotPose &pose) {\n"
       "  slamhip_spe_cfg cfg{};\n"
       "  cfg.gm_fullness_th = 0.1;\n"
       "  cfg.gm_window = 1;\n"
       "  std::vector<HipParticleScoreJob> jobs;\n"
       "  jobs.push_back(HipParticleScoreJob{0, &scan, std::vector<RobotPose>(5, pose)});\n"
       "  jobs.push_back(HipParticleScoreJob{3, &scan, {}});\n"
       "  jobs.push_back(HipParticleScoreJob{3, &other, std::vector<RobotPose>(1, pose)});\n"
       "  std::vector<std::vector<double>> p = hip_estimate_particle_scan_probabilities(ctx, filter, cfg, jobs);\n"
       "  std::vector<std::vector<double>> q = hip_estimate_particle_scan_probabilities(ctx, filter, cfg, jobs, 0, 16);\n"
       "  p.insert(p.end(), q.begin(), q.end());\n"
       "  return p;\n"
       "}\n")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
@pytest.mark.parametrize("beside", [False, True], ids=["alone", "beside_the_reference_adapter"])
def test_gmapping_adapter_header_compiles_with_the_particle_score_call(tmp_path, beside):
    if not os.path.isfile(os.path.join(REFERENCE, "src", "slams", "gmapping", "gmapping_particle_filter.h")):
        pytest.skip("reference tree not present")
    tu = tmp_path / "tu.cpp"
    tu.write_text(('#include "slamhip_reference_adapter.h"\n' if beside else "") + '#include "slamhip_gmapping_adapter.h"\n' + USE)
    cmd = ["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-I" + os.path.join(REFERENCE, "src"), "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "slam-constructor_amd", "host"), str(tu)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "slamhip_gmapping_adapter.h" not in r.stderr, r.stderr[-4000:]  # (no warning of the header's own)


def test_the_call_is_declared_and_exported():
    import __graft_entry__ as ge
    pkg = ge.load_package()
    header = open(os.path.join(ROOT, "include", "slamhip.h")).read()
    for sym in ("slamhip_gmapping_particle_score_poses", "slamhip_gmapping_particle_score_stats"):
        assert sym in pkg.EXPORTS and sym + "(" in header, sym
    assert "slamhip_particle_score_job;" in header
    assert hasattr(pkg.GmappingFilter, "score_particle_poses") and hasattr(pkg.GmappingFilter, "particle_score_stats")
