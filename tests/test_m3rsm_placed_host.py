"""CPU suite: the best-first engine (csrc/m3rsm_engine.cpp, host C++ without HIP) replayed against the matches the compiled
reference made AWAY FROM THE WORLD ORIGIN -- tests/golden/placed_pyramid.npz (make_golden_placed_pyramid.py): occ_square at
N1, occ_1beam at N2, tbm_square at N3, and one many-to-many run whose four requests stand at the origin, N1, N2 and N3 --
through the native programs that replay m3rsm.npz and m3rsm_many.npz (tests/native/m3rsm_engine_test.cpp,
m3rsm_many_engine_test.cpp), plainly and under -fsanitize=address,undefined; and what the fixture holds."""
import os
import shutil
import subprocess

import numpy as np
import pytest
from m3rsm_cases import children
from placed_scenes import N_STATIONS, N_TABLE
from pyramid_cases import LONE_STATIONS, placed_lone_scene, placed_many_scene, placed_raw_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "slam-constructor_amd", "csrc")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")


def lone_file(path, scenes):
    flat = [float(len(scenes))]
    for s in scenes:
        flat += [*s.limits, *s.delta, s.prob, float(len(s.trace)), *s.trace.ravel()]
    np.asarray(flat, dtype=np.float64).tofile(path)
    return path


def many_file(path, scenes):
    flat = [float(len(scenes))]
    for s in scenes:
        flat += [*s.limits, float(len(s.requests)), float(s.winner), *s.delta, s.prob, float(len(s.trace)), *s.trace.ravel()]
    np.asarray(flat, dtype=np.float64).tofile(path)
    return path


def build(tmp_path, name, extra):
    exe = str(tmp_path / name)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", *extra, "-I" + CSRC, os.path.join(ROOT, "tests", "native", name + ".cpp"),
           os.path.join(CSRC, "m3rsm_engine.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300)
    return exe


@needs_gxx
@pytest.mark.parametrize("extra", [[], SANITIZE], ids=["plain", "sanitized"])
def test_engine_replays_the_references_far_matches(tmp_path, extra):
    scenes = [placed_lone_scene(st) for st in N_STATIONS] + [placed_raw_scene()]  # (the engine never sees the provider)
    lone = lone_file(str(tmp_path / "lone.bin"), scenes)
    r = subprocess.run([build(tmp_path, "m3rsm_engine_test", extra), lone], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok %d scenes" % len(scenes)), r.stdout + r.stderr
    many = many_file(str(tmp_path / "many.bin"), [placed_many_scene()])
    r = subprocess.run([build(tmp_path, "m3rsm_many_engine_test", extra), many, lone], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok 1 + %d scenes" % len(scenes)), r.stdout + r.stderr


def test_the_far_fixture_holds_the_cases():
    for st in N_STATIONS:
        s = placed_lone_scene(st)
        (kx, ky), _ = N_TABLE[st]
        assert s.name == LONE_STATIONS[st]
        assert (s.width // 2 - s.origin[0], s.height // 2 - s.origin[1]) == (kx, ky) or (11 - s.origin[0], 20 - s.origin[1]) == (kx, ky)
        assert not (0 <= s.origin[0] < s.width) and not (0 <= s.origin[1] < s.height)
        assert abs(s.pose[0] - kx * s.scale) < 2.0 and abs(s.pose[1] - ky * s.scale) < 2.0  # the match starts AT the station
        assert 40 <= len(s.trace) <= 4500 and np.all(np.isfinite(s.trace))
        seen, n_roots = set(), 2 * len(set(s.trace[:, 0].tolist()))
        for j, row in enumerate(s.trace):  # every call a root or a child, by the rule, of an earlier call at the same rotation
            assert j < n_roots or row[:5].tobytes() in seen, "%s: call %d has no parent on record" % (s.name, j)
            for kid in children(row[1:5], s.limits[4]):
                seen.add(np.asarray([row[0], *kid]).tobytes())
        pts = s.trace[(s.trace[:, 1] == s.trace[:, 2]) & (s.trace[:, 3] == s.trace[:, 4])]
        assert ((pts[:, 3] == s.delta[0]) & (pts[:, 1] == s.delta[1]) & (pts[:, 0] == s.delta[2]) & (pts[:, 5] == s.prob)).any()
    assert len(placed_lone_scene("N2").scan) == 1 and placed_lone_scene("N3").cell_model == 1
    e = placed_raw_scene()  # the edge scene: 0.125 m cells, the pose on a cell centre 16 + N1 cells out, an exact double
    assert e.name == "edge_occ" and e.scale == 0.125 and (16 - e.origin[0], 16 - e.origin[1]) == N_TABLE["N1"][0]
    assert np.all(np.round(e.pose[:2] * 16) == e.pose[:2] * 16) and np.all(np.round(e.pose[:2] * 16) % 2 == 1)
    assert 40 <= len(e.trace) <= 4500 and e.libm_variant in (0, 1)
    m = placed_many_scene()
    assert len(m.maps) == len(m.requests) == 4 and [r.map for r in m.requests] == [0, 1, 2, 3]
    far = [(mp.width // 2 - mp.origin[0], mp.height // 2 - mp.origin[1]) for mp in m.maps]
    assert far[0] == (0, 0) and far[1] == N_TABLE["N1"][0] and far[3] == N_TABLE["N3"][0]
    assert (11 - m.maps[2].origin[0], 20 - m.maps[2].origin[1]) == N_TABLE["N2"][0]
    assert m.winner == int(np.argmax(m.lone[:, 3])) != 0 and len(set(m.trace[:, 0].tolist())) == 4
    assert len(m.trace) < m.lone[:, 4].sum()  # the shared cut saves calls
