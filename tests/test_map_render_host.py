"""CPU suite: the map render's host side (include/slamhip.h "map render"; csrc/map_render.hip, slamhip_internal.h).

  * slamhip_render_cells -- the definition of a cell's occupancy and of the two byte rules that the render kernels
    share -- equals, byte for byte, what the compiled reference's two map consumers make of every golden cell of
    tests/golden/map_render.npz: GridMapToPgmDumber::dump_map's own pixels and the int8 of OccupancyGridPublisher's cell
    loop, for a map of each cell class and for the hand-made edge cells;
  * bad arguments are SLAMHIP_ERR_INVALID;
  * the reference-side adapter headers (host/slamhip_reference_adapter.h with HipResidentMapView::render,
    host/slamhip_map_observers.h) compile against the unmodified reference headers -- only where the reference tree is
    present."""
import os
import shutil
import subprocess

import numpy as np
import pytest
from helpers import load

import __graft_entry__ as ge

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = os.environ.get("REFERENCE", "/root/reference")
CLASSES = ("affine", "mean", "tbm_consistent", "tbm_unknown_even", "gmapping", "credibilist")


@pytest.fixture(scope="module")
def pkg():
    p = ge.load_package()
    if not os.path.exists(p.LIB_PATH):
        p.build()
    return p


@pytest.fixture(scope="module")
def golden():
    return load("map_render.npz")


@pytest.mark.parametrize("name", CLASSES)
def test_render_cells_equals_the_reference_on_every_golden_map_cell(pkg, golden, name):
    g = golden
    model, kind = int(g[name + "_model"]), int(g[name + "_occ_kind"])
    payload = g[name + "_payload"]
    assert payload.shape == (29, 37, pkg.STRIDE[model])
    occ = pkg.render_cells(model, payload, pkg.RENDER_OCCGRID, kind)
    assert occ.dtype == np.int8 and occ.shape == (29, 37)
    np.testing.assert_array_equal(occ, g[name + "_occgrid"])
    pgm = pkg.render_cells(model, payload, pkg.RENDER_PGM, kind)
    assert pgm.dtype == np.uint8
    np.testing.assert_array_equal(pgm[::-1], g[name + "_pgm"])  # the file's rows run top-down
    # the fixture is what the issue asks for: about a third of the cells never observed, and they read unknown
    value = g[name + "_value"]
    fresh = value == (-1.0 if name == "gmapping" else 0.5)
    assert 0.25 < fresh.mean() < 0.45
    assert np.all(pgm[fresh] == 127) and np.all(occ[fresh] == (-1 if name == "gmapping" else 50))
    assert len(np.unique(pgm)) > 100


@pytest.mark.parametrize("name", CLASSES)
def test_render_cells_equals_the_reference_on_every_golden_edge_cell(pkg, golden, name):
    g = golden
    model, kind = int(g[name + "_model"]), int(g[name + "_occ_kind"])
    payload = g[name + "_edge_payload"]
    assert payload.shape[0] > 800
    ok = g[name + "_edge_occgrid_ok"]
    occ = pkg.render_cells(model, payload, pkg.RENDER_OCCGRID, kind)
    np.testing.assert_array_equal(occ[ok], g[name + "_edge_occgrid"][ok])
    np.testing.assert_array_equal(pkg.render_cells(model, payload, pkg.RENDER_PGM, kind), g[name + "_edge_pgm"])
    # where the reference's conversion is undefined (its own value not finite): -1, as the header says
    value = g[name + "_edge_value"]
    assert np.all(occ[~np.isfinite(value)] == -1)
    if name == "affine":  # value * 100 truncates below k for some k / 100
        for v, want in ((0.29, 28), (0.57, 56), (0.0, 0), (1.0, 100), (-1.0, -1)):
            assert np.all(occ[value == v] == want) and np.any(value == v), v


def test_the_tbm_kinds_differ_and_the_never_updated_cell_reads_half(pkg):
    cells = np.array([[1.0, 0.0, 0.0, 0.0], [0.5, 0.25, 0.25, 0.0], [0.0, 0.0, 0.0, 0.0]])
    a = pkg.render_cells(pkg.CELL_TBM, cells, pkg.RENDER_OCCGRID, pkg.OCC_TBM_CONSISTENT)
    b = pkg.render_cells(pkg.CELL_TBM, cells, pkg.RENDER_OCCGRID, pkg.OCC_TBM_UNKNOWN_EVEN)
    c = pkg.render_cells(pkg.CELL_CREDIBILIST, cells, pkg.RENDER_OCCGRID)
    # o / (o + e): 0.5 for the vacuous payload (the prototype), 0.5, 0 / 0 -> -1;  o + 0.5 u: 50, 50, 0
    np.testing.assert_array_equal(a, np.array([50, 50, -1], np.int8))
    np.testing.assert_array_equal(b, np.array([50, 50, 0], np.int8))
    np.testing.assert_array_equal(c, b)
    np.testing.assert_array_equal(pkg.render_cells(pkg.CELL_TBM, cells, pkg.RENDER_PGM, 0), np.array([127, 127, 0], np.uint8))
    assert pkg.render_cells(pkg.CELL_OCC, np.zeros((0, 1)), pkg.RENDER_PGM).shape == (0,)


def test_render_cells_rejects_bad_arguments(pkg):
    one = np.array([[0.5]])
    four = np.array([[0.2, 0.3, 0.5, 0.0]])
    with pytest.raises(pkg.SlamHipError):
        pkg.render_cells(pkg.CELL_OCC, one, 2)          # unknown format
    with pytest.raises(pkg.SlamHipError):
        pkg.render_cells(pkg.CELL_OCC, one, -1)
    with pytest.raises(pkg.SlamHipError):
        pkg.render_cells(7, one, pkg.RENDER_PGM)        # unknown cell model
    for model, p in ((pkg.CELL_OCC, one), (pkg.CELL_GMAPPING, np.zeros((1, 3))), (pkg.CELL_CREDIBILIST, four)):
        with pytest.raises(pkg.SlamHipError):
            pkg.render_cells(model, p, pkg.RENDER_PGM, occ_kind=1)  # occ_kind names a TBM cell class
    with pytest.raises(pkg.SlamHipError):
        pkg.render_cells(pkg.CELL_TBM, four, pkg.RENDER_PGM, occ_kind=2)
    L = pkg.load()
    out = np.zeros(1, np.uint8)
    assert L.slamhip_render_cells(0, 0, 0, 1, None, out.ctypes.data) == -1   # null payload
    assert L.slamhip_render_cells(0, 0, 0, 1, one.ctypes.data_as(pkg._dp), None) == -1  # null out
    assert L.slamhip_render_cells(0, 0, 0, -1, one.ctypes.data_as(pkg._dp), out.ctypes.data) == -1
    assert L.slamhip_render_cells(0, 0, 0, 0, None, None) == 0  # nothing to do


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
@pytest.mark.parametrize("header", ["slamhip_reference_adapter.h", "slamhip_map_observers.h"])
def test_map_render_adapter_headers_compile_against_the_reference(tmp_path, header):
    if not os.path.isfile(os.path.join(REFERENCE, "src", "utils", "map_dumpers.h")):
        pytest.skip("reference tree not present")
    tu = tmp_path / "tu.cpp"
    body = '#include "%s"\n' % header
    if header == "slamhip_map_observers.h":  # ... and its templates and inline functions are instantiated
        body += ("void use(const GridMap &m, HipResidentMapView &v) {\n  std::vector<int8_t> d; int w, h, ox, oy;\n"
                 "  hip_occupancy_grid(m, d, w, h, ox, oy);\n  HipGridMapToPgmDumper dumper(\"map\");\n  dumper.on_map_update(v);\n"
                 "  std::vector<unsigned char> px; v.render(SLAMHIP_RENDER_PGM, px);\n}\n")
    tu.write_text(body)
    cmd = ["g++", "-std=c++14", "-fsyntax-only", "-w", "-I" + os.path.join(REFERENCE, "src"), "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "slam-constructor_amd", "host"), str(tu)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
