"""CPU suite: the peaks rule of a brute-force sweep's score landscape (csrc/bf_peaks.h, plain C++ without HIP).
tests/native/bf_peaks_test.cpp -- the separable form against the triple-loop form on volumes full of ties, plateaus and
NaN, floors at exact equality, the bound B -- is built and run as a stand-alone native program, plainly and under
-fsanitize=address,undefined; slamhip_bf_peaks_host, the public host entry, is compared through ctypes against a window
loop written in numpy here, and its refusals are checked."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "slam-constructor_amd", "csrc")
NATIVE = os.path.join(ROOT, "tests", "native")
ASAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]

needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")


@pytest.fixture(scope="module")
def pkg():
    p = ge.load_package()
    if not os.path.exists(p.LIB_PATH):
        p.build()
    return p


@needs_gxx
@pytest.mark.parametrize("extra", [[], ASAN], ids=["plain", "asan_ubsan"])
def test_separable_form_against_the_definition(tmp_path, extra):
    exe = str(tmp_path / "bf_peaks_test")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *extra, "-I" + CSRC,
                        os.path.join(NATIVE, "bf_peaks_test.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert r.stdout.splitlines()[-1] == "ok bf peaks", r.stdout


def test_the_header_is_free_of_hip():
    text = open(os.path.join(CSRC, "bf_peaks.h")).read()
    assert "#include <hip" not in text and "slamhip_internal.h" not in text


def numpy_peaks(scores, shape, radius, min_ratio, min_score):
    """The rule as it reads: (index, score) of every kept peak, best first."""
    nx, ny, nt = shape
    v = np.asarray(scores, dtype=np.float64).reshape(nt, ny, nx)
    if np.all(np.isnan(v)):
        return np.zeros(0, np.int64), np.zeros(0)
    s_max = np.nanmax(v)
    idx = np.arange(v.size).reshape(v.shape)
    out = []
    for it in range(nt):
        for iy in range(ny):
            for ix in range(nx):
                s = v[it, iy, ix]
                if np.isnan(s):
                    continue
                sl = (slice(max(0, it - radius[2]), it + radius[2] + 1), slice(max(0, iy - radius[1]), iy + radius[1] + 1),
                      slice(max(0, ix - radius[0]), ix + radius[0] + 1))
                w, wi = v[sl], idx[sl]
                with np.errstate(invalid="ignore"):
                    beaten = np.any((w > s) | ((w == s) & (wi < idx[it, iy, ix])))
                if not beaten and s >= min_score and s >= min_ratio * s_max:
                    out.append((idx[it, iy, ix], s))
    out.sort(key=lambda e: (-e[1], e[0]))
    return np.array([e[0] for e in out], np.int64), np.array([e[1] for e in out], np.float64)


CASES = [((1, 1, 1), (0, 0, 0)), ((9, 7, 1), (1, 1, 1)), ((9, 7, 1), (3, 2, 1)), ((17, 5, 9), (1, 1, 1)),
         ((17, 5, 9), (3, 2, 1)), ((17, 5, 9), (32, 32, 32)), ((40, 33, 2), (0, 0, 0)), ((3, 200, 2), (1, 1, 1))]


@pytest.mark.parametrize("shape,radius", CASES)
def test_host_entry_against_a_numpy_window_loop(pkg, shape, radius):
    rs = np.random.RandomState(shape[0] * 131 + shape[1] * 7 + radius[0])
    n = shape[0] * shape[1] * shape[2]
    v = rs.choice([0.25, 0.5, 1.0, 2.0, np.nan], size=n)
    for min_ratio, min_score in [(0.0, -np.inf), (0.5, 0.0), (0.0, 1.0), (1.0, 0.0)]:
        want_i, want_s = numpy_peaks(v, shape, radius, min_ratio, min_score)
        for max_peaks in (0, 1, len(want_i) + 2):
            got = pkg.bf_peaks_host(v, shape, radius, min_ratio, min_score, max_peaks)
            assert got["n_found"] == len(want_i)
            k = min(max_peaks, len(want_i))
            np.testing.assert_array_equal(got["index"], want_i[:k])
            np.testing.assert_array_equal(got["scores"].view(np.uint64), want_s[:k].view(np.uint64))


def test_host_entry_all_nan_and_refusals(pkg):
    v = np.full(9 * 7 * 2, np.nan)
    got = pkg.bf_peaks_host(v, (9, 7, 2), (1, 1, 1), 0.0, -np.inf, 8)
    assert got["n_found"] == 0 and got["index"].size == 0
    ok = np.ones(9 * 7 * 2)
    bad = [dict(radius=(-1, 0, 0)), dict(radius=(0, 33, 0)), dict(max_peaks=-1), dict(max_peaks=8193), dict(min_ratio=-0.1),
           dict(min_ratio=1.5), dict(min_ratio=np.nan), dict(min_score=np.nan)]
    for kw in bad:
        with pytest.raises(pkg.SlamHipError, match="slamhip error -1:"):  # (SLAMHIP_ERR_INVALID)
            pkg.bf_peaks_host(ok, (9, 7, 2), **kw)
    # B = 100 x 100 x 1 > 8192 under radius 0: refused; radius 1 brings it to 2500
    big = np.ones(100 * 100)
    with pytest.raises(pkg.SlamHipError, match="8192"):
        pkg.bf_peaks_host(big, (100, 100, 1), (0, 0, 0))
    assert pkg.bf_peaks_host(big, (100, 100, 1), (1, 1, 0), max_peaks=4)["n_found"] == 1  # (a plateau: its first point only)


def test_host_entry_null_arguments(pkg):
    """Through the C-ABI itself (the wrapper always passes buffers): null scores, radius, n_written, n_found, and null
    outputs with max_peaks > 0 are SLAMHIP_ERR_INVALID; null outputs with max_peaks = 0 count only."""
    import ctypes as C
    L = pkg.load()
    v = np.array([0.5, 1.0, 0.5, 1.0, 0.25])
    rad = (C.c_int * 3)(1, 0, 0)
    idx, out, nw, nf = (C.c_longlong * 4)(), (C.c_double * 4)(), C.c_int(-7), C.c_longlong(-7)
    args = dict(scores=v.ctypes.data_as(C.POINTER(C.c_double)), radius=rad, index_out=idx, score_out=out, n_written=C.byref(nw),
                n_found=C.byref(nf))

    def call(max_peaks=4, shape=(5, 1, 1), **kw):
        a = dict(args, **kw)
        return L.slamhip_bf_peaks_host(a["scores"], *shape, a["radius"], 0.0, 0.0, max_peaks, a["index_out"], a["score_out"],
                                       a["n_written"], a["n_found"])

    for name in args:
        assert call(**{name: None}) == -1, name
    for shape in ((0, 1, 1), (5, 0, 1), (5, 1, -1)):
        assert call(shape=shape) == -1, shape
    assert nw.value == -7 and nf.value == -7  # (a refusal writes nothing)
    assert call(max_peaks=0, index_out=None, score_out=None) == 0 and (nw.value, nf.value) == (0, 2)
    assert call() == 0 and (nw.value, nf.value) == (2, 2) and list(idx)[:2] == [1, 3]
