"""Shared by tests/test_oracle_placed.py (CPU) and tests/test_gpu_placed.py (GPU): the golden recorded far from the world
origin (tests/golden/placed.npz, make_golden_placed.py), the oracle-only scenes at every station of placed_scenes.py, and
the reference-side probe that says how far a score may move when a pose coordinate is off by one ulp.

The oracle is the expected value wherever there is no golden (the F stations, every default-mode comparison), so the CPU
suite pins it to the golden at the Q stations first -- and asserts there what the GPU suite's exclusions rely on."""
import numpy as np
import placed_scenes as ps
from helpers import load
from pyoracle import (CELL_GMAPPING, CELL_OCC, CELL_TBM, OOPE_GMAPPING, OOPE_MAX, OOPE_MEAN, OOPE_OBSTACLE, OOPE_OVERLAP,
                      TRIG_CACHED, TRIG_RAW, GridMapData, Oracle, ScanData, make_cfg)
from pyoracle_mapupdate import AUX_STRIDE, RULE_GMAPPING, RULE_MEAN, RULE_TBM, append_scan_ex

CLASSES = {"mean": (CELL_OCC, RULE_MEAN), "tbm": (CELL_TBM, RULE_TBM), "gmapping": (CELL_GMAPPING, RULE_GMAPPING)}
STRIDE = {CELL_OCC: 1, CELL_TBM: 4, CELL_GMAPPING: 3}
UPDATE_RUNS = [(name, est) for name in CLASSES for est in (0, 1)]
UPDATE_IDS = ["%s-%s" % (name, "area" if est else "const") for name, est in UPDATE_RUNS]
WIN_OOPES = (("max", OOPE_MAX), ("mean", OOPE_MEAN), ("overlap", OOPE_OVERLAP))
PIECEWISE_CONSTANT = (OOPE_OBSTACLE, OOPE_MAX, OOPE_MEAN)  # the score is a step function of the pose
NEAR_RTOL = {OOPE_OBSTACLE: 1e-12, OOPE_MAX: 1e-12, OOPE_MEAN: 1e-12, OOPE_OVERLAP: 1e-12, OOPE_GMAPPING: 1e-11}
MAX_LEFT_OUT = 0.02  # of a case's poses

_golden = None


def golden():
    global _golden
    if _golden is None:
        _golden = load("placed.npz")
    return _golden


def tag(st, name, est, k):
    return "%s_%s%s_step%d_" % (st, name, "_area" if est else "", k)


def has_snapshot(g, st, name, est, k):
    return tag(st, name, est, k) + "payload" in g


def window_geometry(g, st):
    w, h = [int(v) for v in g["window"]]
    return w, h, tuple(int(v) for v in g[st + "_origin"])


def fresh_map(g, st, name):
    """(map, counters, rule): the never-observed window at the station, as the oracle's and the device's starting point"""
    cell_model, rule = CLASSES[name]
    w, h, origin = window_geometry(g, st)
    unk = g["%s_%s_unknown" % (st, name)]
    stn = STRIDE[cell_model]
    m = GridMapData(cell_model, np.tile(unk[:stn], (h, w, 1)).astype(np.float64), origin, float(g["scale"]), unk[:stn])
    aux = np.zeros((h, w, AUX_STRIDE[rule])) if rule in AUX_STRIDE else None
    return m, aux, rule


def final_map(g, st, name):
    """the reference's map after the three appends (const estimator): what the golden's scores were taken on"""
    cell_model, _ = CLASSES[name]
    w, h, origin = window_geometry(g, st)
    unk = g["%s_%s_unknown" % (st, name)]
    return GridMapData(cell_model, g[tag(st, name, 0, 2) + "payload"], origin, float(g["scale"]), unk[:STRIDE[cell_model]])


def adder_args(g, name, est):
    kw = dict(quality=float(g["quality"]), base=g[name + "_base"], blur=float(g[name + "_blur"]))
    return kw, (dict(est_kind=1, shift_amount=float(g["shift_amount"])) if est else {})


def oracle_append(oracle, g, st, name, est, k, m, aux, rule, trig=None):
    """append k of the golden's history on the oracle (raw provider, as in the reference run, unless trig is given)"""
    kw, ex = adder_args(g, name, est)
    return append_scan_ex(oracle, m, aux, rule, g[st + "_append_poses"][k], g[st + "_raw_range"], g[st + "_raw_angle"],
                          g[st + "_raw_occ"], trig=trig, **kw, **ex)


def golden_scan(g, st, trig, weighting="even"):
    """the filtered scan the golden's scores were taken with, behind the raw (0) or the cached (1) provider"""
    kept = g[st + "_kept"]
    r, a = g[st + "_raw_range"][kept], g[st + "_raw_angle"][kept]
    w = g[st + "_viny_weight"] if weighting == "viny" else np.full(r.size, 1.0 / r.size)
    if trig == TRIG_CACHED:
        return ScanData(r, a, w, None, TRIG_CACHED, float(g[st + "_a_min"]), float(g[st + "_a_inc"]), g[st + "_tab_sin"],
                        g[st + "_tab_cos"])
    return ScanData(r, a, w, None, TRIG_RAW)


def raw_trig(g, st, trig):
    """the provider alone, for oracle.filter_scan of the raw scan"""
    r, a = g[st + "_raw_range"], g[st + "_raw_angle"]
    if trig == TRIG_CACHED:
        return ScanData(r, a, None, None, TRIG_CACHED, float(g[st + "_a_min"]), float(g[st + "_a_inc"]), g[st + "_tab_sin"],
                        g[st + "_tab_cos"])
    return ScanData(r, a)


def trace(g, prefix):
    from helpers import trace as _t
    return _t(g, prefix)


# ---- the oracle-only scenes: every station, the rasters the chain tests use ---------------------------------------------------
_scenes = {}


def scene(station, cell_model=CELL_OCC, scale=0.1, n_beams=360, weighting="even", raw=False):
    """placed_scenes.place at the sizes of the issue: raster 240 at 0.1 m, 400 at 0.05 m; made once, handed out unchanged"""
    key = (station, cell_model, scale, n_beams, weighting, raw)
    if key not in _scenes:
        size = {0.1: 240, 0.05: 400}[scale]
        _scenes[key] = ps.place(station, cell_model, size=size, scale=scale, n_beams=n_beams, weighting=weighting, raw=raw)
    return _scenes[key]


WIN_AREA_SYNTH = (-0.06, 0.06, -0.04, 0.04)  # the analysis area of the chain tests' window-OOPE cases
SYNTH_KINDS = {"occ": dict(cell_model=CELL_OCC, scale=0.1, n_beams=360, weighting="even"),
               "tbm": dict(cell_model=CELL_TBM, scale=0.05, n_beams=720, weighting="viny"),  # three 256-beam blocks
               "gm": dict(cell_model=CELL_GMAPPING, scale=0.05, n_beams=360, weighting="even")}


def synth_poses(sc, kind, n=64):
    sigma = (0.05, 0.05, 0.02) if kind == "gm" else (0.2, 0.2, 0.1)
    return ps.candidates(sc, n, 300 + ps.SEEDS[sc["station"]], sigma=sigma)


def scorer_cases(stations=None):
    """Every scorer case of the GPU suite as (id, station, map, scan, oope, area, poses): the golden's at the Q stations
    (reference-built maps, cached and raw provider) and the synthetic scenes at every station.  The CPU suite walks the
    same list to assert that the oracle alone leaves at most 2 % of a case's poses ill-conditioned."""
    g = golden()
    out = []
    for st in ps.Q_STATIONS:
        if stations is not None and st not in stations:
            continue
        for tname, trig in (("cached", TRIG_CACHED), ("raw", TRIG_RAW)):
            for name, weighting in (("mean", "even"), ("tbm", "viny")):
                m, scan = final_map(g, st, name), golden_scan(g, st, trig, weighting)
                out.append(("golden-%s-%s-%s" % (st, name, tname), st, m, scan, OOPE_OBSTACLE, (0, 0, 0, 0), g[st + "_poses"]))
                for kname, kind in WIN_OOPES:
                    out.append(("golden-%s-%s-%s-%s" % (st, name, tname, kname), st, m, scan, kind, tuple(g["win_area"]),
                                g[st + "_poses"][:24]))
            out.append(("golden-%s-gmapping-%s" % (st, tname), st, final_map(g, st, "gmapping"), golden_scan(g, st, trig),
                        OOPE_GMAPPING, (0, 0, 0, 0), g[st + "_gm_poses"]))
    for st in ps.ALL:
        if stations is not None and st not in stations:
            continue
        for kind, kw in SYNTH_KINDS.items():
            sc = scene(st, **kw)
            poses = synth_poses(sc, kind)
            if kind == "gm":
                out.append(("synth-%s-gm" % st, st, sc["map"], sc["scan"], OOPE_GMAPPING, (0, 0, 0, 0), poses))
                continue
            out.append(("synth-%s-%s" % (st, kind), st, sc["map"], sc["scan"], OOPE_OBSTACLE, (0, 0, 0, 0), poses))
            for kname, k in WIN_OOPES:
                out.append(("synth-%s-%s-%s" % (st, kind, kname), st, sc["map"], sc["scan"], k, WIN_AREA_SYNTH, poses[:24]))
    return out


# ---- the reference-side probe -----------------------------------------------------------------------------------------------
def probe(oracle, m, scan, cfg, poses):
    """Scores of `poses` and of their eight neighbours one ulp away in x and / or y, all by the ORACLE: [9, P].  The
    GMapping OOPE gets a fresh cache per row (one estimator across the poses, as everywhere)."""
    rows = []
    for q in ps.ulp_neighbours(poses):
        cache = Oracle.new_gm_cache() if cfg.oope == OOPE_GMAPPING else None
        rows.append(oracle.score_poses(m, scan, cfg, q, cache))
    return np.stack(rows)


def ill_conditioned(rows):
    """poses of a piecewise-constant scorer whose score changes under the probe: an end point sits within an ulp of the
    pose off a cell edge"""
    return (rows != rows[0]).any(axis=0)


def allowance(rows, oope):
    """Relative tolerance of a non-exact mode far out: 4 x the largest relative change the probe shows over the case's
    poses + the near-origin tolerance.  4: one pose rounding and one sincos rounding each move an end point by at most one
    ulp of the coordinate per axis, the probe moves it by one."""
    rel = np.max(np.abs(rows - rows[0]) / np.abs(rows[0]))
    return 4.0 * float(rel) + NEAR_RTOL[oope], float(rel)


def compare_non_exact(got, rows, oope, station, what="", near_rtol=None):
    """A non-exact mode's scores `got` against the oracle's rows[0] under the rules of the issue.  Returns (rtol used,
    share of poses left out).  Station O keeps the near-origin contract (near_rtol: where the suite states another one
    for the form at hand, such as 1e-10 for default-mode GMapping traces)."""
    want = rows[0]
    keep = np.ones(want.size, bool)
    near = NEAR_RTOL[oope] if near_rtol is None else near_rtol
    rtol = near
    if station != "O":
        if oope in PIECEWISE_CONSTANT:
            keep = ~ill_conditioned(rows)
            assert (~keep).mean() <= MAX_LEFT_OUT, "%s: %d of %d poses ill-conditioned" % (what, (~keep).sum(), keep.size)
        else:
            rtol = allowance(rows, oope)[0] - NEAR_RTOL[oope] + near
    np.testing.assert_allclose(got[keep], want[keep], rtol=rtol, atol=0 if oope != OOPE_GMAPPING else 1e-300,
                               err_msg="%s at %s" % (what, station))
    return rtol, float((~keep).mean())


def oracle_tail(t):
    """calls at the end of an ORACLE trace whose pose equals the best pose bit for bit: what a closed-form tail may skip"""
    acc = np.nonzero(t["accepted"])[0]
    best = t["poses"][acc[-1]]
    n = 0
    while n < t["n_calls"] and np.array_equal(t["poses"][-1 - n], best):
        n += 1
    return n
