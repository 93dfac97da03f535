"""Shared by tests/test_oracle_mapupdate_oblong.py (CPU) and tests/test_gpu_mapupdate_oblong.py (GPU): the map-update
golden on a window that is no square (tests/golden/map_update_oblong.npz, make_golden_mapupdate_oblong.py) and the
oracle runs both suites replay on it.  The oracle is the expected value for every GPU case that has no golden, so the
CPU suite pins it to the golden first -- on the full window and on the re-based crop box."""
import numpy as np
from helpers import load
from pyoracle import CELL_GMAPPING, CELL_OCC, CELL_TBM, GridMapData
from pyoracle_mapupdate import AUX_STRIDE, RULE_AFFINE, RULE_GMAPPING, RULE_LAST, RULE_MEAN, RULE_TBM, append_scan_ex

MODELS = {"mean": (CELL_OCC, RULE_MEAN), "affine": (CELL_OCC, RULE_AFFINE), "last": (CELL_OCC, RULE_LAST),
          "tbm": (CELL_TBM, RULE_TBM), "gmapping": (CELL_GMAPPING, RULE_GMAPPING)}
STRIDE = {CELL_OCC: 1, CELL_TBM: 4, CELL_GMAPPING: 3}
UNKNOWN = {CELL_OCC: [0.5], CELL_TBM: [1.0, 0.0, 0.0, 0.0], CELL_GMAPPING: [-1.0, 0.0, 0.0]}
# (cell rule, occupancy estimator): all five rules with the const estimator, three of them with the area estimator
RUNS = [(name, 0) for name in MODELS] + [(name, 1) for name in ("mean", "tbm", "gmapping")]
RUN_IDS = ["%s-%s" % (name, "area" if est else "const") for name, est in RUNS]

_golden = None


def golden():
    global _golden
    if _golden is None:
        _golden = load("map_update_oblong.npz")
    return _golden


def tag(name, est, k):
    return "%s%s_step%d_" % (name, "_area" if est else "", k)


def geometry(g, name, window="full"):
    """(width, height, (origin_x, origin_y)) of the golden's window.  full: the reference's own; crop: the crop box
    bound as a map of its own (the world origin lies outside it); transposed: width <-> height and origin_x <->
    origin_y; origin_swapped: origin_x <-> origin_y alone."""
    w, h = [int(v) for v in g[name + "_size"]]
    ox, oy = [int(v) for v in g[name + "_origin"]]
    x0, y0, x1, y1 = [int(v) for v in g["crop"]]
    return {"full": (w, h, (ox, oy)), "crop": (x1 - x0, y1 - y0, (ox - x0, oy - y0)),
            "transposed": (h, w, (oy, ox)), "origin_swapped": (w, h, (oy, ox))}[window]


def fresh_map(g, name, window="full"):
    cell_model, rule = MODELS[name]
    w, h, origin = geometry(g, name, window)
    st = STRIDE[cell_model]
    unk = g[name + "_unknown"]
    payload = np.tile(unk[:st], (h, w, 1)).astype(np.float64)
    m = GridMapData(cell_model, payload, origin, float(g["scale"]), unk[:st])
    aux = np.zeros((h, w, AUX_STRIDE[rule])) if rule in AUX_STRIDE else None
    return m, aux, rule


def step_args(g, name, est, k):
    """Keyword arguments of step k shared by the oracle's and the device's append_scan (pose, scan and adder)."""
    q, blur, max_range = g["step%d_params" % k]
    return dict(quality=float(q), base=g[name + "_base"], blur=float(blur), max_range=float(max_range)), \
        (dict(est_kind=1, shift_amount=float(g["shift_amount"])) if est else {})


def oracle_step(oracle, g, name, est, k, m, aux, rule):
    """Step k of the golden's history on the oracle, raw trigonometry provider as in the reference run."""
    kw, ex = step_args(g, name, est, k)
    return append_scan_ex(oracle, m, aux, rule, g["step%d_pose" % k], g["step%d_range" % k], g["step%d_angle" % k],
                          g["step%d_occ" % k], **kw, **ex)


def crop_of(g, a):
    x0, y0, x1, y1 = [int(v) for v in g["crop"]]
    return a[y0:y1, x0:x1]


def outside_crop(g, a):
    x0, y0, x1, y1 = [int(v) for v in g["crop"]]
    mask = np.ones(a.shape[:2], bool)
    mask[y0:y1, x0:x1] = False
    return a[mask]
