"""Shared by tests/test_m3rsm_rawtrig_golden.py and tests/test_gpu_m3rsm_rawtrig.py: the goldens of
tests/golden/m3rsm_rawtrig.npz (make_golden_m3rsm_rawtrig.py: whole matches of the compiled reference's
BruteForceMultiResolutionScanMatcher with the scan under RawTrigonometryProvider, and the same matches under the cached
provider) as objects."""
import os
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "m3rsm_rawtrig.npz"))
N_SCENES = int(G["n_scenes"])
LIBM_VARIANT = int(G["libm_variant"])
SCENE_NAMES = [str(G["s%d_name" % i]) for i in range(N_SCENES)]
EDGE_NAMES = [str(G["s%d_name" % i]) for i in range(N_SCENES) if int(G["s%d_edge" % i])]
PER_SCENE = ("name", "cls", "model", "oie", "scale", "origin", "unknown", "payload", "pose", "scan", "angle", "trig", "edge",
             "limits", "delta", "prob", "trace", "delta_cached", "prob_cached", "trace_cached")


def golden_scene(i):
    if isinstance(i, str):
        i = SCENE_NAMES.index(i)
    pre = "s%d_" % i
    s = types.SimpleNamespace(name=str(G[pre + "name"]), cls=str(G[pre + "cls"]), cell_model=int(G[pre + "model"]),
                              oie=int(G[pre + "oie"]), scale=float(G[pre + "scale"]), origin=tuple(int(v) for v in G[pre + "origin"]),
                              unknown=G[pre + "unknown"], payload=G[pre + "payload"], pose=G[pre + "pose"], scan=G[pre + "scan"],
                              angle=G[pre + "angle"], trig=G[pre + "trig"], edge=bool(int(G[pre + "edge"])), limits=G[pre + "limits"],
                              delta=G[pre + "delta"], prob=float(G[pre + "prob"]), trace=G[pre + "trace"],
                              delta_cached=G[pre + "delta_cached"], prob_cached=float(G[pre + "prob_cached"]),
                              trace_cached=G[pre + "trace_cached"])
    s.height, s.width = s.payload.shape[:2]
    return s


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def n_bitwise_different(trace, other):
    """calls of the common prefix of equal (rotation, rectangle) whose scores differ bitwise"""
    n = min(len(trace), len(other))
    same = np.all(bits(trace[:n, :5]) == bits(other[:n, :5]), axis=1)
    k = n if same.all() else int(np.argmin(same))
    return int(np.sum(bits(trace[:k, 5]) != bits(other[:k, 5])))
