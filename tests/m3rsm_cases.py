"""Shared by tests/test_m3rsm_host.py and tests/test_gpu_m3rsm.py: the goldens of tests/golden/m3rsm.npz
(make_golden_m3rsm.py: whole matches of the compiled reference's BruteForceMultiResolutionScanMatcher with their traces)
as objects, and the refinement rule of include/slamhip.h "EXPAND" restated in numpy doubles."""
import os
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "m3rsm.npz"))
N_SCENES = int(G["n_scenes"])
EPS = 2.220446049250313e-16
SLOTS = {1: 5, 2: 30, 3: 155}


def golden_scene(i):
    pre = "s%d_" % i
    s = types.SimpleNamespace(name=str(G[pre + "name"]), cls=str(G[pre + "cls"]), cell_model=int(G[pre + "model"]),
                              oie=int(G[pre + "oie"]), scale=float(G[pre + "scale"]), origin=tuple(int(v) for v in G[pre + "origin"]),
                              unknown=G[pre + "unknown"], payload=G[pre + "payload"], pose=G[pre + "pose"], scan=G[pre + "scan"],
                              limits=G[pre + "limits"], delta=G[pre + "delta"], prob=float(G[pre + "prob"]), trace=G[pre + "trace"])
    s.height, s.width = s.payload.shape[:2]
    return s


SCENE_NAMES = [str(G["s%d_name" % i]) for i in range(N_SCENES)]


def children(rect, step):
    """the children of (bot, top, left, right) under the translation step, in the reference's order"""
    bot, top, left, right = (np.float64(v) for v in rect)
    step = np.float64(step)
    hside, vside = right - left, top - bot
    if not (vside >= 0 and hside >= 0 and np.isfinite(vside) and np.isfinite(hside)):
        return []
    hb, vb = step < hside + EPS, step < vside + EPS
    cx, cy = left + hside / 2, bot + vside / 2
    if hb and vb:
        return [(bot, cy, left, cx), (cy, top, left, cx), (bot, cy, cx, right), (cy, top, cx, right)]
    if hb:
        return [(bot, top, left, cx), (bot, top, cx, right)]
    if vb:
        return [(bot, cy, left, right), (cy, top, left, right)]
    if hside + vside <= 0:
        return []
    return [(bot, bot, left, left), (top, top, left, left), (bot, bot, right, right), (top, top, right, right), (cy, cy, cx, cx)]


def host_slots(rect, step, depth):
    """the slot layout of slamhip_pyramid_expand_matches for one parent: [S, 4], NaN where a slot has no node"""
    out = np.full((SLOTS[depth], 4), np.nan)
    gen, base = [(tuple(rect), True)], 0
    for _ in range(depth):
        nxt = []
        for node, there in gen:
            kids = children(node, step) if there else []
            nxt += [(kids[c], True) if c < len(kids) else (None, False) for c in range(5)]
        for j, (node, there) in enumerate(nxt):
            if there:
                out[base + j] = node
        base += len(nxt)
        gen = nxt
    return out
