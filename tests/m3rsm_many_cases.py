"""Shared by tests/test_m3rsm_many_host.py and tests/test_gpu_m3rsm_many.py: the goldens of tests/golden/m3rsm_many.npz
(make_golden_m3rsm_many.py: the compiled reference's M3RSMEngine given several scan matching requests, with the trace of
its scorer calls over all of them and every request's lone match) as objects."""
import os
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "m3rsm_many.npz"))
N_SCENES = int(G["n_scenes"])


def golden_scene(i):
    pre = "s%d_" % i
    s = types.SimpleNamespace(name=str(G[pre + "name"]), cls=str(G[pre + "cls"]), cell_model=int(G[pre + "model"]),
                              oie=int(G[pre + "oie"]), limits=G[pre + "limits"], winner=int(G[pre + "winner"]),
                              delta=G[pre + "delta"], prob=float(G[pre + "prob"]), trace=G[pre + "trace"], lone=G[pre + "lone"])
    s.maps = []
    for j in range(int(G[pre + "n_maps"])):
        m = types.SimpleNamespace(cell_model=s.cell_model, scale=float(G[pre + "m%d_scale" % j]),
                                  origin=tuple(int(v) for v in G[pre + "m%d_origin" % j]), unknown=G[pre + "m%d_unknown" % j],
                                  payload=G[pre + "m%d_payload" % j])
        m.height, m.width = m.payload.shape[:2]
        s.maps.append(m)
    s.requests = [types.SimpleNamespace(map=int(G[pre + "r%d_map" % j]), pose=G[pre + "r%d_pose" % j], scan=G[pre + "r%d_scan" % j])
                  for j in range(int(G[pre + "n_requests"]))]
    return s


SCENE_NAMES = [str(G["s%d_name" % i]) for i in range(N_SCENES)]
