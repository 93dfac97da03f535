#!/usr/bin/env python3
"""Generate tests/golden/placed_pyramid.npz from the COMPILED REFERENCE: the levels of M3RSMRescalableGridMap
<UnboundedPlainGridMap> and Match::prob_upper_bound of its engine's matches AWAY FROM THE WORLD ORIGIN, at the three N
stations of tests/placed_scenes.py (500 ... 1500 cells out, odd shifts, sign patterns (-, +), (+, -), (-, -)).

    python tests/golden/make_golden_placed_pyramid.py [path/to/reference]

make_golden_pyramid.py's maps, harness (tests/golden/pyramid_harness.cpp, unchanged) and assertions, every one of them --
validate(), no updated cell equal to the prototype, the integer block rule and the tightness of every level, the
separation of impacts, every branch a child of an earlier call and no more than 1e-5 above it -- run per station over
the shapes 37 x 29 with origin (11, 20) and 33 x 33, scales 0.05 / 0.1 / 1.0, GridCell under both OIEs, TBM and Credibilist:
24 maps per station, and 24 match sets (67 beams, 1 beam; 22 roots plus 148 descendants each) on the 37 x 29 maps -- the
33 x 33 maps carry none, which keeps the fixture below the size of placed.npz.  The fine map's origin, the observations'
cells and the poses are moved by the station's shift; the draws are made as make_golden_pyramid.py makes them.

Whole matches, by the unchanged harnesses and with every assertion of make_golden_m3rsm.py, make_golden_m3rsm_many.py and
make_golden_m3rsm_rawtrig.py (validate(), tight levels, every recorded rectangle a child of an earlier call, the
non-prerotated rerun, the rerun with scores times 1 +- 1e-12), the scenes moved by the station's shift:
  lone_<station>_...   occ_square at N1, occ_1beam at N2, tbm_square at N3: what m3rsm.npz holds per scene, trace included
  many_...             ONE many-to-many run whose four requests stand at DIFFERENT stations -- the origin, N1, N2 (37 x 29 at
                       0.05), N3 --, each on its own map: what m3rsm_many.npz holds per scene; its `lone` rows (delta, prob,
                       calls of every request's lone match) are what K independent matches in one call must return
  raw_...              edge_occ under the reference's default (raw) trig provider at N1: what m3rsm_rawtrig.npz holds per
                       scene without the cached provider's trace; raw_n_differ = 0 is recorded behaviour (see below)

The reference's levels above the fine map are DENSE maps that grow from (0, 0) out to the data, so a level's own window
spans back to the origin; what is kept of it is the box of the cells it ever wrote (crop_level) -- the comparison of
pyramid_cases.assert_same_level reads everything outside a window as the prototype.

Keys: <station>_ in front of the members pack() makes of make_golden_pyramid.py's (m<i>_..., s<j>_..., n_maps, n_sets);
stations.

Measured where this fixture was made (all of it, the harnesses as child processes): 65 s wall clock, 0.59 GB peak
resident set of a harness, a fixture of 605 KiB.  No station had to be moved inward."""
import os
import resource
import sys
import time

import numpy as np

GOLDEN_DIR = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(GOLDEN_DIR))
sys.path.insert(0, GOLDEN_DIR)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import make_golden_m3rsm as m3  # noqa: E402
import make_golden_m3rsm_many as mm  # noqa: E402
import make_golden_m3rsm_rawtrig as rt  # noqa: E402
import make_golden_pyramid as mg  # noqa: E402
import placed_scenes as ps  # noqa: E402
from make_golden_placed import save_stable  # noqa: E402

SHAPES = [(37, 29, (11, 20)), (33, 33, None)]
LONE = [("N1", "occ_square"), ("N2", "occ_1beam"), ("N3", "tbm_square")]  # whole matches: one scene of m3rsm.npz per station


def pack(got, n_maps, n_sets):
    """make_golden_pyramid.py's arrays in fewer members (a zip member costs a few hundred bytes, a 1 x 1 level eight): per
    map m<i>_meta (model, oie, scale, origin x, y, levels), _unknown, _payload, _Lgeo [n, 4] (width, height, origin x, y
    of every level's kept box), _Lscale [n], _Lflat (the boxes' payloads one after the other); per set s<j>_meta (map,
    roots, pose[3], limits[5]), _scan, _cand"""
    out = {"n_maps": got["n_maps"], "n_sets": got["n_sets"]}
    for i in range(n_maps):
        pre = "m%d_" % i
        n = int(got[pre + "n_levels"])
        pays = [got[pre + "L%d_payload" % k] for k in range(1, n + 1)]
        out[pre + "meta"] = np.array([got[pre + "model"], got[pre + "oie"], got[pre + "scale"], *got[pre + "origin"], n], dtype=np.float64)
        out[pre + "unknown"], out[pre + "payload"] = got[pre + "unknown"], got[pre + "payload"]
        out[pre + "Lgeo"] = np.array([[p.shape[1], p.shape[0], *got[pre + "L%d_origin" % k]] for k, p in enumerate(pays, 1)])
        out[pre + "Lscale"] = np.array([got[pre + "L%d_scale" % k] for k in range(1, n + 1)], dtype=np.float64)
        out[pre + "Lflat"] = np.concatenate([p.ravel() for p in pays])
    for j in range(n_sets):
        pre = "s%d_" % j
        out[pre + "meta"] = np.array([got[pre + "map"], got[pre + "n_roots"], *got[pre + "pose"], *got[pre + "limits"]], dtype=np.float64)
        out[pre + "scan"], out[pre + "cand"] = got[pre + "scan"], got[pre + "cand"]
    return out


def main():
    if not os.path.isfile(os.path.join(mg.REFERENCE, "src", "core", "scan_matchers", "m3rsm_engine.h")):
        sys.exit("reference tree not found at %s" % mg.REFERENCE)
    t0 = time.time()
    exe = mg.build()
    out = {"stations": np.array(ps.N_STATIONS)}
    for st in ps.N_STATIONS:
        (kx, ky), _ = ps.N_TABLE[st]
        assert kx % 2 and ky % 2 and 500 <= abs(kx) <= 1500 and 500 <= abs(ky) <= 1500
        maps = mg.make_maps(np.random.RandomState(20261020 + ps.N_SEEDS[st]), SHAPES, shift=(kx, ky), match_shapes=SHAPES[:1])
        for m in maps:
            assert not (0 <= m["origin"][0] < m["w"]) and not (0 <= m["origin"][1] < m["h"])
        got, c = mg.run(exe, maps, crop=True, tag="placed_pyramid_" + st)
        for end in ("_in.bin", "_out.bin"):  # (the dense levels written out whole: a few hundred MB per station)
            os.remove(os.path.join(mg.OUT_DIR, "placed_pyramid_" + st + end))
        assert c["sets"] == 24 and c["one_sided"] >= 10 and c["reached_fine"] >= 4, c
        n_levels = {int(got["m%d_n_levels" % i]) for i in range(len(maps))}
        assert n_levels == {12}, n_levels  # ceil(log2(extent)) + 1 levels above the fine map, 500 ... 1500 cells out
        out.update({"%s_%s" % (st, k): v for k, v in pack(got, len(maps), c["sets"]).items()})
        print(st, c)
    # ---- whole matches: make_golden_m3rsm.py's scenes, harness and assertions (validate(), tight levels, every rectangle a
    # child of an earlier call, the non-prerotated rerun, the rerun with scores times 1 +- 1e-12), one scene per station
    exe_lone = m3.build()
    one_sided = five = 0
    levels = set()
    for st, name in LONE:
        k = [s[0] for s in m3.SCENES].index(name)
        got, a, b, lv = m3.run(exe_lone, m3.make_scenes([(k, m3.SCENES[k])], shift=ps.N_TABLE[st][0]), tag="placed_m3rsm_" + st)
        one_sided, five, levels = one_sided + a, five + b, levels | lv
        assert not (0 <= got["s0_origin"][0] < got["s0_payload"].shape[1])
        out.update({"lone_%s_%s" % (st, key[3:]): v for key, v in got.items() if key.startswith("s0_")})
    # (the three scenes named for this fixture; the one-sided splits of m3rsm.npz come from occ_oblong, which is not among them)
    assert five >= 30 and len(levels) >= 5, (one_sided, five, levels)
    # ---- one many-to-many run whose four requests stand at DIFFERENT stations -- the origin, N1, N2, N3 --, each on a map
    # of its own; make_golden_m3rsm_many.py's harness and assertions, which also run every request's LONE match (the
    # `lone` rows: what K independent matches in one call must return)
    shifts = [(0, 0)] + [ps.N_TABLE[st][0] for st in ps.N_STATIONS]
    spec = ("occ_stations", "occ", [(33, 33, None, 0.1, shifts[0]), (33, 33, None, 0.1, shifts[1]), (37, 29, (11, 20), 0.05, shifts[2]),
                                    (33, 33, None, 0.1, shifts[3])], (0.4, 0.4, 5 * m3.DEG, 1 * m3.DEG, 0.05),
            [(0, 67, (0.13, -0.09, 2.2), 0.5), (1, 40, (-0.08, 0.22, -1.3), 0.2), (2, 67, (0.11, 0.06, -2.4), 0.4), (3, 40, (-0.05, -0.12, 3.3), 0.1)])
    got, _nf, _cut = mm.run(mm.build(), mm.make_scenes([spec]), tag="placed_m3rsm_many")
    out.update({"many_" + key[3:]: v for key, v in got.items() if key.startswith("s0_")})
    print("many-to-many: winner %d, %d calls, lone %s" % (int(got["s0_winner"]), len(got["s0_trace"]), got["s0_lone"][:, 3:].tolist()))
    # ---- one edge scene under the reference's DEFAULT trig provider (make_golden_m3rsm_rawtrig.py's edge_occ, harness and
    # assertions) at N1: 0.125 m cells, so the shift is an exact double and cell edges, cell centres and ranges stay what
    # the recipe needs.  Recorded as behaviour, not demanded: next to (0, 0) this scene tells the providers apart (a
    # direction one ulp off (1, 0) moves an end point across a cell edge); 128 m out that ulp of the RANGE vanishes in the
    # ulp of the COORDINATE, and the raw and the cached provider score every call alike (raw_n_differ = 0).  So the
    # scene is handed over as an ordinary one (edge = 0): every other assertion of that generator holds.
    variant = rt.libm_variant()
    assert variant in (0, 1), "this host's libm is neither build of glibc's sin / cos"
    edge_scenes = rt.make_scenes(small=[], edge=rt.EDGE[:1], shift=ps.N_TABLE["N1"][0])
    edge_scenes[0]["edge"] = 0
    got, n_diff, moved = rt.run(rt.build(), edge_scenes, variant, tag="placed_m3rsm_rawtrig")
    out["raw_n_differ"] = np.array(n_diff)
    print("edge_occ at N1 under the raw provider: %d calls, %d scores differ bitwise from the cached provider's" % (len(got["s0_trace"]), n_diff))
    out.update({"raw_" + key[3:]: v for key, v in got.items() if key.startswith("s0_") and key != "s0_trace_cached"})
    out["raw_libm_variant"], out["raw_n_cached_calls"] = np.array(variant), np.array(len(got["s0_trace_cached"]))
    path = os.path.join(GOLDEN_DIR, "placed_pyramid.npz")
    save_stable(path, out)
    size = os.path.getsize(path)
    assert size <= os.path.getsize(os.path.join(GOLDEN_DIR, "placed.npz")), "placed_pyramid.npz is larger than placed.npz"
    print("wrote placed_pyramid.npz %d KiB in %.0f s; peak resident set of the harness %.2f GB"
          % (size // 1024, time.time() - t0, resource.getrusage(resource.RUSAGE_CHILDREN).ru_maxrss / 1e6))


if __name__ == "__main__":
    main()
