"""GPU suite (-m gpu): slamhip_pyramid_refresh_batch (csrc/map_pyramid.hip: k_pyr_reduce_batch, k_pyr_reduce_tail; the
planning: csrc/pyr_refresh_batch_plan.h) against slamhip_pyramid_refresh of the same jobs one after another in job order.

Every test keeps TWIN pyramids on twin maps, applies the same fine-cell writes to both (map_apply_dirty), refreshes one
set with the batch and the other with lone calls and compares every level bit for bit; then with Pyramid.rebuild and
with pyramid_build_host over the host's copy of the fine map.  The writes LOWER blocks' largest impacts (the cells the
top level's payload comes from go down to an impact below every other cell's), make cells unknown again and, on OCC maps,
sprinkle the payloads 0.96875 and 1.03125: equal impacts, different payloads, so which of them a coarse cell copies is
decided by the winners' fine coordinates -- a level's payload is right only if the COORDINATE plane of the level below is.
A lone refresh of a sub-window on both twins after the batch then reads the planes the batch left."""
import types

import numpy as np
import pytest
from pyramid_cases import bits, golden_map
from test_gpu_pyramid import assert_levels_equal, download_levels

import __graft_entry__ as ge

pytestmark = pytest.mark.gpu

MODELS = {"occ": 64, "tbm": 66}  # golden maps the payloads are taken from: GridCell, TBM
# width, height, origin: the 37 x 29 map; the 9 x 9 window; an oblong map whose external x are mostly positive and whose
# level 1 is 261 cells wide (more than a workgroup); a map whose pyramid is the 1 x 1 level alone
SHAPES = {"big": (37, 29, (11, 20)), "small": (9, 9, (4, 5)), "oblong": (520, 12, (3, 9)), "tiny": (2, 2, (1, 1))}
TIE = (0.96875, 1.03125)  # OCC payloads of equal impact under either OIE's discrepancy form: 1 - |p - 1|


@pytest.fixture(scope="module")
def pkg():
    return ge.load_package()


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


class Twin:
    """one map twice on the device (ids base and base + 20, levels behind each) and once on the host"""

    def __init__(self, pkg, ctx, model, shape, base, seed):
        g = golden_map(MODELS[model])
        w, h, origin = SHAPES[shape]
        self.pkg, self.ctx, self.oie, self.base = pkg, ctx, g.oie, base
        self.stride = pkg.STRIDE[g.cell_model]
        rs = np.random.RandomState(seed)
        known = ~np.all(bits(g.payload) == bits(g.unknown), axis=-1)
        self.donors = g.payload[known]
        self.unknown = np.asarray(g.unknown, dtype=np.float64)[:self.stride]
        self.low = np.array([1.0 / 1024]) if self.stride == 1 else np.array([0.1, 0.9, 0.0, 0.0])  # below every donor's impact
        payload = np.empty((h, w, self.stride))
        payload[...] = self.unknown
        fill = rs.rand(h, w) < 0.6
        payload[fill] = self.donors[rs.randint(len(self.donors), size=int(fill.sum()))]
        self.m = types.SimpleNamespace(cell_model=g.cell_model, payload=payload, origin=origin, scale=0.05, unknown=g.unknown,
                                       width=w, height=h)
        self.rs = rs
        self.pyr = []
        for fine in (base, base + 20):
            ctx.upload_map(fine, self.m)
            self.pyr.append(pkg.Pyramid(ctx, fine, self.oie, fine + 1))
        self.a, self.b = self.pyr  # a: refreshed by the batch, b: by lone calls

    def write(self, x0, y0, w, h):
        """writes inside the window, to both twins and the host copy"""
        cells = [(x0 + dx, y0 + dy) for dy in range(h) for dx in range(w)]
        if len(cells) > 96:
            pick = self.rs.choice(len(cells), 90, replace=False)
            corners = [0, w - 1, len(cells) - w, len(cells) - 1]
            cells = [cells[i] for i in sorted(set(pick.tolist() + corners))]
        vals = []
        for j, _ in enumerate(cells):
            kind = j % 5
            if kind == 0:
                vals.append(self.unknown)
            elif kind in (1, 2) and self.stride == 1:
                vals.append(np.array([TIE[(j // 5 + kind) % 2]]))
            elif kind == 3:
                vals.append(self.low)
            else:
                vals.append(self.donors[self.rs.randint(len(self.donors))])
        # the cells the top level's payload comes from go DOWN, where the window holds them
        top = self.ctx.map_download_window(self.a.info()[-1]["map_id"], 0, 0, 1, 1, self.stride)[0, 0]
        for y, x in np.argwhere(np.all(bits(self.m.payload) == bits(top), axis=-1)):
            if x0 <= x < x0 + w and y0 <= y < y0 + h:
                if (int(x), int(y)) in cells:
                    vals[cells.index((int(x), int(y)))] = self.low
                else:
                    cells.append((int(x), int(y)))
                    vals.append(self.low)
        for fine in (self.base, self.base + 20):
            self.ctx.map_apply_dirty(fine, cells, np.asarray(vals))
        for (x, y), v in zip(cells, vals):
            self.m.payload[y, x] = v

    def levels(self, which):
        return download_levels(self.ctx, self.pyr[which], self.stride)

    def check(self):
        """a's levels are b's, a rebuild's and the host build's"""
        got = self.levels(0)
        assert_levels_equal(got, self.levels(1))
        assert_levels_equal(got, self.pkg.pyramid_build_host(self.m, self.oie))
        self.b.rebuild()
        assert_levels_equal(got, self.levels(1))

    def close(self):
        for p in self.pyr:
            p.close()
        for fine in (self.base, self.base + 20):
            self.ctx.map_release(fine)


def run_jobs(ctx, twins, jobs):
    """jobs = [(twin, x0, y0, w, h)]: the writes, the batch on the a side, lone calls in job order on the b side, the check;
    then a lone refresh of the window's first cells on BOTH sides (it reads the coordinate planes the batch left)"""
    for t, x0, y0, w, h in jobs:
        t.write(x0, y0, w, h)
    ctx.pyramid_refresh_batch([(t.a, x0, y0, w, h) for t, x0, y0, w, h in jobs])
    stats = ctx.pyramid_refresh_batch_stats()
    for t, x0, y0, w, h in jobs:
        t.b.refresh(x0, y0, w, h)
    for t in {id(j[0]): j[0] for j in jobs}.values():
        t.check()
    for t, x0, y0, w, h in jobs:
        w2, h2 = min(w, 2), min(h, 2)
        t.write(x0, y0, w2, h2)
        t.a.refresh(x0, y0, w2, h2)
        t.b.refresh(x0, y0, w2, h2)
    for t in {id(j[0]): j[0] for j in jobs}.values():
        t.check()
    return stats


def flat_levels(t, x0, y0, w, h):
    """levels of the job whose window has more than 256 cells, counted from the level geometry"""
    ox, oy = t.m.origin
    n, info = 0, t.a.info()
    for lv, g in enumerate(info[:-1], 1):
        cw = ((x0 + w - 1 - ox) >> lv) - ((x0 - ox) >> lv) + 1
        ch = ((y0 + h - 1 - oy) >> lv) - ((y0 - oy) >> lv) + 1
        assert cw <= g["width"] and ch <= g["height"]
        n += cw * ch > 256
    return n


@pytest.fixture(params=list(MODELS))
def twins(pkg, ctx, request):
    ts = {s: Twin(pkg, ctx, request.param, s, 100 + 40 * k, seed=5 + k) for k, s in enumerate(SHAPES)}
    yield ts
    for t in ts.values():
        t.close()


# ---- 1, 2. shapes and windows ---------------------------------------------------------------------------------
def test_shapes_and_windows(ctx, twins):
    assert len(twins["tiny"].a.info()) == 1 and twins["oblong"].a.info()[0]["width"] == 261
    assert len({len(t.a.info()) for t in twins.values()}) >= 3  # pyramids of different heights in one launch
    whole = [(t, 0, 0, t.m.width, t.m.height) for t in twins.values()]
    # 1 x 1 in a corner (the first and the last cell)
    st = run_jobs(ctx, twins, [(t, 0, 0, 1, 1) for t in twins.values()])
    assert st == dict(rounds=1, jobs_shared=4, jobs_lone=0, launches=1)  # every level in the tail
    run_jobs(ctx, twins, [(t, t.m.width - 1, t.m.height - 1, 1, 1) for t in twins.values()])
    # windows across the external axes: the floor of negative coordinates
    run_jobs(ctx, twins, [(t, max(t.m.origin[0] - 3, 0), max(t.m.origin[1] - 2, 0), min(6, t.m.width), min(5, t.m.height))
                          for t in twins.values()])
    # the whole maps
    st = run_jobs(ctx, twins, whole)
    assert st["rounds"] == 1 and st["launches"] == 1 + max(flat_levels(*j) for j in whole)
    assert flat_levels(*whole[2]) >= 2 > flat_levels(*whole[0]) >= 1  # (the oblong map leaves the flat launches last)
    # a level-1 window of exactly 256 cells (tail alone) and of 257 (one flat launch of two workgroups, then the tail)
    ob = twins["oblong"]
    assert flat_levels(ob, 1, 9, 512, 1) == 0 and flat_levels(ob, 1, 9, 514, 1) == 1
    st = run_jobs(ctx, twins, [(ob, 1, 9, 512, 1)])
    assert st == dict(rounds=1, jobs_shared=1, jobs_lone=0, launches=1)
    st = run_jobs(ctx, twins, [(ob, 1, 9, 514, 1)])
    assert st == dict(rounds=1, jobs_shared=1, jobs_lone=0, launches=2)
    # ... and as the wide job among small ones
    run_jobs(ctx, twins, [(twins["small"], 2, 2, 3, 3), (ob, 1, 8, 514, 3), (twins["tiny"], 1, 0, 1, 2), (twins["big"], 0, 0, 37, 29)])


# ---- 3. the same pyramid twice in one call -------------------------------------------------------------------------
def test_the_same_pyramid_twice_takes_two_rounds(ctx, twins):
    big, small, ob = twins["big"], twins["small"], twins["oblong"]
    # overlapping windows on `big`: the second job's levels read what the first one's wrote
    st = run_jobs(ctx, twins, [(big, 0, 0, 20, 20), (small, 0, 0, 9, 9), (big, 10, 10, 27, 19), (ob, 0, 0, 520, 12)])
    assert st["rounds"] == 2 and st["jobs_shared"] == 4 and st["jobs_lone"] == 0
    # ... and a third window on it a third round (a job whose pyramid the open round holds closes that round)
    st = run_jobs(ctx, twins, [(ob, 0, 0, 520, 12), (ob, 100, 0, 3, 3), (big, 3, 3, 30, 20), (ob, 258, 5, 4, 4)])
    assert st["rounds"] == 3 and st["jobs_shared"] == 4


# ---- 4. a level with a probability plane ---------------------------------------------------------------------------
def test_a_level_with_a_probability_plane_goes_lone(pkg, ctx):
    t = Twin(pkg, ctx, "tbm", "big", 100, seed=9)
    other = Twin(pkg, ctx, "tbm", "small", 140, seed=10)
    n = 40
    ang = np.linspace(-2.0, 2.0, n)
    ctx.scan_upload(np.full(n, 0.4), np.cos(ang), np.sin(ang), np.ones(n))
    cfg = pkg.spe_cfg(oope=pkg.OOPE_OBSTACLE, oie=t.oie)
    poses = np.array([[0.1, -0.2, 0.3], [0.0, 0.0, 0.0], [-0.2, 0.1, 2.0]])
    lv = [p.info()[0]["map_id"] for p in t.pyr]
    for i in lv:  # the 1-cell OOPE on level 1 of both twins: the level gets its probability plane
        ctx.score_poses(i, cfg, poses)
    st = run_jobs(ctx, [t, other], [(other, 0, 0, 9, 9), (t, 0, 0, 37, 29), (other, 3, 3, 2, 2)])
    assert st["jobs_lone"] == 1 and st["jobs_shared"] == 2 and st["rounds"] == 2
    got, want = ctx.score_poses(lv[0], cfg, poses), ctx.score_poses(lv[1], cfg, poses)
    np.testing.assert_array_equal(bits(got), bits(want))
    # ... and what a map that never had a plane gives: the level's cells uploaded under an id of their own
    level = t.levels(0)[0]
    h, w = level["payload"].shape[:2]
    ctx.upload_map(400, types.SimpleNamespace(cell_model=t.m.cell_model, payload=level["payload"], origin=level["origin"],
                                              scale=level["scale"], unknown=t.m.unknown, width=w, height=h))
    np.testing.assert_array_equal(bits(got), bits(ctx.score_poses(400, cfg, poses)))
    ctx.map_release(400)
    t.close()
    other.close()


# ---- 5. launch count -----------------------------------------------------------------------------------------------
def test_launch_count(ctx, twins):
    jobs = [(twins["big"], 0, 0, 37, 29), (twins["small"], 0, 0, 9, 9), (twins["oblong"], 0, 0, 520, 12)]
    st = run_jobs(ctx, twins, jobs)
    assert st["rounds"] == 1
    assert st["launches"] <= max(flat_levels(*j) for j in jobs) + 1
    assert st["launches"] < sum(len(j[0].a.info()) for j in jobs)
    for k in (2, 3):
        st = run_jobs(ctx, twins, jobs[:k])
        assert st["launches"] < sum(len(j[0].a.info()) for j in jobs[:k])


# ---- 6. batch calls back to back ------------------------------------------------------------------------------------
def test_batch_calls_back_to_back(ctx, twins):
    big, small, ob, tiny = (twins[s] for s in SHAPES)
    calls = [[(big, 0, 0, 37, 29), (small, 1, 1, 4, 4)], [(ob, 0, 0, 520, 12), (big, 5, 5, 9, 9), (tiny, 0, 0, 2, 2)],
             [(small, 0, 0, 9, 9)], [(ob, 7, 2, 300, 5), (big, 30, 0, 7, 29)], [(big, 0, 20, 37, 9), (ob, 0, 0, 2, 2)]]
    for jobs in calls:  # (all the writes first: nothing between the calls waits for the stream)
        for t, x0, y0, w, h in jobs:
            t.write(x0, y0, w, h)
    for jobs in calls:  # the job tables' staging takes turns: the third call fills the block the first one sent
        ctx.pyramid_refresh_batch([(t.a, x0, y0, w, h) for t, x0, y0, w, h in jobs])
    for jobs in calls:
        for t, x0, y0, w, h in jobs:
            t.b.refresh(x0, y0, w, h)
    for t in twins.values():
        t.check()


# ---- 7. errors ------------------------------------------------------------------------------------------------------
def test_errors_queue_nothing(pkg, ctx, twins):
    big, small = twins["big"], twins["small"]
    ctx.pyramid_refresh_batch([])  # no jobs: OK, nothing happens
    run_jobs(ctx, twins, [(big, 0, 0, 5, 5)])
    last = ctx.pyramid_refresh_batch_stats()
    # a write the refused calls would have carried up the levels
    big.write(0, 0, 37, 29)
    before = big.levels(0)
    other_ctx = pkg.Context(0)
    other_ctx.upload_map(0, small.m)
    foreign = pkg.Pyramid(other_ctx, 0, small.oie, 1)
    stale = Twin(pkg, ctx, "occ", "small", 300, seed=3)
    stale_before = stale.levels(0)
    ctx.map_bind(300, stale.m.cell_model, 20, 20, (10, 10), stale.m.scale, stale.m.unknown)  # the fine map moves
    good = (big.a, 0, 0, 37, 29)
    for bad, code in (((stale.a, 0, 0, 1, 1), "-4"), ((big.a, 30, 0, 8, 4), "-1"), ((big.a, 0, 0, 0, 1), "-1"),
                      ((small.a, -1, 0, 2, 2), "-1"), ((foreign, 0, 0, 1, 1), "-1"), ((None, 0, 0, 1, 1), "-1")):
        with pytest.raises(pkg.SlamHipError, match=code):
            ctx.pyramid_refresh_batch([good, bad])
        assert_levels_equal(big.levels(0), before)
        assert ctx.pyramid_refresh_batch_stats() == last
    assert_levels_equal(stale.levels(1), stale_before)
    foreign.close()
    other_ctx.close()
    # the same job alone goes through
    ctx.pyramid_refresh_batch([good])
    big.b.refresh(0, 0, 37, 29)
    big.check()
    stale.a.rebuild()
    stale.close()


# ---- 8. a match after the batch refresh ------------------------------------------------------------------------------
def test_match_after_batch_refresh_equals_match_over_fresh_pyramids(pkg, ctx):
    from test_gpu_m3rsm_many import SCENE_NAMES, Scene, golden_scene
    from test_gpu_m3rsm_many import bits as tbits
    scene = Scene(pkg, ctx, golden_scene(SCENE_NAMES.index("occ_m2m")))
    s = scene.s
    m = scene.matcher(strict=True)
    before = m.m3rsm_match_many(scene.table)
    assert before["request"] == s.winner
    # request 2's scan, shortened so that no beam leaves the window, written into map 1 from a pose beside its own, and a
    # few cells of map 0 made walls: impacts change on the levels of BOTH pyramids, one batch refresh brings them up
    rq = s.requests[2]
    pose = rq.pose + np.array([0.04, -0.03, 0.02])
    assert ctx.map_append_scan(10, pkg.RULE_LAST, pose, 0.8 * rq.scan[:, 0], rq.scan[:, 1], rq.scan[:, 2]) > 0
    m0, m1 = s.maps
    cells = [(x, m0.height // 2) for x in range(2, m0.width - 2)]
    ctx.map_apply_dirty(0, cells, np.ones((len(cells), 1)))
    ctx.pyramid_refresh_batch([(scene.pyr[1], 0, 0, m1.width, m1.height), (scene.pyr[0], 2, m0.height // 2, m0.width - 4, 1)])
    assert ctx.pyramid_refresh_batch_stats()["jobs_shared"] == 2
    after = m.m3rsm_match_many(scene.table)
    trace_after = m.m3rsm_trace_many()
    assert len(trace_after) != len(s.trace) or not np.array_equal(tbits(trace_after), tbits(s.trace))  # the maps did change
    m.close()
    scene.matchers.remove(m)
    for j in (0, 1):
        scene.pyr[j].close()
        scene.pyr[j] = pkg.Pyramid(ctx, 10 * j, s.oie, 10 * j + 1)
    scene.table = [(scene.pyr[r.map], k, r.pose) for k, r in enumerate(s.requests)]
    fresh = scene.matcher(strict=True)
    want = fresh.m3rsm_match_many(scene.table)
    np.testing.assert_array_equal(tbits(trace_after), tbits(fresh.m3rsm_trace_many()))
    assert after["request"] == want["request"] and after["prob"] == want["prob"]
    np.testing.assert_array_equal(tbits(after["delta"]), tbits(want["delta"]))
    scene.close()
