"""GPU suite (-m gpu): the scratch blocks a context keeps between calls (csrc/hip_block.h: owners, grow_block,
grow_blocks) across a growth.  Every case is a sequence on ONE context -- a small call, one just past the block's floor,
the small one again -- and every result is bit-equal to the same call made on a fresh context that saw only that call:
a block that grew holds what the kernels need at the new size, and a block that stayed is still the one its capacity
names.  The shapes are the smallest that cross a floor: 2048 beams (the lone map update, run under each
SLAMHIP_OPT_K6_PATH so that the record, bin, line and marker blocks all grow), 64 jobs (the batched update's status
pairs), 1024 dirty cells, 256 poses (with the beam-order sum: the terms), 256 pyramid candidates, the 65536 bytes of the
multi-request stage, a stored scan re-stored at 2049 points with angles.  The last test runs everything on one context,
destroys it and repeats the small calls on a second one made in the same process.  The error paths (a failed allocation
at every point of a growth) are tests/test_hip_block_host.py's: no allocation is made to fail here."""
import types

import numpy as np
import pytest

import __graft_entry__ as ge

pytestmark = pytest.mark.gpu

SMALL, BIG = 0, 1
SEQUENCE = (SMALL, BIG, SMALL)


@pytest.fixture(scope="module")
def pkg():
    return ge.load_package()


def occ_map(side, seed, origin=None):
    rs = np.random.RandomState(seed)
    payload = np.where(rs.uniform(size=(side, side, 1)) < 0.3, rs.uniform(0.6, 1.0, (side, side, 1)), rs.uniform(0.0, 0.4, (side, side, 1)))
    return types.SimpleNamespace(cell_model=0, scale=0.1, origin=origin or (side // 2, side // 2), unknown=[0.5],
                                 payload=np.ascontiguousarray(payload), width=side, height=side)


def fan_scan(n, seed, lo, hi):
    """n beams with ascending directions over less than a turn (what a laser's are), ranges in [lo, hi] metres"""
    rs = np.random.RandomState(seed)
    ang = np.linspace(-2.3, 2.3, n)
    return rs.uniform(lo, hi, n), ang, (rs.uniform(size=n) < 0.8).astype(np.int32)


def point_scan(n, seed, reach):
    rs = np.random.RandomState(seed)
    ang = rs.uniform(-np.pi, np.pi, n)
    return rs.uniform(0.3, 1.3, n) * reach, np.cos(ang), np.sin(ang), np.full(n, 1.0 / n), rs.uniform(0.5, 1.0, n), ang


# ---- the cases: run(pkg, ctx, which) makes the call of size `which` on ctx and returns its results as arrays ----------
def lone_update(path):
    def run(pkg, ctx, which):
        ctx.set_option(pkg.OPT_K6_PATH, path)
        ctx.map_bind(0, pkg.CELL_OCC, 64, 64, (32, 32), 0.1, [0.5])
        # 2049 beams of 2.5 .. 2.9 m cross some 35 cells each: more records than the record blocks' floor of 65536
        rng, ang, occ = fan_scan(16, 3, 0.5, 2.5) if which == SMALL else fan_scan(2049, 4, 2.5, 2.9)
        nu = ctx.map_append_scan(0, pkg.RULE_MEAN, (0.02, -0.03, 0.3), rng, np.cos(ang), np.sin(ang), is_occ=occ, blur=0.15)
        if which == BIG:
            assert nu > 65536, nu
        out = [np.array([nu]), ctx.map_download_window(0, 0, 0, 64, 64, 1), ctx.map_download_aux(0, 0, 0, 64, 64, 1)]
        ctx.map_release(0)  # (a re-bind would carry the cells over)
        return out
    return run


def batch_update(pkg, ctx, which):
    K = 2 if which == SMALL else 65  # (the status pairs' floor is 64 jobs)
    ctx.set_option(pkg.OPT_K6_PATH, 0)  # (the shared launches are the default path's)
    jobs = []
    for k in range(K):
        ctx.map_bind(k, pkg.CELL_OCC, 32, 32, (16, 16), 0.1, [0.5])
        rng, ang, occ = fan_scan(16, 100 + k, 0.3, 1.4)
        jobs.append(dict(map_id=k, pose=(0.01 * (k % 7), -0.02, 0.1 * (k % 5)), range=rng, cos_a=np.cos(ang), sin_a=np.sin(ang),
                         is_occ=occ))
    nu, st = ctx.map_append_scan_batch(pkg.RULE_MEAN, jobs, blur=0.1)
    stats = ctx.map_update_batch_stats()
    assert stats["jobs_shared"] == K and stats["jobs_lone"] == 0, stats  # (the shared launches took the jobs)
    out = [nu, st] + [ctx.map_download_window(k, 0, 0, 32, 32, 1) for k in range(K)]
    for k in range(K):
        ctx.map_release(k)
    return out


def dirty_log(pkg, ctx, which):
    n = 8 if which == SMALL else 1025
    rs = np.random.RandomState(20 + which)
    ctx.upload_map(0, occ_map(64, 1))
    cells = rs.permutation(64 * 64)[:n]
    ctx.map_apply_dirty(0, np.column_stack([cells % 64, cells // 64]), rs.uniform(size=(n, 1)))
    out = [ctx.map_download_window(0, 0, 0, 64, 64, 1)]
    ctx.map_release(0)
    return out


def score_poses(sum_order):
    def run(pkg, ctx, which):
        n = 8 if which == SMALL else 257
        ctx.upload_map(0, occ_map(64, 2))
        ctx.scan_upload(*point_scan(37, 5, 1.5)[:5])
        poses = np.random.RandomState(30 + which).uniform(-0.3, 0.3, (n, 3))
        out = [ctx.score_poses(0, pkg.spe_cfg(sum_order=sum_order, pose_trig=pkg.POSE_TRIG_HOST), poses)]
        ctx.map_release(0)
        return out
    return run


def candidates(n, seed):
    rs = np.random.RandomState(seed)
    lo = rs.uniform(-0.4, 0.2, (n, 2))
    rect = np.column_stack([lo[:, 0], lo[:, 0] + rs.uniform(0.0, 0.3, n), lo[:, 1], lo[:, 1] + rs.uniform(0.0, 0.3, n)])
    return rs.uniform(-0.2, 0.2, n), rect


def pyramid_scores(sum_order):
    def run(pkg, ctx, which):
        n = 8 if which == SMALL else 257
        ctx.upload_map(0, occ_map(32, 6))
        ctx.scan_upload(*point_scan(33, 7, 0.6)[:5])
        pyr = pkg.Pyramid(ctx, 0)
        try:
            rot, rect = candidates(n, 40 + which)
            cfg = pkg.spe_cfg(oope=pkg.OOPE_MAX, sum_order=sum_order, pose_trig=pkg.POSE_TRIG_HOST)
            return list(pyr.score_matches(cfg, (0.03, -0.02, 0.2), rot, rect))
        finally:
            pyr.close()
            ctx.map_release(0)
    return run


def request_stage(pkg, ctx, which):
    # a candidate takes 112 bytes of the stage (68 in, 44 out) behind the request table: 600 of them cross its 65536
    n = 8 if which == SMALL else 600
    ctx.upload_map(0, occ_map(32, 8))
    pyr = pkg.Pyramid(ctx, 0)
    try:
        for slot, beams in enumerate((5, 33)):
            ctx.scan_store(slot, *point_scan(beams, 50 + slot, 0.6)[:5])
        table = [(pyr, 0, (0.03, -0.02, 0.2)), (pyr, 1, (-0.05, 0.04, -1.1))]
        rot, rect = candidates(n, 60 + which)
        cfg = pkg.spe_cfg(oope=pkg.OOPE_MAX, sum_order=pkg.SUM_SEQUENTIAL, pose_trig=pkg.POSE_TRIG_HOST)
        return list(pkg.Pyramid.score_requests(ctx, cfg, table, np.arange(n) % 2, rot, rect))
    finally:
        pyr.close()
        ctx.map_release(0)


def stored_scan(pkg, ctx, which):
    n = 16 if which == SMALL else 2049
    ctx.upload_map(0, occ_map(32, 9))
    *scan, ang = point_scan(n, 70 + which, 0.6)
    ctx.scan_store(3, *scan)
    ctx.scan_store_angles(3, ang)
    ctx.scan_select(3)
    out = [ctx.scan_download(), ctx.score_poses(0, pkg.spe_cfg(), np.random.RandomState(71).uniform(-0.2, 0.2, (8, 3)))]
    if pkg.libm_variant() >= 0:  # the slot's angles in HBM, read by the exact tabulation of a multi-request launch
        pyr = pkg.Pyramid(ctx, 0)
        try:
            rot, rect = candidates(8, 72)
            cfg = pkg.spe_cfg(oope=pkg.OOPE_MAX, pose_trig=pkg.POSE_TRIG_RAW_EXACT)
            out += list(pkg.Pyramid.score_requests(ctx, cfg, [(pyr, 3, (0.03, -0.02, 0.2))], np.zeros(8, np.int32), rot, rect))
        finally:
            pyr.close()
    ctx.map_release(0)
    return out


CASES = {
    "lone_update_path0": lone_update(0),
    "lone_update_path1": lone_update(1),
    "lone_update_path2": lone_update(2),
    "batch_update": batch_update,
    "dirty_log": dirty_log,
    "score_poses": score_poses(0),
    "score_poses_beam_order": score_poses(1),
    "pyramid_scores": pyramid_scores(0),
    "pyramid_scores_beam_order": pyramid_scores(1),
    "request_stage": request_stage,
    "stored_scan": stored_scan,
}

_fresh = {}


def fresh(pkg, name, which):
    """the call of size `which` of a case on a context that saw nothing else: made once, shared, never written"""
    if (name, which) not in _fresh:
        ctx = pkg.Context(0)
        try:
            out = CASES[name](pkg, ctx, which)
        finally:
            ctx.close()
        for a in out:
            a.setflags(write=False)
        _fresh[(name, which)] = out
    return _fresh[(name, which)]


def check_equal(got, want, what):
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(g, w, err_msg="%s, output %d" % (what, i))


@pytest.mark.parametrize("name", list(CASES))
def test_results_across_a_growth_equal_a_fresh_contexts(pkg, name):
    ctx = pkg.Context(0)
    try:
        for step, which in enumerate(SEQUENCE):
            check_equal(CASES[name](pkg, ctx, which), fresh(pkg, name, which), "%s, call %d of the sequence" % (name, step))
    finally:
        ctx.close()


def test_a_context_made_after_one_that_grew_everything_was_destroyed(pkg):
    first = pkg.Context(0)
    try:
        for name in CASES:
            for which in SEQUENCE:
                CASES[name](pkg, first, which)
    finally:
        first.close()
    second = pkg.Context(0)
    try:
        for name in CASES:
            check_equal(CASES[name](pkg, second, SMALL), fresh(pkg, name, SMALL), "%s on the second context" % name)
    finally:
        second.close()
