"""GPU suite: the GMapping scorer (K3, csrc/gm_score_device.h) and the neighbourhood masks it reads, on windows that are
NO squares and on the seams of a tile pool.

Everything else the suite scores GMapping on is a tests/synth.py square with equal origin components, or a crop of a
golden that keeps 60 cells between its end cells and the rims; a tile pool is never scored cell for cell against the
same cells held densely.  An exchange of width and height in one of the rim tests, of pitch and tile rows, of the
origin's components, or a mask bit put into the wrong column across a tile seam passes all of that.

Section 1, dense windows -- tests/golden/gmapping_oblong.npz (the compiled reference on 77 x 45 and 45 x 77 cells, end
cells on / next to / beyond every rim and corner; tests/gmapping_oblong_cases.py, pinned on the CPU by
tests/test_oracle_gmapping_oblong.py):
  a. every launch form of K3 (1 / 160 / 161 / 2048 poses per call, 1 ... 2048 beams) at the project's bars: the golden
     1e-11, the oracle 1e-12, the exact mode bit for bit, one form against another bit for bit;
  b. the nine-cell form against the mask form, odd thresholds, the generic window loop;
  c. the masks after every kind of writer (K6 in its three pipelines, the dirty log, partial uploads, growth);
  d. hill climbing in every chain mode and the particle filter on the wide map.
Section 2, tile pools of 3 x 1, 1 x 3 and 3 x 2 tiles: a 1-particle filter through its tile table against the same
cells uploaded as ONE dense window (bit for bit), walls drawn across the seams, masks and settle states after every
write."""
import ctypes as C

import numpy as np
import pytest
from gmapping_oblong_cases import (GROUPS, INNER_GROUPS, MAPS, RIM_GROUPS, SCALE, SCANS, all_poses, golden, golden_map,
                                   golden_scan, group_poses, group_scores, group_slices, hc_scan, pf_step)
from helpers import assert_trace_equal, trace

import __graft_entry__ as ge

pytestmark = pytest.mark.gpu

UNKNOWN = [-1.0, 0.0, 0.0]
K6_PATHS = {"gather": 0, "counting": 1, "radix": 2}
TILE = 128


@pytest.fixture(scope="module")
def pkg():
    return ge.load_package()


@pytest.fixture(scope="module")
def po():
    import pyoracle
    return pyoracle


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def tctx(pkg):
    c = pkg.Context(0, testing=True)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fresh(pkg):
    c = pkg.Context(0, testing=True)
    yield c
    c.close()


@pytest.fixture(scope="module")
def variant(pkg):
    v = pkg.libm_variant()
    if v < 0:
        pytest.skip("this host's libm is neither build of glibc's sin / cos / exp: no exact modes here")
    return v


def rebind(pkg, ctx, map_id, m):
    """upload_map on an id that holds nothing (a re-bind alone keeps the cells -- and the masks -- of a bound window)"""
    try:
        ctx.map_release(map_id)
    except pkg.SlamHipError:
        pass
    ctx.upload_map(map_id, m)


def upload_scan(pkg, ctx, scan, exact=False):
    if scan.trig_mode == 1:
        idx = np.round((scan.angle - scan.a_min) / scan.a_delta).astype(np.int64)
        c, s = scan.tab_cos[idx], scan.tab_sin[idx]
    else:
        c, s = pkg.beam_trig(scan.angle)
    ctx.scan_upload(scan.range, c, s, scan.weight, scan.factor)
    if exact:
        ctx.scan_set_angles(scan.angle)


def score(ctx, map_id, cfg, poses):
    ctx.gm_cache_reset()  # every sequence starts from an empty OOPE cache, as every scorer object of the generator did
    return ctx.score_poses(map_id, cfg, poses)


def oracle_scores(oracle, po, m, scan, poses, **kw):
    return oracle.score_poses(m, scan, po.make_cfg(oope=po.OOPE_GMAPPING, **kw), poses, po.Oracle.new_gm_cache())


def masks(ctx, map_id):
    valid, bad = C.c_int(-1), C.c_longlong(-1)
    assert ctx.L.slamhip_map_debug_nbr_masks(ctx.h, map_id, C.byref(valid), C.byref(bad)) == 0
    return valid.value, bad.value


def pool_masks(ctx, pf):
    valid, bad, bad_states = C.c_int(-1), C.c_longlong(-1), C.c_longlong(-1)
    assert ctx.L.slamhip_gmapping_debug_nbr_masks(pf.h, C.byref(valid), C.byref(bad)) == 0
    assert ctx.L.slamhip_gmapping_debug_settle_states(pf.h, C.byref(bad_states)) == 0
    return (valid.value, bad.value), bad_states.value


# ======================================================================================================================
# Section 1a: every launch form of K3 on both maps
@pytest.mark.parametrize("key", SCANS)
@pytest.mark.parametrize("name", list(MAPS))
def test_every_launch_form_vs_golden_and_oracle(pkg, ctx, po, oracle, name, key):
    """Per group (one sequence, one cache) against the golden at 1e-11 and the oracle at 1e-12, host and device pose
    trigonometry.  Then the golden's 92 poses tiled to 1 / 160 / 161 / 2048 poses per call -- k_score_gmapping_wide<K, 1024>,
    k_score_gmapping<K, true>, <K, false> (score_kernels.hip launch_score) -- against the oracle over the same sequence
    with one cache, and one form against another bit for bit."""
    g = golden()
    m, scan = golden_map(g, name), golden_scan(g, name, key)
    rebind(pkg, ctx, 0, m)
    upload_scan(pkg, ctx, scan)
    for th in (0.1, 0.5):
        for grp in GROUPS:
            poses, want = group_poses(g, name, key, grp), group_scores(g, name, key, grp, th)
            msg = "%s th %g" % (grp, th)
            host = score(ctx, 0, pkg.spe_cfg(oope=pkg.OOPE_GMAPPING, gm_th=th, pose_trig=1), poses)
            np.testing.assert_allclose(host, want, rtol=1e-11, atol=1e-300, err_msg=msg)
            np.testing.assert_allclose(host, oracle_scores(oracle, po, m, scan, poses, gm_th=th), rtol=1e-12, atol=0,
                                       err_msg=msg)
            dev = score(ctx, 0, pkg.spe_cfg(oope=pkg.OOPE_GMAPPING, gm_th=th), poses)
            np.testing.assert_allclose(dev, want, rtol=1e-11, atol=1e-300, err_msg=msg)
    seq = all_poses(g, name, key)
    cfg = pkg.spe_cfg(oope=pkg.OOPE_GMAPPING, pose_trig=1)
    got = {}
    for count in (1, 160, 161, 2048):
        tiled = np.resize(seq, (count, 3))
        got[count] = score(ctx, 0, cfg, tiled)
        np.testing.assert_allclose(got[count], oracle_scores(oracle, po, m, scan, tiled), rtol=1e-12, atol=0,
                                   err_msg="%d poses per call" % count)
    np.testing.assert_array_equal(got[2048][:161], got[161])
    np.testing.assert_array_equal(got[161][:160], got[160])
    np.testing.assert_array_equal(got[160][:1], got[1])
    # split calls carry the cache across the call boundary: the same bits
    ctx.gm_cache_reset()
    parts = np.concatenate([ctx.score_poses(0, cfg, np.resize(seq, (161, 3))[:37]),
                            ctx.score_poses(0, cfg, np.resize(seq, (161, 3))[37:])])
    np.testing.assert_array_equal(parts, got[161])
    ctx.map_release(0)


@pytest.mark.parametrize("key", [k for k in SCANS if not k.endswith("c")])
@pytest.mark.parametrize("name", list(MAPS))
def test_exact_mode_vs_golden_bit_for_bit(pkg, ctx, variant, name, key):
    """SUM_SEQUENTIAL + POSE_TRIG_RAW_EXACT (k_score_gmapping_exact, exact_kernels.hip): the reference's bits"""
    g = golden()
    m, scan = golden_map(g, name), golden_scan(g, name, key)
    rebind(pkg, ctx, 0, m)
    upload_scan(pkg, ctx, scan, exact=True)
    for th in (0.1, 0.5):
        cfg = pkg.spe_cfg(oope=pkg.OOPE_GMAPPING, gm_th=th, sum_order=pkg.SUM_SEQUENTIAL, pose_trig=pkg.POSE_TRIG_RAW_EXACT)
        for grp in GROUPS:
            np.testing.assert_array_equal(score(ctx, 0, cfg, group_poses(g, name, key, grp)),
                                          group_scores(g, name, key, grp, th), err_msg="%s th %g" % (grp, th))
    ctx.map_release(0)


@pytest.mark.parametrize("n_beams", [1138, 2048])
@pytest.mark.parametrize("name", list(MAPS))
def test_beam_counts_beyond_the_golden_vs_oracle(pkg, ctx, po, oracle, name, n_beams):
    """1138 beams: the first count a 1024-thread workgroup scores without helper lanes; 2048: the most K3 holds.  The
    1080-beam scan repeated, every repetition turned a little, in all three launch forms.  2049 beams: the refusal
    include/slamhip.h documents for slamhip_score_poses."""
    g = golden()
    m, base = golden_map(g, name), golden_scan(g, name, "s1080")
    turn = 0.0021 * (np.arange(n_beams) // base.n)
    scan = po.ScanData(np.resize(base.range, n_beams), np.resize(base.angle, n_beams) + turn)
    rebind(pkg, ctx, 0, m)
    upload_scan(pkg, ctx, scan)
    cfg = pkg.spe_cfg(oope=pkg.OOPE_GMAPPING, pose_trig=1)
    seq = all_poses(g, name, "s1080")
    got = {}
    for count in (len(seq), 161, 2048):  # k_score_gmapping_wide<K, 1024>, k_score_gmapping<K, true>, <K, false>
        tiled = np.resize(seq, (count, 3))
        got[count] = score(ctx, 0, cfg, tiled)
        np.testing.assert_allclose(got[count], oracle_scores(oracle, po, m, scan, tiled), rtol=1e-12, atol=0)
    np.testing.assert_array_equal(got[161][:len(seq)], got[len(seq)])
    np.testing.assert_array_equal(got[2048][:161], got[161])
    assert np.count_nonzero(got[161]) > 60
    if n_beams == 2048:
        upload_scan(pkg, ctx, po.ScanData(np.resize(base.range, 2049), np.resize(base.angle, 2049)))
        with pytest.raises(pkg.SlamHipError, match=r"slamhip error -1: .*the GMapping kernel holds at most 2048 filtered beams per scan"):
            score(ctx, 0, cfg, seq[:2])
    ctx.map_release(0)


# ======================================================================================================================
# Section 1b: nine-cell form against mask form
@pytest.mark.parametrize("name", list(MAPS))
def test_nine_cell_form_equals_mask_form_per_group(pkg, tctx, po, oracle, name):
    """A threshold's FIRST call on a window that holds another threshold's masks is served by the nine-cell form (the
    masks stay); a threshold that asks again takes the masks over (test_gpu_nbr_masks.py).  Per group, on a window bound
    anew for it: the same bits all three times, and the golden's at its bar."""
    g = golden()
    m, key = golden_map(g, name), "s1080"
    upload_scan(pkg, tctx, golden_scan(g, name, key))
    cfg1, cfg2 = pkg.spe_cfg(oope=pkg.OOPE_GMAPPING, pose_trig=1), pkg.spe_cfg(oope=pkg.OOPE_GMAPPING, gm_th=0.5, pose_trig=1)
    differ = 0
    for grp in RIM_GROUPS + INNER_GROUPS:
        poses = group_poses(g, name, key, grp)
        rebind(pkg, tctx, 0, m)
        assert masks(tctx, 0) == (0, 0)
        first = score(tctx, 0, cfg1, poses)
        assert masks(tctx, 0) == (1, 0)
        nine = score(tctx, 0, cfg2, poses)
        assert masks(tctx, 0) == (1, 0)
        for _ in range(2):
            np.testing.assert_array_equal(score(tctx, 0, cfg2, poses), nine, err_msg=grp)
            assert masks(tctx, 0) == (1, 0)
        np.testing.assert_allclose(nine, group_scores(g, name, key, grp, 0.5), rtol=1e-11, atol=1e-300, err_msg=grp)
        np.testing.assert_allclose(first, group_scores(g, name, key, grp, 0.1), rtol=1e-11, atol=1e-300, err_msg=grp)
        differ += int(not np.array_equal(first, nine))
    assert differ >= 4  # (the thresholds are told apart)
    # the same in the narrow kernels: every group's poses as one sequence of 161 (k_score_gmapping<K, true>) and of 2048
    # poses (<K, false>), each on a window bound anew
    seq, scan = all_poses(g, name, key), golden_scan(g, name, key)
    for count in (161, 2048):
        tiled = np.resize(seq, (count, 3))
        rebind(pkg, tctx, 0, m)
        score(tctx, 0, cfg1, tiled)
        assert masks(tctx, 0) == (1, 0)
        nine = score(tctx, 0, cfg2, tiled)
        for _ in range(2):
            np.testing.assert_array_equal(score(tctx, 0, cfg2, tiled), nine, err_msg="%d poses" % count)
        np.testing.assert_allclose(nine, oracle_scores(oracle, po, m, scan, tiled, gm_th=0.5), rtol=1e-12, atol=0)
    tctx.map_release(0)


@pytest.mark.parametrize("kw", [dict(gm_th=0.0), dict(gm_th=-2.0), dict(gm_window=0), dict(gm_window=2)],
                         ids=["th0", "th-2", "window0", "window2"])
@pytest.mark.parametrize("name", list(MAPS))
def test_odd_thresholds_and_the_generic_window_loop_vs_oracle(pkg, tctx, po, oracle, name, kw):
    """fullness_th <= 0: free and never-observed cells are full, every mask all ones, the cells beyond the rim as well
    (they read as the prototype); window 0 and 2: the (2 w + 1)^2 loop -- the out_<side> groups put its cells two cells
    across each rim.  On a window whose masks exist (a window-1 scorer at 0.1 ran before)."""
    g = golden()
    m = golden_map(g, name)
    rebind(pkg, tctx, 0, m)
    for key in ("s65", "s1080"):
        scan, seq = golden_scan(g, name, key), all_poses(g, name, key)
        upload_scan(pkg, tctx, scan)
        score(tctx, 0, pkg.spe_cfg(oope=pkg.OOPE_GMAPPING, pose_trig=1), seq)
        assert masks(tctx, 0) == (1, 0)
        where = group_slices(g)
        for _ in range(2):  # (the second call: a threshold that stays takes the masks over)
            got = score(tctx, 0, pkg.spe_cfg(oope=pkg.OOPE_GMAPPING, pose_trig=1, **kw), seq)
            want = oracle_scores(oracle, po, m, scan, seq, **kw)
            np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
            assert masks(tctx, 0) == (1, 0)
        for count in (161, 2048):  # ... and in k_score_gmapping<K, true> and <K, false>: the same bits as the wide kernel's
            tiled = np.resize(seq, (count, 3))
            more = score(tctx, 0, pkg.spe_cfg(oope=pkg.OOPE_GMAPPING, pose_trig=1, **kw), tiled)
            np.testing.assert_allclose(more, oracle_scores(oracle, po, m, scan, tiled, **kw), rtol=1e-12, atol=0)
            np.testing.assert_array_equal(more[:len(seq)], got)
        if kw.get("gm_window") == 2 and key == "s1080":
            plain = oracle_scores(oracle, po, m, scan, seq)
            for side in ("left", "right", "bottom", "top"):  # two cells outside: only the wider window reaches in
                assert (want[where["out_" + side]] != plain[where["out_" + side]]).any(), side
    tctx.map_release(0)


# ======================================================================================================================
# Section 1c: the masks after every kind of writer
def scores_of_fresh_upload(pkg, fresh, tctx, map_id, scan, cfg, poses):
    """the window of `tctx`'s map downloaded and uploaded to another context as new: its masks come from one pass"""
    info = tctx.map_info(map_id)
    w, h = info["width"], info["height"]
    cells = tctx.map_download_window(map_id, 0, 0, w, h, 3)
    try:
        fresh.map_release(1)
    except pkg.SlamHipError:
        pass
    fresh.map_bind(1, pkg.CELL_GMAPPING, w, h, info["origin"], info["scale"], UNKNOWN)
    fresh.map_upload_window(1, 0, 0, cells)
    upload_scan(pkg, fresh, scan)
    out = score(fresh, 1, cfg, poses)
    fresh.map_release(1)
    return out, cells


def aimed(origin, robot, targets):
    """pose and beams from the centre of internal cell `robot` to the centres of the internal cells `targets`"""
    pose = np.array([(robot[0] - origin[0] + 0.5) * SCALE, (robot[1] - origin[1] + 0.5) * SCALE, 0.0])
    d = np.asarray(targets, dtype=np.float64) - np.asarray(robot, dtype=np.float64)
    return pose, np.hypot(d[:, 0], d[:, 1]) * SCALE, np.arctan2(d[:, 1], d[:, 0])


def rim_writes(W, H):
    """per rim and corner: (robot cell two cells inside, rim cells to hit, the cell beside the robot that is first hit
    and then worn down by twelve beams that pass through it)"""
    lo, hx, hy, mx, my = 2, W - 3, H - 3, W // 2 + 5, H // 2 - 4
    out = {}
    for where, (rx, ry) in {"left": (lo, my), "right": (hx, my), "bottom": (mx, lo), "top": (mx, hy),
                            "bl": (lo, lo), "br": (hx, lo), "tl": (lo, hy), "tr": (hx, hy)}.items():
        ex = 0 if rx == lo else (W - 1 if rx == hx else None)
        ey = 0 if ry == lo else (H - 1 if ry == hy else None)
        if ex is not None and ey is not None:
            hits = [(ex, ey), (ex, ry), (rx, ey), (ex, ey + (1 if ey == 0 else -1)), (ex + (1 if ex == 0 else -1), ey)]
        elif ex is not None:
            hits = [(ex, ry + d) for d in (-2, -1, 0, 1, 2)]
        else:
            hits = [(rx + d, ey) for d in (-2, -1, 0, 1, 2)]
        sx = 1 if rx < W // 2 else -1
        out[where] = ((rx, ry), hits, (rx + 2 * sx, ry), (rx + 5 * sx, ry))
    return out


@pytest.mark.parametrize("path", list(K6_PATHS))
@pytest.mark.parametrize("name", list(MAPS))
def test_masks_follow_k6_on_every_rim_and_corner(pkg, tctx, fresh, name, path):
    """slamhip_map_append_scan with the GMapping rule, every pipeline: from two cells inside each rim and each corner, hits
    on the rim's (the corner's) cells -- never-observed or free cells become full -- and twelve beams through a cell
    that was made full just before -- it becomes free again.  After every append the masks are the ones the occupancies
    give, at the end the scores are those of a fresh upload of the same cells, and the download shows that cells did
    change sides on each rim, in each corner, and both ways."""
    g = golden()
    m, scan = golden_map(g, name), golden_scan(g, name, "s1080")
    W, H = MAPS[name]
    cfg = pkg.spe_cfg(oope=pkg.OOPE_GMAPPING, pose_trig=1)
    seq = all_poses(g, name, "s1080")
    rebind(pkg, tctx, 0, m)
    tctx.set_option(pkg.OPT_K6_PATH, K6_PATHS[path])
    try:
        upload_scan(pkg, tctx, scan)
        base = score(tctx, 0, cfg, seq)
        assert masks(tctx, 0) == (1, 0)
        before = m.payload[..., 0] >= 0.1
        worn = []
        for where, (robot, hits, beside, beyond) in rim_writes(W, H).items():
            pose, rng, ang = aimed(m.origin, robot, hits + [beside])
            c, s = pkg.beam_trig(ang)
            assert tctx.map_append_scan(0, pkg.RULE_GMAPPING, pose, rng, c, s, None) > 0
            assert masks(tctx, 0) == (1, 0), "%s: hits" % where
            pose, rng, ang = aimed(m.origin, robot, [beyond] * 12)
            c, s = pkg.beam_trig(ang)
            assert tctx.map_append_scan(0, pkg.RULE_GMAPPING, pose, rng, c, s, None) > 0
            assert masks(tctx, 0) == (1, 0), "%s: wear" % where
            worn.append(beside)
        upload_scan(pkg, tctx, scan)
        got = score(tctx, 0, cfg, seq)
        want, cells = scores_of_fresh_upload(pkg, fresh, tctx, 0, scan, cfg, seq)
        np.testing.assert_array_equal(got, want)
        assert not np.array_equal(got, base)
        after = cells[..., 0] >= 0.1
        flipped = before != after
        assert flipped[:, 0].any() and flipped[:, W - 1].any() and flipped[0].any() and flipped[H - 1].any()
        for x, y in ((0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)):
            assert after[y, x] and flipped[max(y - 1, 0):y + 2, max(x - 1, 0):x + 2].sum() >= 2, (x, y)
        assert (after & ~before).sum() >= 20 and (before & ~after).sum() >= 1  # free -> full, and full -> free
        for x, y in worn:  # made full by the first append of its placement, free again by the second
            assert not after[y, x] and 0 <= cells[y, x, 0] < 0.1, (x, y)
    finally:
        tctx.set_option(pkg.OPT_K6_PATH, 0)
        tctx.map_release(0)


@pytest.mark.parametrize("name", list(MAPS))
def test_masks_follow_the_dirty_log_and_partial_uploads(pkg, tctx, fresh, name):
    g = golden()
    m, scan = golden_map(g, name), golden_scan(g, name, "s1080")
    W, H = MAPS[name]
    cfg = pkg.spe_cfg(oope=pkg.OOPE_GMAPPING, pose_trig=1)
    seq = all_poses(g, name, "s1080")
    rebind(pkg, tctx, 0, m)
    upload_scan(pkg, tctx, scan)
    last = score(tctx, 0, cfg, seq)
    assert masks(tctx, 0) == (1, 0)

    def check(what, changed=True):
        nonlocal last
        assert masks(tctx, 0) == (1, 0), what
        got = score(tctx, 0, cfg, seq)
        want, cells = scores_of_fresh_upload(pkg, fresh, tctx, 0, scan, cfg, seq)
        np.testing.assert_array_equal(got, want, err_msg=what)
        assert np.array_equal(got, last) != changed, what
        last = got
        return cells

    # map_apply_dirty: the four corners, one cell of each rim, inner cells -- full -> free, then free -> full
    xs, ys = (6, W // 2 + 2, W - 8), (5, H // 2 + 1, H - 7)
    full_cells = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (0, ys[1]), (W - 1, ys[1]), (xs[1], 0), (xs[1], H - 1),
                  (3, ys[1]), (xs[1], 3), (W // 2 - 9, H // 2 + 5)]
    occ = m.payload[..., 0]
    assert all(occ[y, x] >= 0.1 for x, y in full_cells)
    free_cells = [(x + dx, y + dy) for x, y in full_cells[4:8] for dx, dy in ((2, 0), (0, 2), (-2, 0), (0, -2))
                  if 0 <= x + dx < W and 0 <= y + dy < H and (x + dx in (0, W - 1) or y + dy in (0, H - 1))]
    free_cells += [(1, 1), (W - 2, H - 2), (W // 2, H // 2 + 7)]
    assert len(free_cells) >= 11 and all(occ[y, x] < 0.1 for x, y in free_cells)
    tctx.map_apply_dirty(0, full_cells, np.tile([0.0, 0.0, 0.0], (len(full_cells), 1)))
    cells = check("dirty log: full -> free")
    assert all(cells[y, x, 0] == 0.0 for x, y in full_cells)
    vals = np.array([[0.9, (x - m.origin[0] + 0.21) * SCALE, (y - m.origin[1] + 0.83) * SCALE] for x, y in free_cells])
    tctx.map_apply_dirty(0, free_cells, vals)
    cells = check("dirty log: free -> full")
    assert all(cells[y, x, 0] == 0.9 for x, y in free_cells)
    tctx.map_apply_dirty(0, full_cells, np.array([m.payload[y, x] for x, y in full_cells]))
    check("dirty log: back")

    # map_upload_window: a patch against each rim in turn, then one row and one column
    r = np.random.default_rng(31)

    def patch(h, w):
        p = np.zeros((h, w, 3))
        p[..., 0] = r.choice([0.0, 0.05, 0.1, 0.8, -1.0], (h, w))
        p[..., 1:] = r.uniform(-4, 4, (h, w, 2))
        return p

    for what, (x0, y0, w, h) in {"left": (0, ys[1] - 5, 7, 11), "right": (W - 7, ys[0] - 3, 7, 11),
                                 "bottom": (xs[1] - 5, 0, 11, 7), "top": (xs[2] - 6, H - 7, 11, 7),
                                 "one row": (0, ys[2], W, 1), "one column": (xs[0], 0, 1, H),
                                 "corner": (W - 5, H - 3, 5, 3)}.items():
        tctx.map_upload_window(0, x0, y0, patch(h, w))
        check("upload: " + what)
    tctx.map_release(0)


def test_masks_of_an_oblong_window_that_grows_in_one_direction(pkg, tctx, fresh):
    """slamhip_map_set_auto_grow from 21 x 13 cells with origin (3, 10): a scan that reaches out in +x only, then one in -y
    only.  The masks are dropped with the old window and derived again by the next scorer call; the scores are those of a
    fresh upload of the grown window."""
    g = golden()
    scan = golden_scan(g, "wide", "s257")
    cfg = pkg.spe_cfg(oope=pkg.OOPE_GMAPPING, pose_trig=1)
    try:
        tctx.map_release(2)
    except pkg.SlamHipError:
        pass
    tctx.map_bind(2, pkg.CELL_GMAPPING, 21, 13, (3, 10), SCALE, UNKNOWN)
    tctx.map_set_auto_grow(2, True)
    pose = np.array([0.75, -0.35, 0.0])
    r = np.random.default_rng(5)
    poses = pose + r.uniform(-0.2, 0.2, (24, 3))
    ang = np.deg2rad(np.linspace(-5.0, 5.0, 41))  # (a narrow fan: 4 m along it are 0.35 m across)
    c, s = pkg.beam_trig(ang)
    tctx.map_append_scan(2, pkg.RULE_GMAPPING, pose, r.uniform(0.3, 0.8, ang.size), c, s, None)  # stays inside
    upload_scan(pkg, tctx, scan)
    score(tctx, 2, cfg, poses)
    assert masks(tctx, 2) == (1, 0) and tctx.map_info(2)["times_grown"] == 0
    seen = []
    for heading, lo, hi in ((0.0, 2.5, 4.0), (-np.pi / 2, 1.5, 3.0)):  # +x only, then -y only
        before = tctx.map_info(2)
        tctx.map_append_scan(2, pkg.RULE_GMAPPING, pose + [0, 0, heading], r.uniform(lo, hi, ang.size), c, s, None)
        info = tctx.map_info(2)
        assert info["times_grown"] == before["times_grown"] + 1 and masks(tctx, 2)[0] == 0
        seen.append((info["width"] - before["width"], info["height"] - before["height"],
                     info["origin"][0] - before["origin"][0], info["origin"][1] - before["origin"][1]))
        upload_scan(pkg, tctx, scan)
        got = score(tctx, 2, cfg, poses)
        assert masks(tctx, 2) == (1, 0)
        want, _ = scores_of_fresh_upload(pkg, fresh, tctx, 2, scan, cfg, poses)
        np.testing.assert_array_equal(got, want)
        assert got.any()
    (dw0, dh0, dox0, doy0), (dw1, dh1, dox1, doy1) = seen
    assert dw0 > 0 and dh0 == 0 and dox0 == 0 and doy0 == 0      # +x: wider, the origin stays
    assert dw1 == 0 and dh1 > 0 and dox1 == 0 and doy1 == dh1    # -y: higher, origin_y moves with it
    info = tctx.map_info(2)
    assert info["width"] != info["height"] and info["origin"][0] != info["origin"][1]
    tctx.map_release(2)


# ======================================================================================================================
# Section 1d: matchers and the filter
CHAINS = [(2, 0), (2, 256), (2, 512), (2, 1024), (1, 256), (1, 512), (1, 1024), (0, 0)]


@pytest.mark.parametrize("name", list(MAPS))
def test_hill_climbing_across_the_rims_in_every_chain_mode(pkg, ctx, po, oracle, name):
    """HC(6, 0.1, 0.1) from a pose whose first accepted poses throw beams on and across two rims: the co-resident launch,
    the chain of kernels (each at 256 / 512 / 1024 threads) and the host-driven batches against the golden's trace
    (1e-11) and against the oracle's accept loop."""
    g = golden()
    m, s3 = golden_map(g, name), hc_scan(g, name)
    rebind(pkg, ctx, 0, m)
    upload_scan(pkg, ctx, po.ScanData(s3.range, s3.angle, pkg.scan_weights("even", s3.range, s3.angle)))
    init, want = g[name + "_hc_init"], trace(g, name + "_hc6_skip3_")
    b = oracle.process_scan(oracle.enumerator(po.SM_HC, [6, 0.1, 0.1]), m, s3, po.make_cfg(oope=po.OOPE_GMAPPING), init,
                            cache=po.Oracle.new_gm_cache())
    for pose_trig in (1, 0):
        for mode, threads in CHAINS:
            mt = pkg.Matcher(ctx, "HC", pkg.spe_cfg(oope=pkg.OOPE_GMAPPING, pose_trig=pose_trig), [6, 0.1, 0.1])
            mt.set_device_chain(mode, threads)
            ctx.gm_cache_reset()
            t = mt.process_scan(0, init, trace=True)
            what = "pose_trig %d, chain mode %d, %d threads" % (pose_trig, mode, threads)
            assert t["n_calls"] == want["n_calls"] == b["n_calls"], what
            np.testing.assert_array_equal(t["accepted"], b["accepted"], err_msg=what)
            if pose_trig == 1:
                assert_trace_equal(t, want, exact_scores=False, rtol=1e-11)
                np.testing.assert_allclose(t["scores"], b["scores"], rtol=1e-12, atol=0, err_msg=what)
            else:
                np.testing.assert_allclose(t["scores"], want["scores"], rtol=1e-11, atol=1e-300, err_msg=what)
                np.testing.assert_allclose(t["poses"], want["poses"], rtol=0, atol=1e-12, err_msg=what)
            mt.close()
    ctx.map_release(0)


@pytest.mark.parametrize("name", list(MAPS))
def test_hill_climbing_exact_mode_vs_golden_trace_for_trace(pkg, ctx, po, variant, name):
    g = golden()
    m, s3 = golden_map(g, name), hc_scan(g, name)
    rebind(pkg, ctx, 0, m)
    upload_scan(pkg, ctx, po.ScanData(s3.range, s3.angle, pkg.scan_weights("even", s3.range, s3.angle)), exact=True)
    cfg = pkg.spe_cfg(oope=pkg.OOPE_GMAPPING, sum_order=pkg.SUM_SEQUENTIAL, pose_trig=pkg.POSE_TRIG_RAW_EXACT)
    ctx.gm_cache_reset()
    mt = pkg.Matcher(ctx, "HC", cfg, [6, 0.1, 0.1])
    assert_trace_equal(mt.process_scan(0, g[name + "_hc_init"], trace=True), trace(g, name + "_hc6_skip3_"))
    mt.close()
    ctx.map_release(0)


def run_filter(pkg, ctx, g, pose_trig, map_id=5):
    n = len(g["pf_seeds"])
    pf = pkg.GmappingFilter(ctx, pkg.gmapping_params(gp8=g["pf_gp"], skip_rate=3, pose_trig=pose_trig), n, g["pf_seeds"])
    out = []
    for k in range(int(g["pf_n_steps"])):
        st = pf_step(g, k)
        res, _idx = pf.step(map_id, st["range"], st["angle"], None, st["delta"], 7 + k)
        poses, w, ms = pf.state()
        out.append((res, poses, w, ms, pf.stats()["scorer_calls"]))
    pf.close()
    return out


@pytest.mark.parametrize("pose_trig", [1, 0, 2])
def test_filter_steps_on_the_wide_map_vs_golden(pkg, ctx, pose_trig):
    """three GmappingParticleFilter steps of the compiled reference near (+1.3, -1.2) m of the 77 x 45 window, at the bars
    of test_gmapping_filter_vs_reference_golden; POSE_TRIG_RAW_EXACT (2) bit for bit"""
    if pose_trig == 2 and pkg.libm_variant() < 0:
        pytest.skip("this host's libm is neither build of glibc's sin / cos / exp: no exact modes here")
    g = golden()
    rebind(pkg, ctx, 5, golden_map(g, "wide"))
    for k, (res, poses, w, ms, _calls) in enumerate(run_filter(pkg, ctx, g, pose_trig)):
        st = pf_step(g, k)
        assert res == st["resampled"], k
        np.testing.assert_array_equal(ms, st["master"])
        if pose_trig == 2:
            np.testing.assert_array_equal(poses, st["poses"])
            np.testing.assert_array_equal(w, st["weights"])
        else:
            np.testing.assert_allclose(poses, st["poses"], rtol=0, atol=1e-10)
            np.testing.assert_allclose(w, st["weights"], rtol=1e-9, atol=0)
    ctx.map_release(5)


def test_filter_chains_equal_the_lock_step_jobs_on_the_wide_map(pkg):
    """SLAMHIP_OPT_FILTER_CHAINS 1 against 0: poses, weights, scorer calls and resampling decisions bit for bit"""
    g = golden()
    runs = []
    for chains in (1, 0):
        c = pkg.Context(0)
        try:
            c.set_option(pkg.OPT_FILTER_CHAINS, chains)
            c.upload_map(5, golden_map(g, "wide"))
            runs.append(run_filter(pkg, c, g, 0))
        finally:
            c.close()
    for (res_a, poses_a, w_a, ms_a, calls_a), (res_b, poses_b, w_b, ms_b, calls_b) in zip(*runs):
        assert res_a == res_b and calls_a == calls_b
        np.testing.assert_array_equal(poses_a, poses_b)
        np.testing.assert_array_equal(w_a, w_b)
        np.testing.assert_array_equal(ms_a, ms_b)


# ======================================================================================================================
# Section 2: tile pools -- seams and oblong extents
# A pool's first extent is extent_tiles x extent_tiles tiles of 128 x 128 cells around the world origin: external cells
# -64 .. 63 for one tile.  It grows by whole tiles on the side a scan leaves it, so every seam lies at an external
# coordinate 64 + 128 k, and the local coordinate of external cell e is (e + 64) mod 128.
PSCALE = 0.05


def local(e):
    return (e + 64) % TILE


def at_cell(cell, frac):
    """world point in external cell `cell` at `frac` of its extent"""
    return ((cell[0] + frac[0]) * PSCALE, (cell[1] + frac[1]) * PSCALE)


def beams_to(pose, points):
    p = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    d = p - np.asarray(pose[:2])
    return np.hypot(d[:, 0], d[:, 1]), np.arctan2(d[:, 1], d[:, 0]) - pose[2]


HIT_FRAC, END_FRAC = (0.7, 0.35), (0.4, 0.8)
NO_FILL = {(64, 63), (318, 20), (63, -64), (20, -319)}  # hit cells on or next to an extent's own rim


class Pool:
    """a 1-particle filter with per-particle maps (with one particle no OOPE cache is shared between particles) next to
    a context that gets the same cells as ONE dense window"""

    def __init__(self, pkg, chains, ancestor, extent_tiles):
        self.pkg = pkg
        self.ctx, self.dense = pkg.Context(0, testing=True), pkg.Context(0)
        self.pf = None
        for c in (self.ctx, self.dense):
            c.set_option(pkg.OPT_FILTER_CHAINS, chains)
        w, h, origin, pose = ancestor
        self.ctx.map_bind(4, pkg.CELL_GMAPPING, w, h, origin, PSCALE, UNKNOWN)
        ang = np.deg2rad(np.linspace(-170.0, 170.0, 90))
        c, s = pkg.beam_trig(ang)
        r = np.random.default_rng(3).uniform(0.3, 0.3 + 0.4 * min(w, h) * PSCALE * 0.5, ang.size)
        assert self.ctx.map_append_scan(4, pkg.RULE_GMAPPING, pose, r, c, s, None) > 100
        self.ancestor_scan, self.asked = (pose, r, ang), False
        # (no gate and no pose noise: the first pose scored is the pose that was set)
        self.params = pkg.gmapping_params(gp8=[0.0] * 8)
        self.pf = pkg.GmappingFilter(self.ctx, self.params, 1, np.array([77], dtype=np.uint32))
        self.pf.enable_particle_maps(4, extent_tiles=extent_tiles, pool_tiles=48)

    def close(self):
        if self.pf is not None:
            self.pf.close()
        self.ctx.close()
        self.dense.close()

    def append(self, pose, rng, ang):
        nu = self.pf.particle_maps_append([0], np.asarray(pose, dtype=np.float64).reshape(1, 3), rng, ang)
        (valid, bad), bad_states = pool_masks(self.ctx, self.pf)
        # (the masks exist since ask_first(), and every append -- the ones that make the extent grow included -- has to
        # keep them: valid and true)
        assert self.asked and (valid, bad) == (1, 0) and bad_states == 0, "after an append"
        return nu

    def ask_first(self, box):
        """a match on the ancestor's own scan before anything grows: the masks are derived, so that the appends that follow
        -- table reallocation, origin shift, fresh tiles -- meet valid masks"""
        pose, r, ang = self.ancestor_scan
        self.twin(box, pose, r, ang)
        assert self.asked

    def draw(self, pose, cells):
        """one hit in each external cell of `cells`, at HIT_FRAC of it, from `pose`"""
        rng, ang = beams_to(pose, [at_cell(c, HIT_FRAC) for c in cells])
        assert self.append(pose, rng, ang) > 0

    def tiles(self):
        blob = self.pf.export_particle_map(0)
        n = int(np.frombuffer(blob[:8].tobytes(), np.int64)[0])
        ent = np.frombuffer(blob[8:8 + 16 * n].tobytes(), np.int32).reshape(n, 4)
        return set(zip(ent[:, 0].tolist(), ent[:, 1].tolist()))

    def cells(self, box):
        x0, y0, x1, y1 = box
        return self.pf.particle_map(0, x0, y0, x1 - x0, y1 - y0)[0]

    def twin(self, box, pose, rng, ang):
        """the matched pose and raw weight of the particle through its tile table, and of a filter of the same seed on the
        same cells uploaded as a dense window with the same external geometry: bit for bit (both take the smallest squared
        distance over the same full cells, one exp, the canonical sum).  The cells are taken BEFORE the match: a particle
        with a map of its own appends the scan to it from the matched pose (gmapping_world.h:93-97).  Returns them."""
        pkg, x0, y0, x1, y1 = self.pkg, *box
        cells = self.cells(box)
        self.pf.set(np.asarray(pose, dtype=np.float64).reshape(1, 3), np.ones(1))
        raw_t = self.pf.predict_match(4, rng, ang, None, np.zeros(3))
        pose_t = self.pf.state()[0]
        assert self.pf.stats()["scorer_calls"] > 6
        (valid, bad), bad_states = pool_masks(self.ctx, self.pf)
        assert (valid, bad) == (1, 0) and bad_states == 0
        self.asked = True
        self.dense.map_bind(1, pkg.CELL_GMAPPING, x1 - x0, y1 - y0, (-x0, -y0), PSCALE, UNKNOWN)
        self.dense.map_upload_window(1, 0, 0, cells)
        twin = pkg.GmappingFilter(self.dense, self.params, 1, np.array([77], dtype=np.uint32))
        try:
            twin.set(np.asarray(pose, dtype=np.float64).reshape(1, 3), np.ones(1))
            raw_d = twin.predict_match(1, rng, ang, None, np.zeros(3))
            pose_d = twin.state()[0]
        finally:
            twin.close()
            self.dense.map_release(1)
        np.testing.assert_array_equal(pose_t, pose_d)
        np.testing.assert_array_equal(raw_t, raw_d)
        assert raw_t[0] > 0 and np.isfinite(raw_t[0])
        return cells


def winners(cells, box, ends):
    """per end point (world): its external end cell and the external cell of the full cell that wins the minimum of its
    3 x 3 window (None: no full cell), in numpy from the downloaded cells"""
    x0, y0, x1, y1 = box
    out = []
    for ex, ey in ends:
        cx, cy = int(np.floor(ex / PSCALE)), int(np.floor(ey / PSCALE))
        best, win = np.inf, None
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                ix, iy = cx + dx - x0, cy + dy - y0
                if 0 <= ix < x1 - x0 and 0 <= iy < y1 - y0 and not cells[iy, ix, 0] < 0.1:
                    d2 = (cells[iy, ix, 1] - ex) ** 2 + (cells[iy, ix, 2] - ey) ** 2
                    if d2 < best:
                        best, win = d2, (cx + dx, cy + dy)
        out.append(((cx, cy), win))
    return out


def scored_scan(pose, ends, hit_cells, n_beams, seed):
    """`ends` first, then beams that end within 1.6 cells of the hit cells' centres (in turn), n_beams in all.  (Not around
    the hit cells on an extent's own rim, NO_FILL: the scan is appended to the particle's map after the match, and a beam
    beyond the extent would make it grow.)"""
    r = np.random.default_rng(seed)
    hit_cells = [c for c in hit_cells if c not in NO_FILL]
    fill = [at_cell(hit_cells[k % len(hit_cells)], (0.5, 0.5)) + r.uniform(-1.6, 1.6, 2) * PSCALE
            for k in range(n_beams - len(ends))]
    return beams_to(pose, list(ends) + fill)


def seam_cases(xseams, yseams, corners, row0, col0):
    """hit cells and aimed end cells around the given seams (external coordinate of the first cell behind the seam).
    Per vertical seam X: a hit behind the seam alone with the end cell in front of it (local x 127, the winner across),
    the reverse (local x 0), and hits on both sides (a wall across the seam); the same per horizontal seam.  Per corner
    (X, Y, which): ONE hit in the quadrant `which` and end cells in the other three -- the winner lies across the x seam,
    the y seam and the corner."""
    hits, ends, walls = [], [], []
    for k, X in enumerate(xseams):
        y = row0 + 13 * k
        hits += [(X, y), (X - 1, y + 4), (X - 1, y + 8), (X, y + 8)]
        ends += [(X - 1, y), (X, y + 4)]
        walls.append(((X - 1, y + 8), (X, y + 8)))
    for k, Y in enumerate(yseams):
        x = col0 + 13 * k
        hits += [(x, Y), (x + 4, Y - 1), (x + 8, Y - 1), (x + 8, Y)]
        ends += [(x, Y - 1), (x + 4, Y)]
        walls.append(((x + 8, Y - 1), (x + 8, Y)))
    for X, Y, which in corners:
        quad = {"A": (X - 1, Y - 1), "B": (X, Y - 1), "C": (X - 1, Y), "D": (X, Y)}
        hits.append(quad[which])
        ends += [c for q, c in quad.items() if q != which]
    return hits, ends, walls


def check_seams(pool, box, pose, hits, ends, walls, kinds, n_beams):
    """the downloaded map holds the walls across the seams, the aimed end cells are of every kind in `kinds` with the
    winning full cell in ANOTHER tile, and the tiled filter equals its dense twin"""
    rng, ang = scored_scan(pose, [at_cell(c, END_FRAC) for c in ends], hits, n_beams, 100 + n_beams)
    cells = pool.twin(box, pose, rng, ang)
    x0, y0 = box[:2]
    full = ~(cells[..., 0] < 0.1)
    for c in hits:
        assert full[c[1] - y0, c[0] - x0], c
    for a, b in walls:  # full cells on both sides of a seam, side by side
        assert full[a[1] - y0, a[0] - x0] and full[b[1] - y0, b[0] - x0]
        assert (local(a[0]), local(b[0])) == (127, 0) or (local(a[1]), local(b[1])) == (127, 0)
    seen = set()
    for (cx, cy), win in winners(cells, box, [at_cell(c, END_FRAC) for c in ends]):
        assert win is not None, (cx, cy)
        across = ((win[0] + 64) // TILE, (win[1] + 64) // TILE) != ((cx + 64) // TILE, (cy + 64) // TILE)
        lx, ly = local(cx), local(cy)
        if across:
            if lx in (0, 127) and ly in (0, 127):
                seen.add("corner%d_%d" % (lx, ly))
            if lx in (0, 127):
                seen.add("lx%d" % lx)
            if ly in (0, 127):
                seen.add("ly%d" % ly)
    assert set(kinds) <= seen, sorted(set(kinds) - seen)
    return cells


def fan(heading, lo, hi, n=41, half_deg=3.0, seed=1):
    r = np.random.default_rng(seed)
    return r.uniform(lo, hi, n), np.deg2rad(np.linspace(-half_deg, half_deg, n)) + heading


SMALL_ANCESTOR = (40, 24, (12, 9), np.array([0.31, 0.17, 0.2]))  # external cells -12 .. 27 x -9 .. 14


@pytest.mark.parametrize("n_beams", [360, 1080])
@pytest.mark.parametrize("chains", [1, 0])
def test_pool_grown_to_3x1_tiles_equals_its_dense_twin_on_the_seams(pkg, chains, n_beams):
    """extent_tiles = 1, grown toward +x only: 3 x 1 tiles, external x -64 .. 319, seams at x = 64 and 192; the origin
    stays (64, 64).  Both seams, the seam's cells on the extent's top rim, and the extent's own right rim."""
    pool = Pool(pkg, chains, SMALL_ANCESTOR, 1)
    try:
        pool.ask_first((-64, -64, 64, 64))
        pool.append(np.array([1.0, 0.3, 0.0]), *fan(0.0, 9.0, 12.0))
        box = (-64, -64, 320, 64)
        assert {t[0] for t in pool.tiles()} == {-64, 64, 192} and {t[1] for t in pool.tiles()} == {-64}
        hits, ends, walls = seam_cases([64, 192], [], [], row0=-30, col0=0)
        # the seam at x = 64 where it meets the extent's top rim (y = 63): the nine-cell form through the tables, its window
        # clamped against the tile rows; and a cell on the extent's right rim (x = 319)
        hits += [(64, 63), (318, 20)]
        ends += [(63, 63), (319, 20)]
        pool.draw(np.array([3.0, 0.2, 0.0]), [c for c in hits if c[0] < 150])
        pool.draw(np.array([9.4, 0.2, 0.0]), [c for c in hits if c[0] >= 150])
        pose = np.array([5.1, 0.9, -0.2])
        check_seams(pool, box, pose, hits, ends, walls, ["lx0", "lx127", "corner127_127"], n_beams)
    finally:
        pool.close()


@pytest.mark.parametrize("n_beams", [360, 1080])
@pytest.mark.parametrize("chains", [1, 0])
def test_pool_grown_to_1x3_tiles_equals_its_dense_twin_on_the_seams(pkg, chains, n_beams):
    """extent_tiles = 1, grown toward -y only: 1 x 3 tiles, external y -320 .. 63, seams at y = -64 and -192; the origin
    becomes (64, 320)."""
    pool = Pool(pkg, chains, SMALL_ANCESTOR, 1)
    try:
        pool.ask_first((-64, -64, 64, 64))
        pool.append(np.array([0.3, -1.0, 0.0]), *fan(-np.pi / 2, 9.0, 12.0))
        box = (-64, -320, 64, 64)
        assert {t[0] for t in pool.tiles()} == {-64} and {t[1] for t in pool.tiles()} == {-320, -192, -64}
        hits, ends, walls = seam_cases([], [-64, -192], [], row0=0, col0=-30)
        hits += [(63, -64), (20, -319)]  # the seam at y = -64 on the extent's right rim; the extent's bottom rim
        ends += [(63, -65), (20, -320)]
        pool.draw(np.array([0.2, -3.0, 0.0]), [c for c in hits if c[1] > -150])
        pool.draw(np.array([0.2, -9.4, 0.0]), [c for c in hits if c[1] <= -150])
        pose = np.array([0.9, -5.1, -1.2])
        check_seams(pool, box, pose, hits, ends, walls, ["ly0", "ly127", "corner127_127"], n_beams)
    finally:
        pool.close()


@pytest.mark.parametrize("n_beams", [360, 1080])
@pytest.mark.parametrize("chains", [1, 0])
def test_pool_grown_to_3x2_tiles_equals_its_dense_twin_on_seams_and_corners(pkg, chains, n_beams):
    """extent_tiles = 1, grown toward -x (two tiles) and +y (one): 3 x 2 tiles, external x -320 .. 63, y -64 .. 191, the
    origin becomes (320, 64).  Seams in both directions and two four-tile corners.  The tiles (-320, 64) and (-192, 64)
    lie under no scan's rectangle: they stay the shared never-observed tile, so the seams at y = 64 left of x = -64 and
    the corner at (-64, 64) have it on their far side.  Then the 2 x 2 block around that corner is filled."""
    pool = Pool(pkg, chains, SMALL_ANCESTOR, 1)
    try:
        pool.ask_first((-64, -64, 64, 64))
        pool.append(np.array([-1.0, 0.3, 0.0]), *fan(np.pi, 9.0, 12.0))
        pool.append(np.array([0.3, 1.0, 0.0]), *fan(np.pi / 2, 3.0, 5.0))
        box = (-320, -64, 64, 192)
        assert pool.tiles() == {(-320, -64), (-192, -64), (-64, -64), (-64, 64)}  # (what holds data: the rest is shared)
        hits, ends, walls = seam_cases([-64], [64], [(-64, 64, "D")], row0=-30, col0=8)
        # a hit in front of the seam y = 64 whose far side is the never-observed tile, end cells on both sides of it
        hits += [(-100, 63)]
        ends += [(-100, 64), (-99, 63)]
        pool.draw(np.array([0.3, 1.0, 0.0]), [c for c in hits if c[0] >= -64])
        pool.draw(np.array([-4.0, 1.5, 0.0]), [c for c in hits if c[0] < -64])
        assert (-192, 64) not in pool.tiles() and (-320, 64) not in pool.tiles()
        pose = np.array([-1.6, 2.3, 0.4])
        kinds = ["lx0", "lx127", "ly0", "ly127", "corner127_127", "corner0_127", "corner127_0"]
        check_seams(pool, box, pose, hits, ends, walls, kinds, n_beams)
        # the second corner, (-192, 64): ONE hit in its quadrant C, which makes the tile (-320, 64) the particle's own
        h2, e2, _ = seam_cases([-192], [], [(-192, 64, "C")], row0=-30, col0=0)
        pool.draw(np.array([-9.0, 2.0, 0.0]), h2)
        check_seams(pool, box, np.array([-8.1, 2.6, 2.9]), h2, e2, [], ["lx0", "lx127", "corner0_127", "corner0_0"], n_beams)
        # ... and the 2 x 2 block of full cells around the four-tile corner (-64, 64)
        block = [(-65, 63), (-64, 63), (-65, 64), (-64, 64)]
        pool.draw(np.array([-2.9, 2.9, 0.0]), block[:3])
        cells = check_seams(pool, box, pose + [0.07, -0.04, 0.03], hits + block[:3], [], walls, [], n_beams)
        assert all(not cells[y + 64, x + 320, 0] < 0.1 for x, y in block)
        assert sorted((local(x), local(y)) for x, y in block) == [(0, 0), (0, 127), (127, 0), (127, 127)]
    finally:
        pool.close()


@pytest.mark.parametrize("n_beams", [360, 1080])
@pytest.mark.parametrize("chains", [1, 0])
def test_pool_from_an_oblong_ancestor_equals_its_dense_twin_on_the_seams(pkg, chains, n_beams):
    """the 150 x 70 ancestor with origin (20, 50) of test_gpu_mapupdate_oblong.py, extent_tiles = 3 (the smallest square
    extent that takes it): external cells -192 .. 191, the ancestor across the seam at x = 64 and off the extent's middle."""
    pool = Pool(pkg, chains, (150, 70, (20, 50), np.array([2.15, -1.05, 0.4])), 3)
    try:
        box = (-192, -192, 192, 192)
        pool.ask_first(box)
        hits, ends, walls = seam_cases([64], [-64], [(64, -64, "A")], row0=-30, col0=20)
        pool.draw(np.array([2.15, -1.05, 0.0]), hits)
        pose = np.array([2.6, -2.2, 0.3])
        kinds = ["lx0", "lx127", "ly0", "ly127", "corner0_127", "corner127_0", "corner0_0"]
        check_seams(pool, box, pose, hits, ends, walls, kinds, n_beams)
    finally:
        pool.close()


# ---- duplicates that share tiles whose neighbours differ ---------------------------------------------------------------
ROOM = (-12.5, -2.0, 2.0, 6.0)  # x_min, x_max, y_min, y_max of its walls, metres: across the seams x = -9.6, x = -3.2, y = 3.2
SEAM_ANCESTOR = (40, 30, (62, -34))  # external cells -62 .. -23 x 34 .. 63: the room's corner at (-2, 2) m, inside the first tile
SEAM_GATE = 0.55                 # the ancestor holds what the first scan sees within 0.55 m: nothing beyond its window
SEAM_N, SEAM_SEED0, SEAM_STEPS = 4, 4700, 7
SEAM_BOX = (-320, -64, 64, 192)  # the 3 x 2-tile extent the scans make, external cells
SEAM_GP = [0.0, 0.3, 0.0, 0.12, 0.0, 0.0, 0.0, 0.0]  # wide pose noise: the weights diverge and the filter resamples


def seam_filter_scenario():
    """the ancestor's scan and the filter steps of a robot that walks through a 10.5 x 4 m room whose walls cross three
    tile seams, from next to the four-tile corner (-3.2, 3.2) m: (ancestor pose, range, angle), [(range, angle, delta)]"""
    ang = np.deg2rad(np.linspace(-179.0, 179.0, 1080))  # (0.8 cells apart on the far walls: every column of a seam is hit)

    def ranges(pose, seed):
        x, y, th = pose
        c, s = np.cos(th + ang), np.sin(th + ang)
        with np.errstate(divide="ignore"):
            tx = np.where(c > 0, (ROOM[1] - x) / c, np.where(c < 0, (ROOM[0] - x) / c, np.inf))
            ty = np.where(s > 0, (ROOM[3] - y) / s, np.where(s < 0, (ROOM[2] - y) / s, np.inf))
        return np.minimum(tx, ty) + np.random.RandomState(seed).randn(ang.size) * 0.004

    start = np.array([-2.43, 2.47, np.deg2rad(170.0)])
    deltas = [start, [-0.12, 0.05, 0.03], [-0.1, -0.06, -0.04], [-0.08, 0.07, 0.05], [-0.11, -0.03, -0.02],
              [-0.09, 0.04, 0.03], [-0.1, 0.02, -0.03], [-0.07, -0.05, 0.04], [-0.12, 0.03, 0.02]][:SEAM_STEPS]  # westwards
    steps, true = [], np.zeros(3)
    for k, d in enumerate(deltas):
        true = true + np.asarray(d)
        assert ROOM[0] + 0.3 < true[0] < ROOM[1] - 0.3 and ROOM[2] + 0.3 < true[1] < ROOM[3] - 0.3  # (inside the room)
        steps.append((ranges(true, 50 + k), ang, np.asarray(d, dtype=np.float64)))
    return (start, ranges(start, 49), ang), steps


def seam_filter_oracle(oracle, n, seed0):
    """the oracle's filter with a dense map per particle over SEAM_BOX, the ancestor's scan in it"""
    import pyoracle as po
    from pyoracle_mapupdate import RULE_GMAPPING, append_scan_ex, gmapping_enable_particle_maps
    (anc_pose, anc_r, anc_a), steps = seam_filter_scenario()
    x0, y0, x1, y1 = SEAM_BOX
    m = po.GridMapData(po.CELL_GMAPPING, np.tile(UNKNOWN, (y1 - y0, x1 - x0, 1)).astype(np.float64), (-x0, -y0), PSCALE,
                       UNKNOWN)
    aux = np.zeros((y1 - y0, x1 - x0, 2))
    append_scan_ex(oracle, m, aux, RULE_GMAPPING, anc_pose, anc_r, anc_a, max_range=SEAM_GATE)
    seeds = np.arange(seed0, seed0 + n, dtype=np.uint32)
    opf = oracle.gmapping_create(n, SEAM_GP, seeds, skip_rate=3)
    gmapping_enable_particle_maps(oracle, opf, m, aux)
    return m, opf, seeds, (anc_pose, anc_r, anc_a), steps


def test_resampled_duplicates_share_tiles_across_seams_vs_oracle(pkg, oracle):
    """Four particles with maps of their own in a pool that their first scan grows from one tile to 3 x 2.  After a
    resampling the duplicates share every tile; the next step each appends its scan from another pose, so tiles are
    cloned on one side of a seam while the tile on the other side is still shared -- a tile's masks know the cells of
    their own tile only for exactly this.  Every step against the oracle's filter with a dense map per particle at the
    bars of test_gpu_particle_maps.py (poses 1e-10, weights 1e-9, occupancies and counters exact, obstacle means 1e-12);
    masks (1, 0) and settle states 0 after every step."""
    import pyoracle as po
    from pyoracle_mapupdate import gmapping_particle_map, gmapping_particle_map_append
    n, seed0 = SEAM_N, SEAM_SEED0
    m, opf, seeds, (anc_pose, anc_r, anc_a), steps = seam_filter_oracle(oracle, n, seed0)
    x0, y0, x1, y1 = SEAM_BOX
    ctx = pkg.Context(0, testing=True)
    pf = None

    def check(what):
        """every particle's map = the oracle's, masks and settle states true; returns the maps"""
        maps = []
        for i in range(n):
            got_p, got_a = pf.particle_map(i, x0, y0, x1 - x0, y1 - y0)
            want_p, want_a = gmapping_particle_map(oracle, opf, i)
            np.testing.assert_array_equal(got_p[..., 0], want_p[..., 0], err_msg="%s, particle %d" % (what, i))
            np.testing.assert_allclose(got_p[..., 1:], want_p[..., 1:], rtol=1e-12, atol=1e-14)
            np.testing.assert_array_equal(got_a, want_a)
            maps.append(got_p)
        (valid, bad), bad_states = pool_masks(ctx, pf)
        assert (valid, bad) == (1, 0) and bad_states == 0, what
        return maps

    def on_both_sides_of_every_seam(mask):
        return all(mask[:, X - 1 - x0].any() and mask[:, X - x0].any() for X in (-64, -192)) and \
            mask[64 - 1 - y0].any() and mask[64 - y0].any()

    try:
        aw, ah, aorigin = SEAM_ANCESTOR
        ctx.map_bind(4, pkg.CELL_GMAPPING, aw, ah, aorigin, PSCALE, UNKNOWN)
        c, s = pkg.beam_trig(anc_a)
        assert ctx.map_append_scan(4, pkg.RULE_GMAPPING, anc_pose, anc_r, c, s, None, max_range=SEAM_GATE) > 100
        pf = pkg.GmappingFilter(ctx, pkg.gmapping_params(gp8=SEAM_GP, skip_rate=3, pose_trig=1), n, seeds)
        pf.enable_particle_maps(4, extent_tiles=1, pool_tiles=16 + 24 * n)
        diverged = 0
        for it, (rng, ang, d) in enumerate(steps):
            extra = np.arange(9000 + 100 * it, 9000 + 100 * it + n, dtype=np.uint32)
            res, idx = pf.step(4, rng, ang, None, d, 7 + it)
            ores, oidx = opf.step(m, rng, ang, None, d, 7 + it, extra)
            poses, wts, ms = pf.state()
            oposes, owts, oms = opf.state()
            assert res == ores, it
            if res:
                np.testing.assert_array_equal(idx, oidx)
            np.testing.assert_array_equal(ms, oms)
            np.testing.assert_allclose(poses, oposes, rtol=0, atol=1e-10, err_msg="step %d" % it)
            np.testing.assert_allclose(wts, owts, rtol=1e-9, atol=0)
            maps = check("step %d" % it)
            if it == 0:  # the first scan made the extent 3 x 2 tiles; its walls are full cells on both sides of every seam
                blob = pf.export_particle_map(0)
                k = int(np.frombuffer(blob[:8].tobytes(), np.int64)[0])
                ent = np.frombuffer(blob[8:8 + 16 * k].tobytes(), np.int32).reshape(k, 4)
                assert sorted(set(ent[:, 0].tolist())) == [-320, -192, -64] and sorted(set(ent[:, 1].tolist())) == [-64, 64]
                assert on_both_sides_of_every_seam(~(maps[0][..., 0] < 0.1))
            if res:
                # the duplicates of one source share every tile (they hold the same pose and the same generator state, so
                # the filter alone would keep them equal): each appends the scan from a pose of its own -- tiles are cloned
                # where that particle writes, and stay shared with the others where it does not
                src = int(np.argmax(np.bincount(idx.astype(np.int64), minlength=n)))
                dup = [i for i in range(n) if idx[i] == src]
                assert len(dup) >= 2 and pf.particle_map_stats()["tiles_shared"] > 0
                assert not (maps[dup[0]] != maps[dup[1]]).any()
                own = poses + np.outer(np.arange(n), [0.07, -0.05, 0.02])
                cow = pf.particle_map_stats()["cow_copies"]
                cb, sb = pkg.beam_trig(ang)
                tr = po.ScanData(rng, ang, None, None, po.TRIG_CACHED, 0.0, 1.0, sb, cb)  # the device's own cos / sin,
                tr.angle = np.arange(len(rng), dtype=np.float64)                          # one table entry per beam
                nu = pf.particle_maps_append(np.arange(n), own, rng, ang)
                assert nu == sum(gmapping_particle_map_append(oracle, opf, m, i, own[i], rng, tr.angle, None, trig=tr)
                                 for i in range(n))
                maps = check("own poses after the resampling of step %d" % it)
                assert pf.particle_map_stats()["cow_copies"] > cow
                differ = (maps[dup[0]] != maps[dup[1]]).any(axis=2)
                assert on_both_sides_of_every_seam(differ) and not differ.all()
                diverged += 1
        assert diverged >= 1 and it > 3  # (and steps followed the divergence: their matches read the cloned tiles)
    finally:
        if pf is not None:
            pf.close()
        ctx.close()
