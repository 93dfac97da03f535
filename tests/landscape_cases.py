"""Shared by tests/golden/make_golden_landscapes.py, tests/test_oracle_landscapes.py and tests/test_gpu_landscapes.py:
DESIGNED score landscapes.  A one-beam scan of range 0 at heading 0, weight 1, factor 1, scores a pose with the value of
the cell under it: on a GridCell map under the discrepancy OIE the score is 1 - |c - 1|, which for c in [0.5, 1] is c bit
for bit (both subtractions are exact).  The map is a score table: the author writes the score sequence a matcher's walk
meets, and PoseEnumerationScanMatcher::process_scan (pose_enumeration_scan_matcher.h:31-77) -- `best < candidate`, ties
and NaN rejected -- decides.  The tables hold multiples of 2^-20 in [0.5, 1], np.nextafter neighbours and NaN where a
case says so.

A case (types.SimpleNamespace):
  name, kind ("BF" / "HC" / "MC"), params (the matcher's), payload [h, w], origin (array index = cell + origin), rng (the
  beam's range: 0, one hill-climbing case 1.0), inits (poses; one match each ON THE SAME matcher object, in this order),
  expect (per match dict(n_calls, accepted [call indices, 0 = the initial pose], win = the call whose pose is returned);
  None for MC, whose poses are drawn, not designed), shape ((nx, ny, nt), BF), settles ("device": the checked default mode
  decides every comparison of the sweep itself; "host": it may not -- two sums one ulp apart; BF).
The expected decision comes from the designed sequence through accept_loop below, nothing else.

Margin: moving a beam's end point by less than MARGIN (0.02 m) along x, along y or both never changes the cell VALUE it
reads -- the end point is at least 0.02 m from every cell edge, or the cells across the edge hold the same bits.  (A hill
climber halves its steps at the pose it ends in, so no position in a cell keeps 0.02 m from the edges for every
candidate; there the cells on the side the halved steps approach are equal by design, and the comparison ties whichever
cell is read.)  Asserted when a case is built.  The drawn poses of the MC cases cannot be placed: for them the margin is
DRAWN_MARGIN, held by the golden generator and the CPU suite on the oracle's trace."""
import hashlib
import os
import types

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "landscapes.npz")

S = 0.1            # cell size
Q = 2.0 ** -20     # the tables' quantum
PROTO = 0.5        # cells nobody wrote: MockGridCell's default
MARGIN = 0.02
DRAWN_MARGIN = 1e-7
NAN = float("nan")
BF_SIZES = ((1, 1, 1), (9, 7, 1), (8, 8, 1), (13, 5, 1), (33, 31, 1), (32, 32, 1), (41, 25, 1), (64, 32, 1), (683, 3, 1))
BF_BIG = (201, 201, 1)  # the search-space evaluator's shape: 40401 candidates, 40 blocks of the device arg-max
POSITIONS = (1, 63, 64, 65, 1023, 1024, 1025, 1026, 2048, 2049)
HC_LIMITS = (6, 60)
MC_PARAMS = [666666, 0.2, 0.1, 20, 100]


def q(k):
    """0.5 + k * 2^-20, k in [0, 2^19]"""
    k = np.asarray(k)
    assert np.all((k >= 0) & (k <= 1 << 19))
    return 0.5 + k * Q


def lvl(k):
    """steps of 2^-10 from 0.625"""
    return q((1 << 17) + (np.asarray(k) << 10))


def ulps(v, k):
    """v moved by k ulps (k may be negative)"""
    for _ in range(abs(k)):
        v = np.nextafter(v, 2.0 if k > 0 else 0.0)
    return v


def accept_loop(scores):
    """the reference's loop over a score sequence, scores[0] the initial pose's: (accepted call indices, the winner)"""
    best, win, accepted = scores[0], 0, [0]
    for e in range(1, len(scores)):
        if best < scores[e]:
            best, win = scores[e], e
            accepted.append(e)
    return accepted, win


# ---- geometry ----------------------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def cell_values(payload, origin, ex, ey):
    """the value under the end points (ex, ey): RegularSquaresGrid::world_to_cell = floor(x / scale), PROTO outside"""
    h, w = payload.shape
    ix = np.floor(np.asarray(ex) / S).astype(np.int64) + origin[0]
    iy = np.floor(np.asarray(ey) / S).astype(np.int64) + origin[1]
    inside = (ix >= 0) & (ix < w) & (iy >= 0) & (iy < h)
    return np.where(inside, payload[np.clip(iy, 0, h - 1), np.clip(ix, 0, w - 1)], PROTO)


def end_points(poses, rng):
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    return poses[:, 0] + rng * np.cos(poses[:, 2]), poses[:, 1] + rng * np.sin(poses[:, 2])


def margin_holds(payload, origin, poses, rng, margin=MARGIN):
    ex, ey = end_points(poses, rng)
    here = bits(cell_values(payload, origin, ex, ey))
    return all(np.array_equal(bits(cell_values(payload, origin, ex + dx, ey + dy)), here)
               for dx in (-margin, 0.0, margin) for dy in (-margin, 0.0, margin))


def cell_pose(origin, i, j, vx=0.5, vy=0.5, theta=0.0):
    """the pose at (vx, vy) cells inside the cell of array index (i, j)"""
    return np.array([(i - origin[0] + vx) * S, (j - origin[1] + vy) * S, theta])


# ---- brute force -------------------------------------------------------------------------------------------------------
def bf_axis(n, lo, below):
    """from, to, step of an axis of n values: `to` half a step clear of the accumulated value that ends the axis (x, y: the
    first value not below `to` is the last one handed out; theta: the values <= to)"""
    return [lo, lo + (n - (1.5 if below else 0.5)) * S if n > 1 or not below else lo, S]


def bf_params(shape):
    nx, ny, nt = shape
    return bf_axis(nx, S, True) + bf_axis(ny, 0.0, True) + bf_axis(nt, 0.0, False)


def bf_offsets(lo, to, step, below):
    out, v = [], lo
    while True:
        if not below and not v <= to:
            return out
        out.append(v)
        if below and not v < to:
            return out
        v += step


def bf_poses(shape, base):
    """candidates 1 .. nx * ny * nt of the walk around `base`: x fastest, then y, then theta; offsets accumulated as
    BruteForcePoseEnumerator::feedback accumulates them"""
    p = bf_params(shape)
    xs, ys, ts = bf_offsets(*p[0:3], True), bf_offsets(*p[3:6], True), bf_offsets(*p[6:9], False)
    assert (len(xs), len(ys), len(ts)) == tuple(shape)
    return np.array([(base[0] + x, base[1] + y, base[2] + t) for t in ts for y in ys for x in xs])


def bf_case(name, shape, init_score, cand, settles="device", second=None):
    """cand: the nx * ny scores of one theta slab in walk order (every slab repeats them: range 0).  The initial pose's
    cell lies in a column of its own left of the candidates; second = the score of a second initial pose one cell above
    it, matched after the first on the same matcher object."""
    nx, ny, nt = shape
    cand = np.asarray(cand, dtype=np.float64)
    assert cand.shape == (nx * ny,)
    payload = np.full((ny + 2, nx + 3), PROTO)
    payload[1:1 + ny, 2:2 + nx] = cand.reshape(ny, nx)
    payload[1, 1] = init_score
    origin = ((nx + 3) // 2, (ny + 2) // 2)
    inits, seqs = [cell_pose(origin, 1, 1)], [np.concatenate([[init_score], np.tile(cand, nt)])]
    if second is not None:
        payload[2, 1] = second
        inits.append(cell_pose(origin, 1, 2))
        seqs.append(np.concatenate([[second], np.tile(cand, nt)]))
    c = types.SimpleNamespace(name=name, kind="BF", params=bf_params(shape), payload=payload, origin=origin, rng=0.0,
                              inits=inits, shape=tuple(shape), settles=settles, expect=[])
    walk = bf_poses(shape, inits[0])  # (the base pose is latched at the first match)
    for init, seq in zip(inits, seqs):
        poses = np.concatenate([init[None], walk])
        assert np.array_equal(bits(cell_values(payload, origin, poses[:, 0], poses[:, 1])), bits(seq)), name
        assert margin_holds(payload, origin, poses, 0.0), name
        accepted, win = accept_loop(seq)
        c.expect.append(dict(n_calls=len(seq), accepted=accepted, win=win))
    check_values(c)
    return c


def check_values(c):
    v = c.payload[~np.isnan(c.payload)]
    assert np.all((v >= 0.5) & (v <= 1.0)), c.name


def background(n, seed):
    """n scores in [0.5, 0.75): multiples of 2^-20, the same for a seed for ever (RandomState's legacy stream)"""
    return q(np.random.RandomState(seed).randint(0, 1 << 18, n))


def size_tag(shape):
    return "n%d" % (shape[0] * shape[1] * shape[2])


def with_max(n, seed, at, value=0.9):
    s = background(n, seed)
    for e in at:
        s[e - 1] = value
    return s


def staircase_starts(n):
    """the first candidates of the plateaus: the plateaus in front of them end on lanes 62 / 63 of a wave, on waves and
    on blocks of the device arg-max"""
    return [e for e in [1, 64, 65, 129, 1024, 1025, 2049] + [1024 * k + 1 for k in range(3, 40)] if e <= n]


def bf_cases():
    out = []
    for shape in BF_SIZES:
        n, tag = shape[0] * shape[1], size_tag(shape)
        e = np.arange(1, n + 1)
        out.append(bf_case(tag + "-increasing", shape, q(0), q(e * 8)))
        out.append(bf_case(tag + "-decreasing", shape, q(1 << 19), q((1 << 19) - e * 8)))
        out.append(bf_case(tag + "-all_equal", shape, 0.75, np.full(n, 0.75)))
        starts = staircase_starts(n)
        out.append(bf_case(tag + "-staircase", shape, lvl(0), lvl(np.searchsorted(starts, e, side="right"))))
        out.append(bf_case(tag + "-initial_is_max", shape, 0.95, background(n, 7)))
        for p in sorted(set(POSITIONS + (n,))):
            if p <= n:
                out.append(bf_case("%s-max_at_%d" % (tag, p), shape, 0.6, with_max(n, 11, [p])))
        pairs = [(63, 64), (64, 65), (1023, 1024), (1024, 1025), (1, n)] + ([(517, min(1024 * ((n - 1) // 1024) + 2, n))] if n > 1025 else [])
        for a, b in pairs:
            if a < b <= n:
                out.append(bf_case("%s-tie_%d_%d" % (tag, a, b), shape, 0.6, with_max(n, 13, [a, b])))
    # the same maximum again one theta slab later: the first wins
    out.append(bf_case("n128-slab_tie_64_128", (8, 8, 2), 0.6, with_max(64, 17, [64])))
    out.append(bf_case("n2048-slab_tie_1024_2048", (32, 32, 2), 0.6, with_max(1024, 17, [1024])))
    out.append(bf_case("n3072-slab_tie_517_1541_2565", (32, 32, 3), 0.6, with_max(1024, 17, [517])))
    # 201 x 201: the tie in block 0 and in the last thread of the last (partial) block, a staircase under it
    n = BF_BIG[0] * BF_BIG[1]
    e = np.arange(1, n + 1)
    s = lvl(np.searchsorted(staircase_starts(n), e, side="right"))
    s[517 - 1] = s[n - 1] = 0.9
    out.append(bf_case("n40401-staircase_tie_517_40401", BF_BIG, lvl(0), s))
    # NaN
    for shape in ((13, 5, 1), (41, 25, 1), (683, 3, 1)):
        n, tag = shape[0] * shape[1], size_tag(shape)
        out.append(bf_case(tag + "-nan_initial", shape, NAN, background(n, 19)))
        out.append(bf_case(tag + "-nan_all_candidates", shape, 0.6, np.full(n, NAN)))
        out.append(bf_case(tag + "-nan_everything", shape, NAN, np.full(n, NAN)))
        for p in (65, 1025):
            if p <= n:
                s = with_max(n, 23, [p])
                s[p - 2] = NAN
                out.append(bf_case("%s-nan_in_front_of_max_at_%d" % (tag, p), shape, 0.6, s))
        for p in (63, 65, 1022, 1025):
            if p <= n:
                s = with_max(n, 29, [p])
                s[[k - 1 for k in (64, 1023, 1024) if k <= n]] = NAN
                out.append(bf_case("%s-nan_64_1023_1024_max_at_%d" % (tag, p), shape, 0.6, s))
        # NaN on the first lane of a wave or of a block (candidates 1, 65, 1025), the maximum behind it in the same wave: a
        # NaN that took part in the scan as a value would be kept by every fold behind it
        for p in (2, 66, 100, 1026, 1030):
            if p <= n:
                s = with_max(n, 43, [p])
                s[[k - 1 for k in (1, 65, 1025) if k <= n]] = NAN
                out.append(bf_case("%s-nan_1_65_1025_max_at_%d" % (tag, p), shape, 0.6, s))
    s = with_max(2049, 31, [1000, 2049])
    s[1024:2048] = NAN  # candidates 1025 .. 2048: all of block 1
    out.append(bf_case("n2049-nan_block_between_tie_1000_2049", (683, 3, 1), 0.6, s))
    # one ulp: the strict loop accepts the later, larger one; bit-equal values in two cells are a tie.  The pairs lie in one
    # wave, in two waves of one block (the hand-over through LDS carries the earlier one to the later), in two blocks, and
    # on both sides of a block boundary
    for shape, a, b in (((13, 5, 1), 10, 64), ((64, 32, 1), 10, 700), ((64, 32, 1), 100, 1500), ((64, 32, 1), 1024, 1025)):
        n, tag = shape[0] * shape[1], size_tag(shape)
        s = with_max(n, 37, [a])
        s[b - 1] = np.nextafter(0.9, 2.0)
        out.append(bf_case("%s-one_ulp_above_%d_at_%d" % (tag, a, b), shape, 0.6, s, settles="host"))
        s = with_max(n, 37, [b])
        s[a - 1] = np.nextafter(0.9, 2.0)
        out.append(bf_case("%s-one_ulp_below_%d_at_%d" % (tag, a, b), shape, 0.6, s, settles="host"))
        out.append(bf_case("%s-bit_equal_%d_%d" % (tag, a, b), shape, 0.6, with_max(n, 37, [a, b])))
    # a second match on the same matcher object: the candidates stay around the first base pose
    out.append(bf_case("n1025-second_match_initial_is_max", (41, 25, 1), 0.6, with_max(1025, 41, [1024]), second=0.95))
    out.append(bf_case("n1025-second_match_loses_to_1024", (41, 25, 1), 0.95, with_max(1025, 41, [1024]), second=0.8))
    return out


# ---- hill climbing -----------------------------------------------------------------------------------------------------
HC_W = 24  # the tables' side; origin (12, 12)
HC_ORIGIN = (12, 12)


def hc_walk(payload, origin, rng, init, limit, dt, dr):
    """HillClimbingScanMatcher over the table: (poses, scores) of every scorer call.  Round after round the six
    candidates +x -y +theta -x +y -theta around the pose the round began at; a round without an accept halves the steps
    (hill_climbing_scan_matcher.h:26-52, :83-116)."""
    def score(p):
        ex, ey = end_points(p, rng)
        return float(cell_values(payload, origin, ex, ey)[0])
    best = np.array(init, dtype=np.float64)
    best_s = score(best)
    poses, scores = [best.copy()], [best_s]
    action, failed, round_failed, base = 0, 0, True, None
    while failed < limit:
        if action >= 6:  # next() of a round that is used up: count it if it failed, begin the next one
            if round_failed:
                dt, dr, failed = dt * 0.5, dr * 0.5, failed + 1
            action, round_failed, base = 0, True, None
        if base is None:
            base = best.copy()
        p = base.copy()
        p[action % 3] += (-1.0 if action % 2 else 1.0) * (dr if action % 3 == 2 else dt)
        action += 1
        s = score(p)
        poses.append(p)
        scores.append(s)
        if best_s < s:
            best, best_s, round_failed = p, s, False
    return np.array(poses), np.array(scores)


def hc_case(name, payload, start, limit, rng=0.0, min_accepts=0):
    payload = np.ascontiguousarray(payload, dtype=np.float64)
    c = types.SimpleNamespace(name="%s-limit%d" % (name, limit), kind="HC", params=[limit, S, 0.1], payload=payload,
                              origin=HC_ORIGIN, rng=rng, inits=[np.asarray(start, dtype=np.float64)], shape=None, settles=None)
    poses, scores = hc_walk(payload, HC_ORIGIN, rng, c.inits[0], limit, S, 0.1)
    assert margin_holds(payload, HC_ORIGIN, poses, rng), c.name
    accepted, win = accept_loop(scores)
    assert len(accepted) - 1 >= min_accepts, (c.name, accepted)
    c.expect = [dict(n_calls=len(scores), accepted=accepted, win=win)]
    c.walk_scores = scores
    check_values(c)
    return c


def hc_tables():
    """(name, payload, start pose, beam range, the accepts the design promises at least)"""
    i, j = np.meshgrid(np.arange(HC_W), np.arange(HC_W))  # payload[j, i]
    i0 = j0 = 8
    at = lambda vx, vy, th=0.0, ii=i0, jj=j0: cell_pose(HC_ORIGIN, ii, jj, vx, vy, th)  # noqa: E731
    out = []
    # a ramp in +x up to a crest column, flat behind it: one accept a round, then failed rounds only
    out.append(("ramp_x_to_crest", lvl(np.clip(i, 2, 13)), at(0.75, 0.75), 0.0, 5))
    # nothing to climb at all: 1 + 6 * limit calls, the inert tail from the first round
    out.append(("plateau", np.full((HC_W, HC_W), lvl(5)), at(0.75, 0.75), 0.0, 0))
    # -y higher than +x, both higher than the base: two accepts in one round
    t = np.full((HC_W, HC_W), lvl(0))
    t[j0, i0], t[j0, i0 + 1] = lvl(1), lvl(2)
    t[j0 - 2:j0, i0:i0 + 2] = lvl(3)
    out.append(("two_accepts_in_a_round", t, at(0.75, 0.25), 0.0, 2))
    # a ridge along the diagonal, two cells wide, a flat top behind it: the accepts alternate between +x and +y
    c, r = i - i0, j - j0
    t = np.where((c >= 0) & (r >= 0) & (c - r >= 0) & (c - r <= 1) & (c + r < 6), lvl(1 + np.clip(c + r, 0, 6)), lvl(0))
    t = np.where((c >= 3) & (r >= 3), lvl(7), t)
    out.append(("diagonal_ridge", t, at(0.75, 0.75), 0.0, 6))
    # a NaN wall one cell in +x, the slope goes on in +y
    t = lvl(1 + np.clip(r, -1, 5))
    t = np.where(c == 1, NAN, t)
    out.append(("nan_wall_slope_in_y", t, at(0.25, 0.75), 0.0, 5))
    # the initial pose on a NaN cell: NaN is kept for ever, finite candidates in -x and -y are rejected
    t = np.full((HC_W, HC_W), lvl(3))
    t[j0:j0 + 2, i0:i0 + 2] = NAN
    out.append(("nan_initial", t, at(0.75, 0.75), 0.0, 0))
    # every +x cell one ulp above the one before, up to the crest
    t = np.zeros((HC_W, HC_W))
    for col in range(HC_W):
        t[:, col] = ulps(lvl(4), int(np.clip(col - i0, -1, 5)))
    out.append(("one_ulp_ramp", t, at(0.75, 0.75), 0.0, 5))
    # a beam of range 1 m: +-0.1 rad moves its end by about a cell in y; rows rise up to a crest, columns are alike.  The
    # rotation comes before +y in a round and reaches the same row: +theta is accepted, +y ties with it and is rejected
    out.append(("rotation_climbs", lvl(np.clip(j, 2, 13)), at(0.75, 0.77, 0.0, ii=2, jj=10), 1.0, 3))
    return out


def hc_cases():
    return [hc_case(name, payload, start, limit, rng, need) for name, payload, start, rng, need in hc_tables() for limit in HC_LIMITS]


# ---- Monte Carlo -------------------------------------------------------------------------------------------------------
MC_W = 60
MC_ORIGIN = (30, 30)
MC_PEAK = (33, 31)


def mc_cases():
    i, j = np.meshgrid(np.arange(MC_W), np.arange(MC_W))
    d = np.maximum(np.abs(i - MC_PEAK[0]), np.abs(j - MC_PEAK[1]))  # Chebyshev distance from the peak cell
    cone = lvl(np.clip(300 - 8 * d, 0, 300))
    ulp_cone = np.zeros((MC_W, MC_W))
    for k in range(int(d.max()) + 1):
        ulp_cone[d == k] = ulps(lvl(200), -min(k, 40))
    start = cell_pose(MC_ORIGIN, MC_PEAK[0] - 4, MC_PEAK[1] - 3, 0.3, 0.6)
    tables = (("cone", cone), ("plateau", np.full((MC_W, MC_W), lvl(5))), ("one_ulp_cone", ulp_cone),
              ("cone_with_nan_ring", np.where(d == 2, NAN, cone)))
    out = []
    for name, t in tables:
        c = types.SimpleNamespace(name=name, kind="MC", params=list(MC_PARAMS), payload=np.ascontiguousarray(t), origin=MC_ORIGIN,
                                  rng=0.0, inits=[start, start + np.array([0.1, -0.2, 0.05])], shape=None, settles=None, expect=None)
        check_values(c)
        out.append(c)
    return out


# ---- all ---------------------------------------------------------------------------------------------------------------
_cache = {}


def all_cases():
    if not _cache:
        for c in bf_cases() + hc_cases() + mc_cases():
            assert c.kind + ":" + c.name not in _cache, c.name
            _cache[c.kind + ":" + c.name] = c
    return list(_cache.values())


def cases_of(kind):
    return [c for c in all_cases() if c.kind == kind]


def case_map(c, po):
    return po.GridMapData(po.CELL_OCC, c.payload, c.origin, S, [PROTO])


def case_scan(c, po):
    """one beam at heading 0, weight 1, factor 1"""
    return po.ScanData([c.rng], [0.0], [1.0], [1.0])


def oracle_matches(c, oracle, po):
    """the oracle's traces of the case's matches, one enumerator object for all of them"""
    kind = dict(BF=po.SM_BF, HC=po.SM_HC, MC=po.SM_MC)[c.kind]
    e, m, scan = oracle.enumerator(kind, c.params), case_map(c, po), case_scan(c, po)
    return [oracle.process_scan(e, m, scan, po.make_cfg(), p) for p in c.inits]


# ---- the golden --------------------------------------------------------------------------------------------------------
def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


def load_golden():
    """tests/golden/landscapes.npz as dict(rows = {"KIND:case#k": dict(n_calls, prob, delta, accepted, scores_sha256,
    poses_sha256)}, refused = the cases the reference's own assertions ended)"""
    g = np.load(GOLDEN)
    off, idx = g["accepted_off"], g["accepted_idx"]
    rows = {str(name): dict(n_calls=int(g["n_calls"][k]), prob=float(g["prob"][k]), delta=g["delta"][k],
                            accepted=idx[off[k]:off[k + 1]].tolist(), scores_sha256=g["scores_sha256"][k],
                            poses_sha256=g["poses_sha256"][k]) for k, name in enumerate(g["names"])}
    return dict(rows=rows, refused=set(str(n) for n in g["refused"]))


def golden_rows(g, c):
    """the golden's rows of the case's matches; None for a case the reference refused"""
    if c.kind + ":" + c.name in g["refused"]:
        return None
    return [g["rows"]["%s:%s#%d" % (c.kind, c.name, k)] for k in range(len(c.inits))]


def assert_equals_row(t, row):
    """a trace (dict of process_scan: n_calls, prob, delta, poses, scores, accepted) against a golden row, bit for bit"""
    assert t["n_calls"] == row["n_calls"]
    assert np.nonzero(t["accepted"])[0].tolist() == row["accepted"]
    assert np.array_equal(sha(t["scores"]), row["scores_sha256"]), "the scores differ"
    assert np.array_equal(sha(t["poses"]), row["poses_sha256"]), "the poses differ"
    assert bits(t["prob"]) == bits(row["prob"]) and np.array_equal(bits(t["delta"]), bits(row["delta"]))
