"""Shared by tests/test_oracle_placed_particle_maps.py (CPU) and tests/test_gpu_placed_particle_maps.py (GPU): the per-particle
tiled maps (csrc/tile_pool.hip) FAR FROM THE WORLD ORIGIN.  (No test in here.)

The references are the ones tests/placed_cases.py already hands out: tests/golden/placed.npz holds, per Q station and
occupancy estimator, a real UnboundedLazyTiledGridMap of the compiled reference that grew from (0, 0) to the station in
three append_scans, exported over a 108 x 76 window after each; the oracle's per-particle append
(gmapping_particle_map_append) is the expected value where there is no golden.

Geometry of the pool, restated here so that the tests can say where its tile seams lie: a pool created with E x E tiles
has its virtual origin at E * 64 cells (virtual cell = external cell + origin); every growth adds whole tiles, 128 cells
each, so the origin stays what it was modulo 128.  Seams in EXTERNAL cells are therefore the multiples of 128 for an even E
and the multiples of 128 plus 64 for an odd one.  A golden window is 108 x 76 cells: which parity puts a seam through it on
BOTH axes depends on the station (START_EXTENT; asserted by the CPU suite)."""
import numpy as np
import placed_cases as pc
import placed_scenes as ps

TILE = 128
MAX_TABLE = 1 << 20  # tile_pool_create / tile_pool_grow refuse a table of more entries per slot
RING = 8             # cells around a golden window that the three appends leave untouched
# the start extent whose parity puts a seam through the station's golden window in x AND in y
START_EXTENT = {"Q1": 2, "Q2": 2, "Q3": 1, "Q4": 1}
MODES = ("fast", "sorted", "key64")  # the batch modes of tests/test_gpu_particle_maps.py::test_particle_maps_filter_vs_oracle

# bars of tests/test_gpu_placed.py::check_snapshot for the dense route under the cached provider's arithmetic
MEAN_STRICT = dict(rtol=1e-13, atol=1e-15)  # (the pool meets it: one ulp measured; its near-origin 1e-12 is not needed)
AREA_BAR = dict(rtol=1e-11, atol=1e-13)


def golden_window(g, st):
    """(x0, y0, w, h) of the station's golden window in external cells"""
    w, h, (ox, oy) = pc.window_geometry(g, st)
    return -ox, -oy, w, h


def ringed(win, ring=RING):
    x0, y0, w, h = win
    return x0 - ring, y0 - ring, w + 2 * ring, h + 2 * ring


def seams(extent_tiles, lo, hi):
    """external cells c in [lo, hi) at which a tile of a pool that started with extent_tiles begins; a seam at lo itself
    does not count (the window would only touch it)"""
    off = (extent_tiles * (TILE // 2)) % TILE  # origin mod 128
    first = ((lo + off) // TILE + 1) * TILE - off
    return list(range(first, hi, TILE))


def window_seams(extent_tiles, win):
    x0, y0, w, h = win
    return seams(extent_tiles, x0, x0 + w), seams(extent_tiles, y0, y0 + h)


def smallest_extent(origin, w, h):
    """the smallest E for which a dense window (index bias `origin`) fits E x E tiles around the world origin"""
    need = max(origin[0], w - origin[0], origin[1], h - origin[1])
    return max(1, -(-need // (TILE // 2)))


def device_adder(g, est):
    """enable_particle_maps' adder arguments for the golden's GMapping history"""
    kw = dict(base=tuple(float(v) for v in g["gmapping_base"]), blur=float(g["gmapping_blur"]))
    if est:
        kw.update(estimator=1, shift_amount=float(g["shift_amount"]))
    return kw


def oracle_adder(g, est):
    kw = dict(base=g["gmapping_base"], blur=float(g["gmapping_blur"]))
    if est:
        kw.update(est_kind=1, shift_amount=float(g["shift_amount"]))
    return kw


def raw_scan(g, st):
    return g[st + "_raw_range"], g[st + "_raw_angle"], g[st + "_raw_occ"]


def snapshot(g, st, est, k):
    t = pc.tag(st, "gmapping", est, k)
    return g[t + "payload"], g[t + "aux"]


def check_window(got, want, est, what, mean_bar=MEAN_STRICT):
    """(payload, counters) of a 108 x 76 window against the reference's: hits / tries exact; const estimator: occupancy bit
    for bit, obstacle means within mean_bar; area estimator 1e-11.  Returns the largest deviation of an obstacle mean
    relative to its size (0 for the area estimator, whose bar covers the whole payload)."""
    (got_p, got_a), (want_p, want_a) = got, want
    np.testing.assert_array_equal(got_a, want_a, err_msg=what + ": hits / tries")
    if est:
        np.testing.assert_allclose(got_p, want_p, err_msg=what, **AREA_BAR)
        return 0.0
    # (the GMAPPING case of cell_update in oracle/map_update_oracle.c -- GmappingBaseCell::operator+= -- does not read
    # `quality`: the golden's scan quality 0.9 and the pool's fixed 1.0 are the same update)
    np.testing.assert_array_equal(got_p[..., 0], want_p[..., 0], err_msg=what + ": occupancy")
    dev = np.abs(got_p[..., 1:] - want_p[..., 1:])
    rel = float(np.max(dev / np.maximum(np.abs(want_p[..., 1:]), 1e-300), initial=0.0, where=want_p[..., 1:] != 0.0))
    np.testing.assert_allclose(got_p[..., 1:], want_p[..., 1:], err_msg=what + ": obstacle means (largest relative deviation %.3g)" % rel,
                               **mean_bar)
    return rel


def never_observed(payload, aux, unknown):
    return bool(np.all(payload == np.asarray(unknown, dtype=np.float64)[:3]) and not aux.any())


# ---- the key window of the batched update (csrc/map_update.hip: mu_append_batch), restated ------------------------------------
def scan_bbox(pose, rng, ang, scale):
    """(lo_x, lo_y, hi_x, hi_y): the rectangle of the cells of a job's pose and end points, in external cells -- what the
    walks stay inside (blur 0; the last bit of an end point does not matter for a bit count)"""
    pose = np.asarray(pose, dtype=np.float64)
    x = np.concatenate([[pose[0]], pose[0] + rng * np.cos(pose[2] + ang)])
    y = np.concatenate([[pose[1]], pose[1] + rng * np.sin(pose[2] + ang)])
    cx, cy = np.floor(x / scale).astype(np.int64), np.floor(y / scale).astype(np.int64)
    return int(cx.min()), int(cy.min()), int(cx.max()), int(cy.max())


def key_window(bboxes):
    """mu_append_batch's key window over the jobs' rectangles: one cell of margin, the width padded to a power of two;
    cell_bits + job_bits + 1 (the invalid key sorts last) > 32 sends the batch to the 8-byte keys"""
    b = np.asarray(bboxes, dtype=np.int64).reshape(-1, 4)
    lo_x, lo_y, hi_x, hi_y = b[:, 0].min(), b[:, 1].min(), b[:, 2].max(), b[:, 3].max()
    key_shift = 1
    while (1 << key_shift) < hi_x - lo_x + 3:
        key_shift += 1
    key_w = 1 << key_shift
    key_cells = key_w * int(hi_y - lo_y + 3)
    cell_bits = job_bits = 1
    while (1 << cell_bits) < key_cells:
        cell_bits += 1
    while (1 << job_bits) < b.shape[0]:
        job_bits += 1
    return dict(key_shift=key_shift, key_w=key_w, cell_bits=cell_bits, job_bits=job_bits, end_bit=cell_bits + job_bits + 1,
                span=(int(hi_x - lo_x + 1), int(hi_y - lo_y + 1)))


# ---- what a 3 x 3 window of the GMapping scorer sees (tests/particle_score_scenes.py: window_view, at any scale and seam) ----------
def window_view(m, scan, poses, th, extent_tiles):
    """(nonzero[P, B]: a full cell in the window; other_tile[P, B]: the best full cell lies in another tile than the end
    point's cell) over the flat map m (an oracle GridMapData / a_map), statistics only"""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    a = poses[:, 2:3] + scan.angle[None, :]
    wx = poses[:, 0:1] + scan.range[None, :] * np.cos(a)
    wy = poses[:, 1:2] + scan.range[None, :] * np.sin(a)
    cx, cy = np.floor(wx / m.scale).astype(np.int64), np.floor(wy / m.scale).astype(np.int64)
    h, w = m.payload.shape[:2]
    best = np.full(wx.shape, np.inf)
    bdx, bdy = np.zeros(wx.shape, np.int64), np.zeros(wx.shape, np.int64)
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            ix, iy = cx + dx + m.origin[0], cy + dy + m.origin[1]
            inb = (ix >= 0) & (ix < w) & (iy >= 0) & (iy < h)
            cell = m.payload[np.clip(iy, 0, h - 1), np.clip(ix, 0, w - 1)]
            full = inb & (cell[..., 0] >= th)
            d2 = np.where(full, (cell[..., 1] - wx) ** 2 + (cell[..., 2] - wy) ** 2, np.inf)
            better = d2 < best
            best = np.where(better, d2, best)
            bdx, bdy = np.where(better, dx, bdx), np.where(better, dy, bdy)
    nonzero = np.isfinite(best)
    off = (extent_tiles * (TILE // 2)) % TILE
    tile = lambda c: (c + off) // TILE  # noqa: E731
    other_tile = nonzero & ((tile(cx + bdx) != tile(cx)) | (tile(cy + bdy) != tile(cy)))
    return nonzero, other_tile


def check_shares(views, what, need_seam=True):
    """particle_score_scenes.check_conditions' shares: at least 20 % of the (pose, beam) values above 0 and 20 % equal to
    0, and a best full cell across a tile seam (need_seam False: the map has no cell beside a seam that is full at the
    threshold -- the caller asserts that, and that the other threshold has one)"""
    nz = np.concatenate([v[0].ravel() for v in views])
    assert nz.size > 0, what
    assert nz.mean() >= 0.2 and (~nz).mean() >= 0.2, (what, nz.mean())
    if need_seam:
        assert sum(int(v[1].sum()) for v in views) >= 1, what + ": no window whose best cell lies across a seam"


# ---- the jobs of the readers ---------------------------------------------------------------------------------------------------
THRESHOLDS = (0.1, 0.8)  # particle_score_scenes.TH_FILTER (the tiles' masks are valid for it), TH_OTHER (the nine-cell path)


def beside_seams(m, extent_tiles, th):
    """[K, 2] world points, one per cell of m that is full at th and lies beside a tile seam: the cell's obstacle mean moved
    one cell ACROSS the seam (a beam that ends there has its best full cell in the other tile)"""
    x0, y0 = -m.origin[0], -m.origin[1]
    h, w = m.payload.shape[:2]
    sx, sy = window_seams(extent_tiles, (x0, y0, w, h))
    full = m.payload[..., 0] >= th
    ends = []
    for s in sx:
        for col, step in ((s - x0 - 1, 1.0), (s - x0, -1.0)):
            for row in np.nonzero(full[:, col])[0]:
                ends.append((m.payload[row, col, 1] + step * m.scale, m.payload[row, col, 2]))
    for s in sy:
        for row, step in ((s - y0 - 1, 1.0), (s - y0, -1.0)):
            for col in np.nonzero(full[row])[0]:
                ends.append((m.payload[row, col, 1], m.payload[row, col, 2] + step * m.scale))
    return np.array(ends, dtype=np.float64).reshape(-1, 2)


def reader_poses(base, true_pose, scan, m, extent_tiles, seed, n_off=40, n_seam=24):
    """`base` (the station's Q*_gm_poses: all next to the true pose, nine windows in ten see a full cell), then poses up to
    2.5 m off with any heading (most of their beams end in free or never-observed space) and poses whose FIRST end point
    lies one cell across a tile seam from a full cell of m (particle_score_scenes.seam_poses, with the seams of a pool that
    started with extent_tiles), the cells full at the higher threshold first."""
    rs = np.random.RandomState(seed)
    off = true_pose + np.column_stack([rs.uniform(-2.5, 2.5, n_off), rs.uniform(-2.0, 2.0, n_off), rs.uniform(-3.1, 3.1, n_off)])
    ends = np.vstack([beside_seams(m, extent_tiles, th) for th in sorted(THRESHOLDS, reverse=True)])
    assert len(ends), "no full cell beside a seam"
    ends = np.vstack([ends, ends + [0.3 * m.scale, -0.2 * m.scale], ends - [0.2 * m.scale, 0.3 * m.scale]])[:n_seam]
    th = rs.rand(len(ends)) * 6.3 - 3.15
    r, a = scan.range[0], scan.angle[0]
    seam = np.column_stack([ends[:, 0] - r * np.cos(th + a), ends[:, 1] - r * np.sin(th + a), th])
    return np.vstack([base, off, seam])


def golden_reader_poses(g, st, m, extent_tiles):
    return reader_poses(g[st + "_gm_poses"], g[st + "_true_pose"], pc.golden_scan(g, st, 0), m, extent_tiles, 700 + ps.SEEDS[st])


CARRY_SHIFTS = np.array([[0.0, 0.0, 0.0], [2e-4, -1e-4, 0.0], [-1e-4, 3e-4, 0.0], [3e-4, 2e-4, 0.0]])


def carry_from(scan, bases):
    """The carry job of tests/test_gpu_particle_score.py::test_the_run_cache_is_carried_within_a_job_and_nowhere_else for a
    scene of its own: a scan whose last point repeats its first (the first 40 points of `scan`), and groups of four poses
    equal up to a fraction of a cell -- a pose's first beam ends in the cell the pose before it ended in.
    Returns (scan as a ScanData without a provider, poses[4 * len(bases), 3])."""
    from pyoracle import ScanData
    rng, ang = scan.range[:40].copy(), scan.angle[:40].copy()
    rng[-1], ang[-1] = rng[0], ang[0]
    poses = np.vstack([b + d for b in bases for d in CARRY_SHIFTS])
    return ScanData(rng, ang, np.full(40, 1.0 / 40)), poses


def carry_case(g, st, n_bases=12):
    """... moved to the station: the golden scan and the golden's own GMapping poses"""
    return carry_from(pc.golden_scan(g, st, 0), g[st + "_gm_poses"][2:2 + n_bases])


def scan_gen_poses(true_pose, scale, seed, n_poses=8, n_angles=90, max_dist=4.0):
    """8 poses within 1 m of the true pose, 90 angles all around; the external window that holds every beam's last cell:
    the poses' cells with a margin of max_dist / scale cells (+ 2).  Returns (poses, angles, max_dist, window)."""
    rs = np.random.RandomState(seed)
    poses = true_pose + np.column_stack([rs.uniform(-1.0, 1.0, n_poses), rs.uniform(-1.0, 1.0, n_poses), rs.uniform(-3.1, 3.1, n_poses)])
    poses[0] = true_pose
    angles = np.linspace(-np.pi, np.pi, n_angles, endpoint=False) + 0.003
    margin = int(np.ceil(max_dist / scale)) + 2
    cx, cy = np.floor(poses[:, 0] / scale).astype(int), np.floor(poses[:, 1] / scale).astype(int)
    x0, y0 = int(cx.min()) - margin, int(cy.min()) - margin
    return poses, angles, max_dist, (x0, y0, int(cx.max()) + margin + 1 - x0, int(cy.max()) + margin + 1 - y0)


def scan_gen_case(g, st):
    return scan_gen_poses(g[st + "_true_pose"], float(g["scale"]), 900 + ps.SEEDS[st])


# ---- one batch over the four quadrants -----------------------------------------------------------------------------------------
def four_quadrant_jobs(g, lead, k):
    """(poses[4, 3], range, angle, occ) of append k: particle i stands at Q(i + 1) and takes append pose k of its station.
    particle_maps_append hands ONE scan to all its jobs and the stations' scans differ, so the call carries the scan of
    the `lead` station: the lead's particle repeats the golden's history, the other three are held to the oracle."""
    r, a, occ = raw_scan(g, lead)
    return np.array([g[st + "_append_poses"][k] for st in ps.Q_STATIONS]), r, a, occ


def wide_window(st, half=80):
    """(x0, y0, w, h): 160 x 160 external cells around the station's cell -- another station's scan, cast under another
    heading, leaves the 108 x 76 golden window but not this one"""
    (kx, ky), _ = ps.station_entry(st)
    return kx - half, ky - half, 2 * half, 2 * half


def fresh_window_map(g, win):
    """(map, counters): a never-observed GMapping window of the oracle over the external cells `win`"""
    from pyoracle import CELL_GMAPPING, GridMapData
    x0, y0, w, h = win
    unk = g["Q1_gmapping_unknown"][:3]
    return GridMapData(CELL_GMAPPING, np.tile(unk, (h, w, 1)).astype(np.float64), (-x0, -y0), float(g["scale"]), unk), np.zeros((h, w, 2))


# ---- the filter's own step at a station (tests/golden/gmapping_pf_update.npz moved by whole cells) --------------------------------
PF_GP = [0, 0.1, 0, 0.05, 0, 0, 0, 0]  # (the pose noise of test_particle_maps_resampling_shares_then_clones_tiles)
PF_N = 6
# found with the oracle alone (as for test_particle_maps_resampling_shares_then_clones_tiles): with these seeds the run
# resamples at its 13th step -- the fixture's five steps, then its scans 1 .. 4 replayed twice -- at every station
PF_SEED0, PF_EXTRA = 3100, 9


def pf_steps(gg, extra):
    n_base = int(gg["n_steps"])
    return list(range(n_base)) + [1 + (k % (n_base - 1)) for k in range(extra)]


def pf_geometry(gg, station):
    """(w, h, origin, scale, unknown, shift): the fixture's window moved to the station by whole cells"""
    w, h = [int(v) for v in gg["size"]]
    scale = float(gg["scale"])
    (kx, ky), _ = ps.station_entry(station)
    ox, oy = [int(v) for v in gg["origin"]]
    return w, h, (ox - kx, oy - ky), scale, gg["unknown"][:3], ps.shift_m(station, scale)


def pf_oracle_start(oracle, gg, station):
    """(map, counters, shift): the common ancestor of tests/test_gpu_particle_maps.py::run_both at the station -- the
    first scan appended from the moved first pose into a never-observed window"""
    from pyoracle import CELL_GMAPPING, GridMapData
    w, h, origin, scale, unknown, shift = pf_geometry(gg, station)
    m = GridMapData(CELL_GMAPPING, np.tile(unknown, (h, w, 1)).astype(np.float64), origin, scale, unknown)
    aux = np.zeros((h, w, 2))
    pc.append_scan_ex(oracle, m, aux, pc.RULE_GMAPPING, gg["step0_delta"] + shift, gg["step0_range"], gg["step0_angle"])
    return m, aux, shift
