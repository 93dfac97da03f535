"""make_scene-style scenes at a STATION far from the world origin (numpy only, on top of synth.py).

Every scene of synth.make_scene has the robot at (scale/2, scale/2, 90 deg) in a window whose origin is its centre.
A station moves such a scene by a whole number of cells (kx, ky) and gives the robot another true heading h:
  * the ground truth is synth.make_world, whose raster is centred on its own (0, 0); the scan is cast from
    (scale/2, scale/2, h) and the map built by synth.build_map, all still next to (0, 0);
  * then the scene is moved: map.origin = (size//2 - kx, size//2 - ky), (kx*scale, ky*scale) is added to every pose
    (true, initial, candidates) and, for GMapping payloads, to the obstacle means of the known cells.
Scan ranges, angles, weights and the other payload numbers are untouched: the moved scene is a scene of its own (an end
point next to a cell edge may round into the neighbour cell out there), which is all a parity test needs -- device and
oracle get the SAME moved inputs.  With shift (0, 0) and h = pi/2 the arrays are make_scene's bit for bit.

Stations are given in cells, so they serve any scale: at 0.05 m the Q stations lie 500 ... 1000 m out, one per quadrant,
and the F stations about 1e5 m out; at 0.1 m twice that.  For a map that does not contain (0, 0) the window's origin
(an index bias) lies outside the window: negative, or beyond the extent.
"""
import numpy as np
import synth

#            shift in cells           true heading
STATIONS = {
    "O": ((0, 0), np.pi / 2),                   # control: synth.make_scene
    "Q1": ((20011, 10007), 0.3),
    "Q2": ((-20011, 10007), 3.1),
    "Q3": ((-10007, -20011), -2.9),
    "Q4": ((10007, -20011), 7.6),               # beyond 2 pi: the reference never normalises a pose
    "F1": ((2097155, -2097157), -0.07),
    "F2": ((-2097155, 1048577), -1.5708),
}
ALL = list(STATIONS)
Q_STATIONS = ["Q1", "Q2", "Q3", "Q4"]
F_STATIONS = ["F1", "F2"]
# world seed per station, fixed (Q1, Q4: the first seeds from 11 / 14 on at which the golden's Monte-Carlo trace accepts a
# candidate; tests/golden/make_golden_placed.py asserts it)
SEEDS = {"O": 3, "Q1": 15, "Q2": 12, "Q3": 13, "Q4": 19, "F1": 21, "F2": 22}
INIT_OFFSET = np.array([0.07, -0.04, 0.03])  # synth.make_scene's perturbation of the true pose

# A second table, apart from STATIONS (whose parametrised tests do not change): the N stations, 500 ... 1500 cells out,
# which the compiled reference reaches with a DENSE pyramid (M3RSMRescalableGridMap<UnboundedPlainGridMap>: every level
# grows from (0, 0) to the data, so its cost is the square of the distance).  Both shifts odd -- no block corner of any
# level falls on the window's -- one station per sign pattern that is not (+, +).
N_TABLE = {
    "N1": ((-1021, 517), 2.2),
    "N2": ((1303, -771), -0.8),
    "N3": ((-643, -1459), -2.4),
}
N_STATIONS = list(N_TABLE)
N_SEEDS = {"N1": 31, "N2": 32, "N3": 33}


def station_entry(name):
    """((kx, ky), heading) of a station of either table"""
    return STATIONS[name] if name in STATIONS else N_TABLE[name]


def shift_m(station, scale):
    """The station's shift in metres, as the doubles every moved quantity is built from."""
    (kx, ky), _ = station_entry(station)
    return np.array([kx * scale, ky * scale, 0.0])


def move_map(m, station):
    """The map of a scene built next to (0, 0), moved to the station (a new MapData; GMapping means moved too)."""
    (kx, ky), _ = station_entry(station)
    s = shift_m(station, m.scale)
    pay = m.payload.copy()
    if m.cell_model == synth.CELL_GMAPPING:
        known = pay[..., 0] != m.unknown[0]
        pay[..., 1][known] += s[0]
        pay[..., 2][known] += s[1]
    return synth.MapData(m.cell_model, pay, (m.origin[0] - kx, m.origin[1] - ky), m.scale, m.unknown, m.bounded)


def place(station, cell_model=synth.CELL_OCC, size=240, scale=0.1, n_beams=360, weighting="even", max_dist=30.0,
          blur_m=0.3, seed=None, raw=False):
    """One scene at `station`: dict(map, scan, init_pose, true_pose, gt, shift, local[, raw]) like synth.make_scene's.
    raw: also the scan as the scanner hands it over, (ranges, angles, is_occupied) of every beam (cast_scan's raw form;
    ranges[is_occupied] are scan.range)."""
    _, h = station_entry(station)
    seed = {**SEEDS, **N_SEEDS}[station] if seed is None else seed
    gt = synth.make_world(size, scale, seed)
    local = np.array([scale / 2, scale / 2, h])
    rng, ang = synth.cast_scan(gt, scale, local, n_beams, max_dist=max_dist)
    m = synth.build_map(cell_model, size, scale, local, rng, ang,
                        blur_m=blur_m if cell_model != synth.CELL_GMAPPING else 0.0)
    w = np.full(rng.size, 1.0 / rng.size) if weighting == "even" else synth.viny_weights(rng, ang)
    s = shift_m(station, scale)
    true_pose = local + s
    out = dict(map=move_map(m, station), scan=synth.Scan(rng, ang, w), init_pose=local + INIT_OFFSET + s,
               true_pose=true_pose, gt=gt, shift=s, station=station, local=local)
    if raw:
        out["raw"] = synth.cast_scan(gt, scale, local, n_beams, max_dist=max_dist, raw=True)
    return out


def candidates(scene, n, seed, sigma=(0.2, 0.2, 0.1)):
    """n candidate poses around the scene's initial pose: drawn next to (0, 0), then moved like every other pose (so the
    offsets are the same numbers at every station); the first two are the initial pose itself, twice."""
    rs = np.random.RandomState(seed)
    local = scene["local"] + INIT_OFFSET
    poses = local + rs.randn(n, 3) * np.asarray(sigma)
    poses[:2] = local
    return poses + scene["shift"]


def ulp_neighbours(poses):
    """[9, P, 3]: every pose and its eight neighbours one ulp away in x and / or y (the probe the far-out allowances and
    the ill-conditioned poses of the piecewise-constant scorers are measured with, on the reference side only)."""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    out = []
    for dx in (0, -1, 1):
        for dy in (0, -1, 1):
            q = poses.copy()
            if dx:
                q[:, 0] = np.nextafter(q[:, 0], dx * np.inf)
            if dy:
                q[:, 1] = np.nextafter(q[:, 1], dy * np.inf)
            out.append(q)
    return np.stack(out)
