"""A small numpy ray-caster for the odometry tests: sweeps of a WORLD-FIXED scene seen from a moving sensor, with the true poses.

(`liso_amd.datasets.synthetic.render` cannot serve: its walls sit at +-48 m in the sensor frame and would vouch for zero motion.)

The scene: an irregular five-sided room (no two walls parallel), a ground plane, ten static boxes and three moving ones.  The sensor
has 16 rings x 360 azimuths (5760 rays), sits 1.7 m above the ground and follows a curved path with 0.25-0.6 m and up to 2 degrees
per frame; range noise is 1 cm.  Rays without a hit are dropped, the rest padded with NaN rows.  With `PARAMS` (max_range 30 ->
voxels of 0.3 m, min_range 1) six frames are the smallest shape at which every path of the odometry runs: voxels reach their
20-point cap, the map drops voxels by range (the room's far corner is 29.6 m from the start and the sensor drives away from it), the
threshold leaves its initial value, and the moving boxes meet the robust weight.  tests/test_odometry_host.py asserts each of these.
"""
import functools

import numpy as np

PARAMS = dict(max_range=30.0, min_range=1.0)  # voxel_size -> 0.3
N_RINGS, N_AZIMUTH = 16, 360
N_MAX = N_RINGS * N_AZIMUTH
SENSOR_HEIGHT, WALL_HEIGHT, RANGE_NOISE = 1.7, 8.0, 0.01
ROOM = np.array([(-27.0, -8.0), (14.0, -10.0), (17.0, 9.0), (-5.0, 12.0), (-26.0, 7.0)])  # counter-clockwise
# centre x, y, size x, y, z, yaw; all stand on the ground
STATIC_BOXES = np.array([(6.0, 3.0, 2.0, 1.0, 1.5, 0.3), (9.0, -5.0, 4.2, 1.8, 1.6, 0.1), (-4.0, 6.0, 1.0, 3.0, 2.2, -0.4),
                         (-8.0, -4.0, 2.5, 2.5, 1.0, 0.8), (12.0, 5.0, 1.2, 1.2, 3.0, 0.0), (3.0, -6.0, 4.5, 1.9, 1.7, -0.2),
                         (-13.0, 2.0, 3.0, 1.0, 2.0, 1.2), (-18.0, -3.0, 2.0, 4.0, 2.5, 0.5), (1.0, 8.0, 5.0, 0.8, 1.2, 0.15),
                         (-21.0, 4.0, 1.5, 1.5, 4.0, 0.6)])
# the same columns, then velocity x, y per frame
MOVING_BOXES = np.array([(5.0, -2.5, 4.0, 1.8, 1.5, 0.0, 0.7, 0.0), (-6.0, 2.0, 4.0, 1.8, 1.5, 3.1, -0.5, 0.05),
                         (8.0, 6.5, 0.8, 0.8, 1.8, 1.0, -0.1, -0.3)])
# per-frame speed (m) and yaw rate (degrees) of the three trajectories
PATHS = {"a": dict(start=(1.5, 0.0, 0.05), speed=(0.30, 0.50, 0.25, 0.60, 0.35), yaw_deg=(1.0, -1.5, 2.0, 0.5, -2.0)),
         "b": dict(start=(-3.0, -1.0, 0.6), speed=(0.45, 0.25, 0.55), yaw_deg=(-2.0, 1.0, -0.5)),
         "c": dict(start=(4.0, 2.0, -1.0), speed=(), yaw_deg=())}


def _pose(x, y, yaw):
    c, s = np.cos(yaw), np.sin(yaw)
    T = np.eye(4)
    T[:2, :2], T[:3, 3] = [[c, -s], [s, c]], (x, y, SENSOR_HEIGHT)
    return T


def true_poses(path):
    """w_T_lidar float64 [F,4,4] of trajectory `path` in the scene's world"""
    p = PATHS[path]
    x, y, yaw = p["start"]
    poses = [_pose(x, y, yaw)]
    for v, w in zip(p["speed"], p["yaw_deg"]):
        yaw += np.deg2rad(w)
        x, y = x + v * np.cos(yaw), y + v * np.sin(yaw)
        poses.append(_pose(x, y, yaw))
    return np.stack(poses)


def _hit_boxes(o, d, boxes):
    """nearest positive ray parameter per ray against boxes standing on the ground (slab test in the box frame), inf without a hit"""
    t_best = np.full(len(d), np.inf)
    for cx, cy, sx, sy, sz, yaw in boxes[:, :6]:
        c, s = np.cos(yaw), np.sin(yaw)
        R = np.array([[c, s, 0.0], [-s, c, 0.0], [0.0, 0.0, 1.0]])  # world -> box
        ob, db = R @ (o - np.array([cx, cy, 0.5 * sz])), d @ R.T
        half = 0.5 * np.array([sx, sy, sz])
        with np.errstate(divide="ignore", invalid="ignore"):
            t1, t2 = (-half - ob) / db, (half - ob) / db
        lo, hi = np.nanmax(np.minimum(t1, t2), axis=1), np.nanmin(np.maximum(t1, t2), axis=1)
        hit = (lo <= hi) & (lo > 0.0)
        t_best = np.where(hit & (lo < t_best), lo, t_best)
    return t_best


def _hit_room(o, d, room):
    t_best = np.full(len(d), np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = -o[2] / d[:, 2]  # the ground
        t_best = np.where((d[:, 2] < 0.0) & (t > 0.0), t, t_best)
        for a, b in zip(room, np.roll(room, -1, axis=0)):
            e = b - a
            den = d[:, 0] * e[1] - d[:, 1] * e[0]
            t = ((a[0] - o[0]) * e[1] - (a[1] - o[1]) * e[0]) / den
            u = ((a[0] - o[0]) * d[:, 1] - (a[1] - o[1]) * d[:, 0]) / den
            z = o[2] + t * d[:, 2]
            hit = (t > 0.0) & (u >= 0.0) & (u <= 1.0) & (z >= 0.0) & (z <= WALL_HEIGHT)
            t_best = np.where(hit & (t < t_best), t, t_best)
    return t_best


def sweep(T, frame, rng, n_rings=N_RINGS, n_azimuth=N_AZIMUTH, elevation_deg=(-15.0, 15.0), spread=1.0):
    """the sweep float32 [n,3] (sensor frame, rays without a hit dropped) seen from w_T_lidar `T` at frame `frame`; `spread` moves the
    room's corners and the boxes' centres apart by that factor (a larger scene of the same objects, for timing)"""
    az = np.deg2rad(np.arange(n_azimuth) * (360.0 / n_azimuth))
    el = np.deg2rad(np.linspace(*elevation_deg, n_rings))
    d_sensor = np.stack([np.outer(np.cos(az), np.cos(el)), np.outer(np.sin(az), np.cos(el)), np.outer(np.ones_like(az), np.sin(el))], -1).reshape(-1, 3)
    d = d_sensor @ T[:3, :3].T
    static, moving = STATIC_BOXES.copy(), MOVING_BOXES.copy()
    moving[:, :2] += frame * moving[:, 6:8] / spread
    static[:, :2], moving[:, :2] = static[:, :2] * spread, moving[:, :2] * spread
    t = np.minimum(_hit_room(T[:3, 3], d, ROOM * spread), np.minimum(_hit_boxes(T[:3, 3], d, static), _hit_boxes(T[:3, 3], d, moving)))
    t = t + RANGE_NOISE * rng.standard_normal(len(t))
    hit = np.isfinite(t)
    return (d_sensor[hit] * t[hit, None]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def sequence(path):
    """-> (clouds float32 [F, N_MAX, 3] padded with NaN rows, counts int32 [F], true w_T_lidar float64 [F,4,4]); read-only"""
    poses = true_poses(path)
    rng = np.random.default_rng(sorted(PATHS).index(path))
    clouds, counts = np.full((len(poses), N_MAX, 3), np.nan, np.float32), np.zeros(len(poses), np.int32)
    for f, T in enumerate(poses):
        pts = sweep(T, f, rng)
        clouds[f, :len(pts)], counts[f] = pts, len(pts)
    for a in (clouds, counts, poses):
        a.setflags(write=False)
    return clouds, counts, poses


@functools.lru_cache(maxsize=None)
def batch(paths=("a", "b", "c")):
    """the sequences of `paths` padded to the longest -> (clouds [S,F,N_MAX,3], counts [S,F], n_frames [S]); padded frames are NaN rows
    with a count of N_MAX, so that a kernel that looked at them would show"""
    seqs = [sequence(p) for p in paths]
    F = max(len(c) for c, _, _ in seqs)
    clouds, counts = np.full((len(seqs), F, N_MAX, 3), np.nan, np.float32), np.full((len(seqs), F), N_MAX, np.int32)
    for s, (c, n, _) in enumerate(seqs):
        clouds[s, :len(c)], counts[s, :len(c)] = c, n
    n_frames = np.array([len(c) for c, _, _ in seqs], np.int32)
    for a in (clouds, counts, n_frames):
        a.setflags(write=False)
    return clouds, counts, n_frames


def relative(poses):
    """inv(T_{n-1}) T_n for n >= 1"""
    return [np.linalg.inv(a) @ b for a, b in zip(poses[:-1], poses[1:])]


def pose_distance(A, B, radius=PARAMS["max_range"]):
    """how far two poses are apart, in metres at `radius`: 2 radius sin(theta / 2) + |t| of inv(A) B"""
    D = np.linalg.inv(A) @ B
    theta = np.arccos(np.clip(0.5 * (np.trace(D[:3, :3]) - 1.0), -1.0, 1.0))
    return 2.0 * radius * np.sin(theta / 2.0) + np.linalg.norm(D[:3, 3])
