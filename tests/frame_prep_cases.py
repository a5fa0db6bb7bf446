"""Inputs for the frame-preparation tests (tests/test_frame_prep_host.py, tests/test_gpu_frame_prep.py) and for the generator of their
fixture (tests/golden/make_frame_prep_golden.py): hand-made sequences of post-NMS boxes with the sweeps they were detected in.

Every box is 4 x 1.8 x 1.6 m around z = -1 m; boxes of a frame sit on fixed spots at least 7 m apart.  A box's points are drawn in its own
frame at least 5 cm from every face, so they stay 1 cm clear of it after the rounding to fp32; the background lies 4-8 m above the
sensor, the ground points of the field-of-view cloud at z = -2.5 m: neither is inside any box.  The odometry is 0.8-1 m forwards with a
small turn; a static box's points carry the flow that undoes it, a moving box's points the flow of its planted displacement (both with
1 cm of noise).  min_points_in_box is 5, bev_range_m (80, 80): with dx = 4 a box is clearly inside for |x| < 42.

sequence A, 5 frames, P = 8
  frame 0  slot 0 static; 1 exactly 5 points: kept; 2 four points: dropped; 3 at x one fp32 step below 42: kept; 4 at x = 42: dropped on the
           BEV boundary; 5 no point: dropped, and under "keep_all" its propagated poses are its pose; 6 twelve points, all with
           point_valid = 0: mean flow 0; 7 behind the sensor: kept, outside the annotated field of view
  frame 1  slots 0-3 displaced 0.05 m, 0.2 m, 0.5 m forwards and 0.2 m backwards (flipped), 4-5 static
  frame 2  8 boxes with displacements drawn from (0, 0.15, 0.25, 0.6, -0.25, -0.6)
  frame 3  4 boxes and a sweep without a point
  frame 4  3 boxes
sequence B, 3 frames, P = 8: 5 boxes; a frame without boxes; 8 boxes
sequence W, 1 frame, P = 70: a 10 x 7 grid of boxes 8 m apart, every third with four points only -- the compaction crosses a wavefront
sequence X, 1 frame, P = 300: a 20 x 15 grid of boxes 6 m apart with 0-8 points each, the outer columns beyond the BEV boundary -- more
boxes than a tile of the point pass (128) and than a round of the compaction (256) hold; not in the fixture
sequence empty: no frame"""
import functools

import numpy as np

T, P, N, C, N_FOV, C_FOV = 5, 8, 2500, 4, 3000, 4
MIN_POINTS, BEV_RANGE_M = 5, (80.0, 80.0)
CONFIGS = {
    "filter": dict(drop_boxes_on_bev_boundaries=True, min_points_in_box=MIN_POINTS, align_predicted_boxes_using_flow=True),
    "keep_all": dict(drop_boxes_on_bev_boundaries=False, min_points_in_box=0, align_predicted_boxes_using_flow=True, fov_min_points=3),
    "flow_cluster": dict(drop_boxes_on_bev_boundaries=True, min_points_in_box=MIN_POINTS, align_predicted_boxes_using_flow=True,
                         is_flow_cluster_detector=True),
}
BATCHES = {"AB_empty": ("A", "B", "empty"), "A": ("A",), "B": ("B",), "W": ("W",), "X": ("X",)}
SHAPES = {"A": (T, P), "B": (T, P), "empty": (T, P), "W": (1, 70), "X": (1, 300)}
DIMS = (4.0, 1.8, 1.6)
FRONT = [(14.0, 0.0), (26.0, 9.0), (26.0, -9.0), (36.0, 2.0), (20.0, -6.0), (33.0, -12.0)]  # inside the camera's opening angle
BEHIND = [(-15.0, 3.0), (-25.0, -6.0)]
STEP_INSIDE = float(np.nextafter(np.float32(42.0), np.float32(0.0)))
MARGINS = dict(margin=1e-6, face_margin=0.01, angle_margin=1e-4)  # the conditions under which the reference decides every case
KEYS = ("n_box", "boxes", "conf", "odom", "clouds", "counts", "point_valid", "flow", "fov_clouds", "fov_counts")


def config(name):
    return dict(bev_range_m=BEV_RANGE_M, **CONFIGS[name])


def odometry(t):
    """sensor(t) <- sensor(t + 1)"""
    a = 0.01 * (t + 1)
    M = np.eye(4)
    M[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    M[:3, 3] = [0.8 + 0.05 * t, 0.03, 0.0]
    return M


def _frame(rng, t, spots, n_pts, displacement, n_cloud, invalid=()):
    """one frame: boxes on `spots` (x, y) with `n_pts[i]` points inside and the planted `displacement[i]` along their heading"""
    k = len(spots)
    boxes = np.zeros((k, 7), np.float32)
    boxes[:, :2], boxes[:, 2] = np.asarray(spots, np.float64).reshape(k, 2), rng.uniform(-1.1, -0.9, k)
    boxes[:, 3:6], boxes[:, 6] = DIMS, rng.uniform(-np.pi, np.pi, k)
    conf = rng.uniform(0.3, 0.95, k).astype(np.float32)
    odom = odometry(t)
    inv_odom = np.linalg.inv(odom)
    pts, flow, valid = [], [], []
    for i in range(k):
        b = boxes[i].astype(np.float64)
        c, s = np.cos(b[6]), np.sin(b[6])
        R = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
        local = rng.uniform(-1.0, 1.0, (n_pts[i], 3)) * (0.5 * np.array(DIMS) - 0.05)
        p = local @ R.T + b[:3]
        moved = b[:3] + R @ np.array([displacement[i], 0.0, 0.0])  # where the box centre is a frame later, in this frame's sensor
        m = inv_odom[:3, :3] @ moved + inv_odom[:3, 3] - b[:3]      # odom (centre + m) = moved
        pts.append(p), flow.append(m + rng.uniform(-0.01, 0.01, (n_pts[i], 3))), valid.append(np.full(n_pts[i], i not in invalid))
    n_bg = n_cloud - sum(n_pts)
    r, phi = rng.uniform(5.0, 50.0, n_bg), rng.uniform(-np.pi, np.pi, n_bg)
    pts.append(np.stack([r * np.cos(phi), r * np.sin(phi), rng.uniform(4.0, 8.0, n_bg)], -1))
    flow.append(rng.normal(0.0, 0.5, (n_bg, 3))), valid.append(rng.uniform(size=n_bg) > 0.1)
    pts, flow, valid = np.concatenate(pts), np.concatenate(flow), np.concatenate(valid)
    order = rng.permutation(len(pts)) if len(pts) else np.zeros(0, np.int64)
    cloud = np.concatenate([pts, rng.uniform(0.0, 1.0, (len(pts), 1))], -1)[order].astype(np.float32)
    # the field-of-view cloud (pcl_full_ta): the sweep's points in another order, plus ground
    n_ground = 300
    r, phi = rng.uniform(5.0, 50.0, n_ground), rng.uniform(-np.pi, np.pi, n_ground)
    ground = np.stack([r * np.cos(phi), r * np.sin(phi), np.full(n_ground, -2.5), rng.uniform(0.0, 1.0, n_ground)], -1)
    full = np.concatenate([cloud[rng.permutation(len(cloud))].astype(np.float64), ground]).astype(np.float32)
    ang = np.arctan2(full[:, 1], full[:, 0])
    lo, hi = (np.float32(a / 180.0 * np.pi) for a in (-41.95, 40.16))
    full = full[(np.abs(ang - lo) > 1e-3) & (np.abs(ang - hi) > 1e-3)]  # (no point on the edge of the camera's opening angle)
    return boxes, conf, odom, cloud, flow.astype(np.float32)[order], valid[order].astype(np.uint8), full


def _plans(name, rng):
    """per frame: (spots, points per box, displacement per box, rows of the sweep, boxes whose points are all invalid)"""
    if name == "A":
        some = lambda k: list(rng.choice([0.0, 0.15, 0.25, 0.6, -0.25, -0.6], k))  # noqa: E731
        return [
            (FRONT[:3] + [(STEP_INSIDE, 5.0), (42.0, -6.0), FRONT[4], FRONT[5], BEHIND[0]], [12, 5, 4, 9, 9, 0, 12, 12], [0.0] * 8, N, (6,)),
            (FRONT, [12, 10, 14, 11, 9, 13], [0.05, 0.2, 0.5, -0.2, 0.0, 0.0], 2300, ()),
            (FRONT + BEHIND, [9, 10, 11, 12, 13, 14, 15, 16], some(8), N, ()),
            (FRONT[:4], [0, 0, 0, 0], [0.0] * 4, 0, ()),
            (FRONT[1:4], [20, 7, 6], [0.25, 0.0, -0.6], 1111, ()),
        ]
    if name == "B":
        return [(FRONT[:5], [8, 9, 4, 11, 12], [0.0, 0.6, 0.0, -0.25, 0.15], 2047, ()), ([], [], [], 2049, ()),
                (FRONT + BEHIND, [6, 7, 8, 9, 3, 11, 12, 13], [0.15, 0.0, 0.6, 0.0, 0.0, -0.6, 0.0, 0.25], N, ())]
    if name == "W":
        spots = [(8.0 * (i - 4.5), 8.0 * (j - 3)) for j in range(7) for i in range(10)]
        return [(spots, [4 if i % 3 == 1 else 8 for i in range(70)], list(rng.choice([0.0, 0.15, 0.25, 0.6, -0.25, -0.6], 70)), N, ())]
    if name == "X":
        spots = [(6.0 * (i - 9.5), 6.0 * (j - 7)) for j in range(15) for i in range(20)]
        return [(spots, [i % 9 for i in range(300)], list(rng.choice([0.0, 0.15, 0.25, 0.6, -0.25, -0.6], 300)), N, ())]
    return []


@functools.lru_cache(maxsize=None)
def scene(name):
    """-> dict of the arrays of one sequence, named like the arguments of prepare_tracker_frames without the leading S: n_frames (int),
    n_box [T], boxes [T,P,7], conf [T,P], odom [T,4,4], clouds [T,N,C] NaN-padded, counts [T], point_valid [T,N], flow [T,N,3],
    fov_clouds [T,N_FOV,C_FOV] NaN-padded, fov_counts [T]"""
    t_max, p_max = SHAPES[name]
    rng = np.random.default_rng({"A": 21, "B": 22, "W": 23, "empty": 24, "X": 25}[name])
    plans = _plans(name, rng)
    out = {"n_frames": len(plans), "n_box": np.zeros(t_max, np.int32), "boxes": np.zeros((t_max, p_max, 7), np.float32),
           "conf": np.zeros((t_max, p_max), np.float32), "odom": np.tile(np.eye(4), (t_max, 1, 1)),
           "clouds": np.full((t_max, N, C), np.nan, np.float32), "counts": np.zeros(t_max, np.int32),
           "point_valid": np.zeros((t_max, N), np.uint8), "flow": np.zeros((t_max, N, 3), np.float32),
           "fov_clouds": np.full((t_max, N_FOV, C_FOV), np.nan, np.float32), "fov_counts": np.zeros(t_max, np.int32)}
    for t, (spots, n_pts, disp, n_cloud, invalid) in enumerate(plans):
        boxes, conf, odom, cloud, flow, valid, full = _frame(rng, t, spots, n_pts, disp, n_cloud, invalid)
        k, n, m = len(boxes), len(cloud), len(full)
        out["n_box"][t], out["boxes"][t, :k], out["conf"][t, :k], out["odom"][t] = k, boxes, conf, odom
        out["counts"][t], out["clouds"][t, :n], out["point_valid"][t, :n], out["flow"][t, :n] = n, cloud, valid, flow
        out["fov_counts"][t], out["fov_clouds"][t, :m] = m, full
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def batch(name):
    """the sequences of BATCHES[name] stacked: dict with n_frames int32 [S] and the arrays of `scene` with a leading S"""
    scenes = [scene(n) for n in BATCHES[name]]
    out = {k: np.stack([sc[k] for sc in scenes]) for k in KEYS}
    out["n_frames"] = np.array([sc["n_frames"] for sc in scenes], np.int32)
    return out


def args_of(b):
    """the positional arguments of prepare_tracker_frames / prepare_tracker_frames_host"""
    return [b[k] for k in ("n_frames",) + KEYS]


def checksum(name):
    """a scene's inputs in one number: the fixture stores it, so inputs that drift from the ones it was generated on are noticed"""
    sc = scene(name)
    return float(sum(np.nansum(sc[k].astype(np.float64) * (1.0 + np.arange(sc[k].size).reshape(sc[k].shape) % 7)) for k in KEYS))
