"""Inputs for the track-mining tests (tests/test_track_mining_host.py, tests/test_gpu_track_mining.py): two hand-made sequences of
T = 12 frames with at most K = 6 detections per frame, sweeps of about 2 000 points, and the configurations they are mined under.

Objects sit 14 m apart in x and move along +y only, so no two come near each other; a detection sits on its object (positions without
noise in an object's first and last frame, where the travelled distance is read, and within 0.05 m in between), its propagated poses on
the object one frame earlier / later.  Time between frames 0.1 s, min_track_age 4, confidence threshold 0.5, minimum speed 1 m/s, travel
filter 3 m (flow-cluster branch), smoothing from 5 m.

sequence A (object: frames, travelled distance, median confidence -> fate)
  0: 0-11, 6.6 m, 0.8                    kept, smoothed; its id (1) is lower than that of object 1, which a frame lists first
  1: 0-11, 4.99 m, 0.8                   kept, just under the smoothing distance
  2: 0-11, 0 m, 0.8                      stationary but long: dropped by the speed filter
  3: 3-5, 3 m, 0.8                       3 frames, one short of min_track_age; frame 5 holds all six objects
  4: 5-8, 6 m, 0.8                       4 frames: kept and smoothed (MIN_TRACK_LEN_FOR_SMOOTHING)
  5: 0-5 and 7-11, 8.8 m                 a hole at frame 6 (filled with the detection of frame 5); 12 confidences whose two middle ones
                                         are 0.5 and 0.7: the median is the lower one, equal to the threshold -> kept; no point inside
sequence B
  0: 0-11, 6.6 m                         lower middle confidence one fp32 step below 0.5 -> dropped
  1: 0-11, 6.6 m                         middle confidences 0.4 and 0.9 -> dropped (a mean or the upper middle would keep it)
  2: 2-6, 2 m, 0.8                       4 m/s, but under the travel filter: kept by a network's boxes, dropped by flow-cluster boxes
  3: 0-10, 5.01 m, 0.8                   just over the smoothing distance
  4: 8-11, 6 m, 0.8                      the only kept track of frame 11, where its detection lies outside the annotated field of view
Sweeps: a ring of background points 80-100 m away and 30 points on two edges of the objects named in PLANTED (their true outline, which
is turned by 3 degrees and 5 % larger than a typical detection), none near the others."""
import functools

import numpy as np

import tracker_scenes as TS

T, DT, N_POINTS = 12, 0.1, 2048
BASE = dict(min_track_age=4, confidence_threshold_mined_boxes=0.5, min_track_obj_speed_mps=1.0, time_between_frames_s=DT,
            is_flow_cluster_detector=False, flow_cluster_detector_min_travel_dist_filter_m=3.0, fit_rot=False, fit_pos=False,
            fitting_dims_bloat_factor=1.2, min_dist_for_track_smoothing=5.0, use_track_smoothing=True, track_smoothing_method="none",
            export_only_in_annotated_fov=False)
# configuration name -> what it changes
CONFIGS = {"network": {}, "flow_cluster": {"is_flow_cluster_detector": True}, "fov": {"export_only_in_annotated_fov": True},
           "no_smoothing": {"use_track_smoothing": False}, "no_speed_filter": {"min_track_obj_speed_mps": 0.0}}
BATCHES = {"AB": ("A", "B"), "A": ("A",), "B": ("B",), "A_empty": ("A", "empty"), "empty_A": ("empty", "A")}
STEP_BELOW = float(np.nextafter(np.float32(0.5), np.float32(0.0)))
_A5 = [0.35, 0.4, 0.45, 0.5, 0.7, 0.3, None, 0.75, 0.8, 0.85, 0.9, 0.95]  # (frame 5's 0.3 counts twice: it fills the hole)
OBJECTS = {
    "A": [dict(frames=(0, 11), dist=6.6), dict(frames=(0, 11), dist=4.99), dict(frames=(0, 11), dist=0.0), dict(frames=(3, 5), dist=3.0),
          dict(frames=(5, 8), dist=6.0), dict(frames=(0, 11), dist=8.8, hole=6, conf=_A5)],
    "B": [dict(frames=(0, 11), dist=6.6, conf=[0.9, 0.2, 0.8, 0.3, STEP_BELOW, 0.7, 0.1, 0.95, 0.4, 0.6, 0.45, 0.85]),
          dict(frames=(0, 11), dist=6.6, conf=[0.9, 0.1, 0.95, 0.2, 0.4, 0.3, 0.92, 0.15, 0.97, 0.25, 0.91, 0.99]),
          dict(frames=(2, 6), dist=2.0), dict(frames=(0, 10), dist=5.01), dict(frames=(8, 11), dist=6.0)],
}
PLANTED = {"A": (0, 1, 4), "B": (3, 4)}
OUTSIDE_FOV = {"A": [(4, 0)], "B": [(11, 4)]}  # (frame, object) whose detection lies outside the annotated field of view


@functools.lru_cache(maxsize=None)
def scene(name):
    """-> the arrays of one sequence as tests/tracker_scenes.py packs them, plus clouds float32 [T,N_POINTS,4] NaN-padded, counts int32
    [T], in_fov uint8 [T,K] and object_of int [T,K] (the object behind each detection, -1 for padding)"""
    objs = OBJECTS[name]
    rng = np.random.default_rng({"A": 11, "B": 12}[name])
    n = len(objs)
    x0 = (np.arange(n) - (n - 1) / 2) * 14.0
    y0 = rng.uniform(-10, 10, n)
    yaw = np.full(n, np.pi / 2) + rng.uniform(-0.2, 0.2, n)
    dims = np.stack([rng.uniform(3.5, 5.0, n), rng.uniform(1.6, 2.2, n), rng.uniform(1.4, 2.0, n)], axis=1)
    odom = TS.compose(rng.uniform(0.5, 1.5, T), rng.uniform(-0.2, 0.2, T), rng.uniform(-0.05, 0.05, T), rng.uniform(-0.05, 0.05, T))
    W = [np.eye(4)]
    for t in range(T - 1):
        W.append(W[-1] @ odom[t])

    def world_pose(i, t, noise=0.0):
        first, last = objs[i]["frames"]
        y = y0[i] + objs[i]["dist"] * (t - first) / max(last - first, 1)
        jitter = rng.uniform(-noise, noise, 2) if first < t < last else np.zeros(2)
        return TS.compose(np.array(x0[i] + jitter[0]), np.array(y + jitter[1]), np.array(0.3 * i - 0.5), np.array(yaw[i]))

    frames, clouds, counts = [], np.full((T, N_POINTS, 4), np.nan, np.float32), np.zeros(T, np.int32)
    fov, object_of = np.ones((T, 6), np.uint8), np.full((T, 6), -1)
    for t in range(T):
        seen = [i for i, o in enumerate(objs) if o["frames"][0] <= t <= o["frames"][1] and o.get("hole") != t]
        inv = np.linalg.inv(W[t])
        own = np.stack([inv @ world_pose(i, t, 0.05) for i in seen])
        into_prev = np.stack([np.linalg.inv(W[max(t - 1, 0)]) @ world_pose(i, t - 1) for i in seen])
        into_next = np.stack([np.linalg.inv(W[min(t + 1, T - 1)]) @ world_pose(i, t + 1) for i in seen])
        conf = np.array([objs[i]["conf"][t] if "conf" in objs[i] else 0.8 for i in seen], np.float32)[:, None]
        det_dims = (dims[seen] * rng.uniform(0.9, 1.0, (len(seen), 3))).astype(np.float32)
        det_yaw = np.arctan2(own[:, 1, 0], own[:, 0, 0]) + np.deg2rad(3.0)
        frames.append({"pos": own[:, :3, 3].astype(np.float32), "rot": det_yaw[:, None].astype(np.float32), "dims": det_dims, "probs": conf,
                       "odom": odom[t], "into_prev": into_prev, "into_next": into_next})
        object_of[t, :len(seen)] = seen
        for k, i in enumerate(seen):
            fov[t, k] = 0 if (t, i) in OUTSIDE_FOV[name] else 1
        # the sweep: a far ring, and two edges of the planted objects' true outline
        m = int(rng.integers(1800, 1901))
        ang, rad = rng.uniform(-np.pi, np.pi, m), rng.uniform(80.0, 100.0, m)
        pts = [np.stack([rad * np.cos(ang), rad * np.sin(ang), rng.uniform(-2, 1, m)], axis=1)]
        for k, i in enumerate(seen):
            if i in PLANTED[name]:
                u = rng.uniform(-0.5, 0.5, 30)
                edge = np.where(np.arange(30)[:, None] < 18, np.stack([u, np.full(30, -0.5)], 1), np.stack([np.full(30, 0.5), u], 1)) * dims[i, :2] * 1.05
                true = inv @ world_pose(i, t)
                pts.append(np.concatenate([edge, np.zeros((30, 1)), np.ones((30, 1))], axis=1) @ true.T[:, :3])
        pts = np.concatenate(pts)
        pts = pts[rng.permutation(len(pts))]
        counts[t] = len(pts)
        clouds[t, :len(pts), :3], clouds[t, :len(pts), 3] = pts, rng.uniform(0, 1, len(pts))
    out = TS.pack(frames)
    assert out["boxes"].shape[1] <= 6 and counts.max() <= N_POINTS
    out.update(clouds=clouds, counts=counts, in_fov=fov[:, :out["boxes"].shape[1]], object_of=object_of[:, :out["boxes"].shape[1]])
    return out


@functools.lru_cache(maxsize=None)
def batch(name):
    """-> (the arrays `track_sequences` takes, {clouds [S,T,N,4], counts [S,T], in_fov [S,T,K]}, sample ids [S][T]); the sequence
    "empty" is sequence A with n_frames = 0"""
    names = BATCHES[name]
    scenes = [scene("A" if n == "empty" else n) for n in names]
    arrays = TS.batch([{k: s[k] for k in ("n_det", "boxes", "conf", "odom", "into_prev", "into_next")} for s in scenes])
    K = arrays["boxes"].shape[2]
    extra = {"clouds": np.stack([s["clouds"] for s in scenes]), "counts": np.stack([s["counts"] for s in scenes]),
             "in_fov": np.zeros((len(scenes), T, K), np.uint8)}
    for i, (n, s) in enumerate(zip(names, scenes)):
        extra["in_fov"][i, :, :s["in_fov"].shape[1]] = s["in_fov"]
        if n == "empty":
            arrays["n_frames"][i] = 0
    return arrays, extra, [[f"{n}{i}_{t:03d}" for t in range(T)] for i, n in enumerate(names)]


@functools.lru_cache(maxsize=None)
def tracked_host(name):
    """the tracker's result for a batch, by the host restatement (read-only); cap = what always suffices"""
    from liso_amd.tracker.device_tracker import needed_capacity, track_sequences_host

    arrays, _, _ = batch(name)
    cap = max(needed_capacity(arrays["n_det"][s]) for s in range(len(arrays["n_frames"])))
    return track_sequences_host(**arrays, threshold=TS.THRESHOLD, cap=cap, margin=1e-3), cap


def config(name, **more):
    return dict(BASE, **CONFIGS[name], **more)


def needed_tracks(name):
    return int(max(tracked_host(name)[0]["track_ids"].max(), 1))
