"""Inputs for the sequence-tracker tests (tests/test_device_tracker_host.py, tests/test_gpu_device_tracker.py): the golden sequences
of tests/golden/tracker_reference.npz as the padded arrays `track_sequences` takes, and generated sequences.

A generated sequence is a set of objects on a jittered lattice (14 m apart, jitter 1 m, constant velocities of at most 0.1 m per frame,
so that objects stay more than 6 m apart over 25 frames) with a visibility table that says in which frames an object is detected.  A
detection sits within 0.1 m of its object, its two propagated poses within 0.1 m of the object one frame earlier / later; with a
matching threshold of 2 m a detection's own track is at most ~1 m away (a carried box extrapolates) and every other one more than 4 m.
`pairs` places an object 1.5 m beside another one (same velocity): when one of the two is not detected, both tracks want the other's
detection -- the competition that the order of equal confidences decides.  The margin condition (no distance within 1e-3 m of the
threshold, no two candidates of a track within 1e-3 m of each other) is asserted by `track_sequences_host(..., margin=1e-3)`, never
repaired by drawing again."""
import os

import numpy as np

THRESHOLD = 2.0
G = np.load(os.path.join(os.path.dirname(__file__), "golden", "tracker_reference.npz"))


def compose(x, y, z, yaw):
    c, s, o, l = np.cos(yaw), np.sin(yaw), np.zeros_like(x), np.ones_like(x)
    return np.stack([np.stack([c, -s, o, x], -1), np.stack([s, c, o, y], -1), np.stack([o, o, l, z], -1), np.stack([o, o, o, l], -1)], -2)


def golden_frames(tag, key):
    off = G[f"{tag}_{key}_offsets"]
    return [G[f"{tag}_{key}"][off[i]:off[i + 1]] for i in range(len(off) - 1)]


def pack(frames):
    """frames: list of dicts (pos [n,3], rot [n,1], dims [n,3], probs [n,1], into_prev / into_next [n,4,4], odom [4,4]) -> the arrays of
    one sequence: n_det [T], boxes [T,K,7], conf [T,K], odom [T,4,4], into_prev / into_next [T,K,4,4]"""
    T, K = len(frames), max(1, max(len(f["pos"]) for f in frames))
    out = {"n_det": np.zeros(T, np.int32), "boxes": np.zeros((T, K, 7), np.float32), "conf": np.zeros((T, K), np.float32),
           "odom": np.zeros((T, 4, 4)), "into_prev": np.zeros((T, K, 4, 4)), "into_next": np.zeros((T, K, 4, 4))}
    for t, f in enumerate(frames):
        n = len(f["pos"])
        out["n_det"][t] = n
        out["boxes"][t, :n] = np.concatenate([f["pos"], f["dims"], f["rot"]], axis=1)
        out["conf"][t, :n] = f["probs"][:, 0]
        out["odom"][t] = f["odom"]
        out["into_prev"][t, :n], out["into_next"][t, :n] = f["into_prev"].reshape(n, 4, 4), f["into_next"].reshape(n, 4, 4)
    return out


def golden_scene(tag):
    ins = {k: golden_frames(tag, "in_" + k) for k in ("pos", "rot", "dims", "probs", "into_prev", "into_next")}
    return pack([dict({k: v[t] for k, v in ins.items()}, odom=G[f"{tag}_in_odom"][t]) for t in range(len(ins["pos"]))])


def make_scene(vis, seed, pairs=(), noise=0.1):
    """vis: bool [T, n_obj] -> the arrays of one sequence (see `pack`); the detections of a frame come in a shuffled order"""
    vis = np.asarray(vis, bool)
    T, n_obj = vis.shape
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(max(n_obj, 1))))
    cell = np.stack(np.divmod(np.arange(n_obj), side), axis=1).astype(np.float64)
    p0 = np.concatenate([(cell - (side - 1) / 2) * 14.0 + rng.uniform(-1, 1, (n_obj, 2)), rng.uniform(-1, 1, (n_obj, 1))], axis=1)
    vel = np.concatenate([rng.uniform(-0.1, 0.1, (n_obj, 2)), np.zeros((n_obj, 1))], axis=1)
    for a, b in pairs:
        p0[b], vel[b] = p0[a] + np.array([1.5, 0.0, 0.0]), vel[a]
    yaw = rng.uniform(-np.pi, np.pi, n_obj)
    dims = rng.uniform(1.0, 5.0, (n_obj, 3)).astype(np.float32)
    odom = compose(rng.uniform(0.5, 1.5, T), rng.uniform(-0.2, 0.2, T), rng.uniform(-0.05, 0.05, T), rng.uniform(-0.05, 0.05, T))
    W = [np.eye(4)]
    for t in range(T - 1):
        W.append(W[-1] @ odom[t])

    def sensor_poses(t_sensor, objs, t_obj):
        at = p0[objs] + vel[objs] * t_obj + np.concatenate([rng.uniform(-noise, noise, (len(objs), 2)), np.zeros((len(objs), 1))], axis=1)
        assert np.abs(at).max(initial=0.0) < 500.0
        return np.linalg.inv(W[t_sensor]) @ compose(at[:, 0], at[:, 1], at[:, 2], yaw[objs])

    frames = []
    for t in range(T):
        objs = rng.permutation(np.where(vis[t])[0])
        own = sensor_poses(t, objs, t)
        frames.append({"pos": own[:, :3, 3].astype(np.float32), "rot": np.arctan2(own[:, 1, 0], own[:, 0, 0])[:, None].astype(np.float32),
                       "dims": dims[objs], "probs": rng.uniform(0.3, 1.0, (len(objs), 1)).astype(np.float32), "odom": odom[t],
                       "into_prev": sensor_poses(max(t - 1, 0), objs, t - 1), "into_next": sensor_poses(min(t + 1, T - 1), objs, t + 1)})
    return pack(frames)


def counts_vis(counts, n_obj):
    """a frame with c detections sees the first c objects"""
    return np.arange(n_obj)[None, :] < np.asarray(counts)[:, None]


def story_vis():
    """25 objects over 8 frames: 17 steady ones, then the stories the tracker has to get right (object: frames detected)
    17: 0 . 2 ....   carried once and re-detected: its hole at frame 1 is filled
    18: 0 . . 3 ...  carried twice, dead, re-detected under a new id: no fill
    19: 3 4          last - first = 1: no fill
    20: 0 1 2 . . .  lost for good
    21 / 22: a pair 1.5 m apart, 21 is missing at frame 4 (both tracks want 22's detection) and back at frame 5
    23 / 24: the same pair story, 24 missing at frame 2"""
    vis = np.zeros((8, 25), bool)
    vis[:, :17] = True
    vis[[0, 2, 3, 4, 5, 6, 7], 17] = True
    vis[[0, 3, 4, 5], 18] = True
    vis[[3, 4], 19] = True
    vis[[0, 1, 2], 20] = True
    vis[:, 21:25] = True
    vis[4, 21] = False
    vis[2, 24] = False
    return vis


STORY_PAIRS = ((21, 22), (23, 24))


def random_vis(T, n_obj, seed, p_miss=0.25):
    return np.random.default_rng(seed).uniform(size=(T, n_obj)) > p_miss


def generated_scenes():
    """name -> arrays of one sequence; together they cover T in {1, 2, 3, 6, 25} and 0, 1, 63, 64, 65, 130 detections per frame"""
    scenes = {"story": make_scene(story_vis(), 1, STORY_PAIRS)}
    scenes["T1"] = make_scene(counts_vis([5], 5), 2)
    scenes["T2"] = make_scene(counts_vis([3, 4], 4), 3)
    scenes["T3_all_lost"] = make_scene(np.array([[1, 1, 1, 0, 0, 0], [0, 0, 0, 1, 1, 1], [1, 1, 1, 1, 1, 1]], bool), 4)  # frame 1 matches nothing
    scenes["T6_counts"] = make_scene(counts_vis([64, 63, 65, 0, 130, 1], 130), 5)  # an empty frame in the middle
    scenes["T25"] = make_scene(random_vis(25, 20, 6), 6)
    scenes["T6_65"] = make_scene(random_vis(6, 65, 7, 0.1), 7)
    return scenes


def batch(scenes):
    """list of sequences -> the arrays of one call, with a leading sequence axis, padded to the longest / widest"""
    S, T, K = len(scenes), max(len(s["n_det"]) for s in scenes), max(s["boxes"].shape[1] for s in scenes)
    out = {"n_frames": np.array([len(s["n_det"]) for s in scenes], np.int32), "n_det": np.zeros((S, T), np.int32),
           "boxes": np.zeros((S, T, K, 7), np.float32), "conf": np.zeros((S, T, K), np.float32), "odom": np.zeros((S, T, 4, 4)),
           "into_prev": np.zeros((S, T, K, 4, 4)), "into_next": np.zeros((S, T, K, 4, 4))}
    for i, s in enumerate(scenes):
        t, k = s["boxes"].shape[:2]
        out["n_det"][i, :t], out["odom"][i, :t] = s["n_det"], s["odom"]
        for key in ("boxes", "conf", "into_prev", "into_next"):
            out[key][i, :t, :k] = s[key]
    return out


def run_host_class(scene, tracker, attributes=True):
    """the sequence through `update` / `run_tracker` of a tracker object (host tensors, or on `tracker.test_device`); each detection's
    attribute entry is {"uid": 1000 * frame + slot}, or no attributes are given at all"""
    import torch

    from liso_amd.kabsch.shape_utils import Shape

    dev = getattr(tracker, "test_device", "cpu")
    for t in range(len(scene["n_det"])):
        n = int(scene["n_det"][t])
        b = torch.from_numpy(scene["boxes"][t, :n]).to(dev)
        boxes = Shape(pos=b[:, :3].clone(), dims=b[:, 3:6].clone(), rot=b[:, 6:7].clone(), probs=torch.from_numpy(scene["conf"][t, :n, None]).to(dev),
                      valid=torch.ones(n, dtype=torch.bool, device=dev))
        tracker.update(boxes, torch.from_numpy(scene["into_next"][t, :n]).to(dev), torch.from_numpy(scene["into_prev"][t, :n]).to(dev),
                       torch.from_numpy(scene["odom"][t]).to(dev), [{"uid": 1000 * t + k} for k in range(n)] if attributes else None)
    tracker.run_tracker()
    return tracker
