"""Generates tests/golden/snippet_harvest_reference.npz with the reference's own python.

The cut loop of track_boxes_on_data_sequence (liso/tracker/tracking.py:1568-1610, :1848-1891) is inline in a 1,400-line function
and cannot be called.  The poses come from the reference's `Shape.get_poses`, `torch.linalg.inv` and `homogenize_pcl`; the
product, the mask and the two draws (:1541-1565, :1825-1842) are stated here in the generator's own words.  Called directly from
the reference: `decide_keep_or_drop_box`, `update_world_boxes_from_sensor_boxes`, `update_sensor_boxes_from_world_boxes`
(liso/tracker/tracking.py) and `drop_boxes_from_augmentation_db` (liso/tracker/augm_box_db_utils.py).  liso.tracker.tracking as a
whole cannot be imported here (see make_tracking_golden.py): the three functions are compiled at generation time from the reference
file's own text with the reference's Shape / torch_decompose_matrix as their globals; nothing of the reference is stored.  Absent
third-party modules are stubbed with empty modules (no arithmetic).

The generator asserts what the tests rely on, and fails loudly otherwise:
  * the reference's bound `1.1 * 0.5 * dims` on float32 dims is bitwise float32(0.55) * dims;
  * no point of the cut case lies within 1e-4 m of a bloated box face (points that do are removed from the sweeps beforehand, at
    most 1 % of them), so no membership decision hangs on the last bit of the closed-form against the LU inverse.
Run in the build container only:
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_snippet_harvest_golden.py
"""
import os
import sys
import types

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, "/root/reference")

from make_targets_golden import _Anything, cfg, import_with_stubs  # noqa: E402
from make_tracking_golden import function_from_reference_file  # noqa: E402

sys.modules["torch.utils.tensorboard"] = _Anything("torch.utils.tensorboard")  # logging only; absent from this image

T, N, C, MARGIN = 3, 2000, 5, 1e-4


def box_frame64(b7, pts):
    """fp64 coordinates of pts [n, 3] in the frame of one box"""
    c, s = np.cos(np.float64(b7[6])), np.sin(np.float64(b7[6]))
    d = pts.astype(np.float64) - b7[:3].astype(np.float64)
    return np.stack([d[:, 0] * c + d[:, 1] * s, d[:, 1] * c - d[:, 0] * s, d[:, 2]], -1)


def cut_case(Shape, homogenize_pcl, out):
    g = np.random.default_rng(11)
    pos = np.array([[10.2, 4.1, -0.8], [-14.6, 9.3, -1.0], [22.5, -18.4, -0.7], [-6.1, -25.2, -0.9], [10.9, 4.6, -0.8], [35.0, 30.0, 12.0],
                    [-14.0, 9.0, -1.0], [3.3, 15.8, -0.6]], np.float32)
    dims = np.stack([g.uniform(3.5, 5.0, 8), g.uniform(1.6, 2.2, 8), g.uniform(1.4, 1.9, 8)], -1).astype(np.float32)
    rot = g.uniform(-np.pi, np.pi, (8, 1)).astype(np.float32)
    probs = g.uniform(0.3, 1.0, (8, 1)).astype(np.float32)
    job_cloud = np.array([2, 0, 1, 0, 2, 1, 0, 2], np.int32)  # out of cloud order; jobs 0 and 4 overlap in sweep 2; job 5 is empty
    b7 = np.concatenate([pos, dims, rot], -1)
    clouds = np.full((T, N, C), np.nan, np.float32)
    counts = np.array([N, 1500, N], np.int32)
    for t in range(T):
        n = int(counts[t])
        p = np.concatenate([g.uniform(-40, 40, (n, 2)), g.uniform(-3, 2, (n, 1))], -1)
        jobs = [j for j in range(8) if job_cloud[j] == t and j != 5]
        for k, j in enumerate(jobs):  # a cluster of points in and around each box of this sweep
            m = 150
            local = g.uniform(-0.7, 0.7, (m, 3)) * dims[j]
            c, s = np.cos(rot[j, 0]), np.sin(rot[j, 0])
            p[k * m:(k + 1) * m] = np.stack([pos[j, 0] + c * local[:, 0] - s * local[:, 1], pos[j, 1] + s * local[:, 0] + c * local[:, 1],
                                             pos[j, 2] + local[:, 2]], -1)
        p = p[g.permutation(n)].astype(np.float32)
        near = np.zeros(n, bool)
        for j in range(8):
            near |= (np.abs(np.abs(box_frame64(b7[j], p)) - 0.55 * dims[j].astype(np.float64)) < MARGIN).any(-1)
        assert near.sum() <= 0.01 * n, near.sum()
        p = p[~near]
        counts[t] = p.shape[0]
        clouds[t, :p.shape[0], :3] = p
        clouds[t, :p.shape[0], 3] = g.uniform(0, 1, p.shape[0])
        clouds[t, :p.shape[0], 4] = g.uniform(0, 255, p.shape[0])  # the intensity: the LAST channel
    clouds[0, 17, 1] = np.nan  # a NaN row inside the count
    lidar_rows = g.integers(0, 64, (T, N)).astype(np.int32)

    boxes = Shape(pos=torch.from_numpy(pos), dims=torch.from_numpy(dims), rot=torch.from_numpy(rot), probs=torch.from_numpy(probs))
    pts, rows, sizes, inv = [], [], [], []
    for j in range(8):
        t = int(job_cloud[j])
        pcl_at_t = torch.from_numpy(clouds[t, :counts[t]])
        box_at_t = boxes[j]
        bound = 1.1 * 0.5 * box_at_t.dims
        assert bound.dtype == torch.float32 and np.array_equal(bound.numpy().view(np.uint32), (np.float32(0.55) * dims[j]).view(np.uint32))
        sensor_T_box = box_at_t[None].get_poses()[0]
        box_T_sensor = torch.linalg.inv(sensor_T_box)
        homog = homogenize_pcl(pcl_at_t[:, :3])
        pcl_box = torch.cat([torch.einsum("ij,nj->ni", box_T_sensor, homog.double())[:, :3].float(), pcl_at_t[:, [-1]]], dim=-1)
        inside = torch.all(torch.abs(pcl_box[:, 0:3]) <= bound, dim=-1)
        pts.append(pcl_box[inside].numpy().astype(np.float32))
        rows.append(lidar_rows[t, :counts[t]][inside.numpy()])
        sizes.append(int(inside.sum()))
        inv.append(box_T_sensor.numpy())
    assert sizes[5] == 0 and min(sizes[:5] + sizes[6:]) > 20, sizes
    shared = set(pts[0][:, 3].tolist()) & set(pts[4][:, 3].tolist())  # the intensities identify the points
    assert shared, "jobs 0 and 4 are meant to share points"
    out.update(cut_clouds=clouds, cut_counts=counts, cut_lidar_rows=lidar_rows, cut_job_cloud=job_cloud, cut_pos=pos, cut_dims=dims,
               cut_rot=rot, cut_probs=probs, cut_offsets=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64),
               cut_points=np.concatenate(pts, 0), cut_rows=np.concatenate(rows).astype(np.int32), cut_box_T_sensor=np.stack(inv))
    print("cut sizes", sizes)


def draw_case(out):
    tracks = np.array([[12, 0, 7.9, 4], [5, 3, 0.4, 5], [20, 2, 3.2, 4], [9, 11, 14.0, 3], [4, 0, 100.0, 4]], np.float64)  # len, start, dist, min age
    np.random.seed(321)
    picks = []
    for track_len, start, dist, min_age in tracks:
        track_len, start, min_age = int(track_len), int(start), int(min_age)
        num = min(max(1, (track_len // min_age) * int(dist)), min(10, track_len))
        picks.append(np.random.choice(np.arange(start=start, stop=track_len + start, step=1), size=num, replace=False))
    out["draw_tracks"], out["draw_track_seed"] = tracks, np.array(321)
    out["draw_track_sizes"] = np.array([len(p) for p in picks])
    out["draw_track_picks"] = np.concatenate(picks)
    g = np.random.default_rng(3)
    frames = [g.uniform(0.1, 1.0, n).astype(np.float32) for n in (2, 7, 3, 4, 12)]
    np.random.seed(77)
    idxs = []
    for probs in frames:
        n = probs.shape[0]
        if min(3, n) >= n:
            idxs.append(np.arange(n))
        else:
            p = probs + 1e-6
            p /= p.sum()
            idxs.append(np.random.choice(np.arange(n), size=3, p=p, replace=False))
    out["draw_box_seed"] = np.array(77)
    out["draw_box_sizes"] = np.array([f.shape[0] for f in frames])
    out["draw_box_probs"] = np.concatenate(frames)
    out["draw_box_picks"] = np.concatenate(idxs)


def mirror_case(tr, Shape, out):
    g = np.random.default_rng(8)
    n = 6
    yaw, xy = g.uniform(-np.pi, np.pi, n), g.uniform(-30, 30, (n, 2))
    w_T_s = np.tile(np.eye(4), (n, 1, 1))
    w_T_s[:, 0, 0], w_T_s[:, 0, 1], w_T_s[:, 1, 0], w_T_s[:, 1, 1] = np.cos(yaw), -np.sin(yaw), np.sin(yaw), np.cos(yaw)
    w_T_s[:, :2, 3], w_T_s[:, 2, 3] = xy, g.uniform(-0.5, 0.5, n)

    def seq(dtype):
        return Shape(pos=torch.from_numpy(g.uniform(-20, 20, (n, 3))).to(dtype), dims=torch.from_numpy(g.uniform(1.5, 5, (n, 3))).to(dtype),
                     rot=torch.from_numpy(g.uniform(-np.pi, np.pi, (n, 1))).to(dtype), probs=torch.from_numpy(g.uniform(0.2, 1, (n, 1))).to(dtype))

    sensor, world = seq(torch.float64), seq(torch.float64)
    out["mir_w_T_s"] = w_T_s
    for k in ("pos", "dims", "rot", "probs"):
        out[f"mir_sensor_{k}"], out[f"mir_world_{k}"] = getattr(sensor, k).numpy().copy(), getattr(world, k).numpy().copy()
    res = tr.update_world_boxes_from_sensor_boxes(box_sequence_sensor=sensor.clone(), box_sequence_world=world.clone(), w_T_sensor_ti=torch.from_numpy(w_T_s))
    for k in ("pos", "dims", "rot", "probs"):
        out[f"mir_to_world_{k}"] = getattr(res, k).numpy()
    res = tr.update_sensor_boxes_from_world_boxes(box_sequence_world=world.clone(), box_sequence_sensor=sensor.clone(), w_T_sensor_ti=torch.from_numpy(w_T_s))
    for k in ("pos", "dims", "rot", "probs"):
        out[f"mir_to_sensor_{k}"] = getattr(res, k).numpy()

    # keep / drop: tracks of 8 frames at 0.1 s that cover about 0, 0.5, 2 and 9 m; speed filter on / off, travel filter on / off
    tcfg = cfg({"flow_cluster_detector_min_travel_dist_filter_m": 1.5})
    keeps, dists, cases = [], [], []
    tracks = []
    for reach in (0.0, 0.5, 2.0, 9.0):
        step = reach / 7.0
        pos = np.stack([5.0 + step * np.arange(8) * 0.8, -3.0 + step * np.arange(8) * 0.6, np.full(8, -1.0)], -1) + g.normal(0, 0.01, (8, 3))
        tracks.append(np.concatenate([pos, g.uniform(-1, 1, (8, 1))], -1))
    out["keep_tracks"] = np.stack(tracks)
    for ti, trk in enumerate(tracks):
        box = Shape(pos=torch.from_numpy(trk[:, :3]), dims=torch.ones(8, 3, dtype=torch.float64) * 2.0, rot=torch.from_numpy(trk[:, 3:]),
                    probs=torch.ones(8, 1, dtype=torch.float64))
        for speed in (0.0, 1.0):
            for fcd in (False, True):
                keep, dist = tr.decide_keep_or_drop_box(tracking_cfg=tcfg, box_sequence_world_for_specific_track_id=box, min_track_obj_speed_mps=speed,
                                                        track_id=ti, time_between_frames_s=0.1, verbose=False, is_flow_cluster_detector=fcd)
                cases.append([ti, speed, float(fcd)])
                keeps.append(bool(keep))
                dists.append(float(dist))
    out["keep_cases"], out["keep_keep"], out["keep_dist"] = np.array(cases), np.array(keeps), np.array(dists)
    assert 0 < sum(keeps) < len(keeps)


def cap_case(u, Shape, out):
    g = np.random.default_rng(21)
    sizes = g.integers(2000, 9000, 14)
    probs = g.uniform(0.3, 1.0, 14).astype(np.float32)
    db = u.get_empty_augm_box_db()
    for i, n in enumerate(sizes):
        db["pcl_in_box_cosy"].append(np.zeros((n, 4), np.float32))
        db["lidar_rows"].append(np.zeros(n, np.int32))
        db["boxes"].append(Shape(pos=torch.zeros(3), dims=torch.ones(3), rot=torch.zeros(1), probs=torch.tensor([probs[i]])))
        db["box_T_sensor"].append(np.eye(4))
        db["unique_track_id"].append(i)
    max_mb = 0.5
    assert u.estimate_augm_db_size_mb(db) > max_mb
    np.random.seed(5)
    small = u.drop_boxes_from_augmentation_db(db, max_mb)
    out.update(cap_sizes=sizes, cap_probs=probs, cap_max_mb=np.array(max_mb), cap_seed=np.array(5), cap_keep=np.array(small["unique_track_id"]))
    assert 0 < len(small["unique_track_id"]) < 14


def main():
    def _imp():
        import liso.tracker.augm_box_db_utils as u
        from liso.kabsch.shape_utils import Shape
        from liso.utils.torch_transformation import homogenize_pcl, torch_decompose_matrix
        return u, Shape, homogenize_pcl, torch_decompose_matrix

    u, Shape, homogenize_pcl, torch_decompose_matrix = import_with_stubs(_imp)
    env = {"Shape": Shape, "torch_decompose_matrix": torch_decompose_matrix, "torch": torch, "np": np}
    tr = types.SimpleNamespace(**{name: function_from_reference_file("/root/reference/liso/tracker/tracking.py", name, env) for name in (
        "decide_keep_or_drop_box", "update_world_boxes_from_sensor_boxes", "update_sensor_boxes_from_world_boxes")})
    out = {}
    cut_case(Shape, homogenize_pcl, out)
    draw_case(out)
    mirror_case(tr, Shape, out)
    cap_case(u, Shape, out)
    np.savez_compressed(os.path.join(HERE, "snippet_harvest_reference.npz"), **out)
    print({k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
