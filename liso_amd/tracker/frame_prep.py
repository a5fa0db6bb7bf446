"""Detections -> tracker tables on the device (include/liso_frame_prep.h, csrc/frame_prep.hip): the per-frame body of
`track_boxes_on_data_sequence` between NMS and `simple_tracker.update` (liso/tracker/tracking.py:745-1017) for every frame of many
padded sequences in one call -- BEV-boundary and point-count filters, the annotated-field-of-view flag, the mean flow per box, the
poses propagated one frame forward and back, the alignment of a box with its motion, and the padding of the result.

* `prepare_tracker_frames`       the batched call on device tensors -> `TrackerFrames` (no synchronisation, graph-capturable)
* `prepare_tracker_frames_host`  the same contract in numpy, step by step: the yardstick of the device tests
* `TrackerFrames.track`          hands the tables to `track_sequences`; `in_fov` is what `mine_tracked_sequences` takes
"""
import ctypes
import dataclasses

import numpy as np
import torch

from liso_amd import _lib as L
from liso_amd.kabsch.shape_utils import UNKNOWN_CLASS_ID, Shape
from liso_amd.tracker.device_tracker import TrackedSequences, track_sequences

MAX_BOX, CHUNK = 1024, 2048  # LISO_FRAME_PREP_MAX_BOX, LISO_FRAME_PREP_CHUNK
# the camera's opening angles of count_box_points_in_kitti_annotated_fov (liso/eval/eval_ours.py:98-107)
KITTI_CAM_MIN_OPENING_ANGLE_DEG, KITTI_CAM_MAX_OPENING_ANGLE_DEG = -41.95, 40.16
FIELDS = ("n_det", "boxes", "rot", "conf", "velo", "into_prev", "into_next", "in_fov", "src", "n_points", "mean_flow", "dropped_bev",
          "dropped_points", "overflow")


# ---- host restatement ------------------------------------------------------------------------------------------------------------
def _inverse_poses(b):
    """boxes float32 [K,7] -> the rows x, y, z of inv(sensor_T_box) as float64 [K,3,4] (closed form of the yaw-only pose)"""
    x, y, z, yaw = (b[:, i].astype(np.float64) for i in (0, 1, 2, 6))
    c, s, o, l = np.cos(yaw), np.sin(yaw), np.zeros_like(yaw), np.ones_like(yaw)
    return np.stack([np.stack([c, s, o, -(c * x + s * y)], -1), np.stack([-s, c, o, s * x - c * y], -1), np.stack([o, o, l, -z], -1)], 1)


def _inside(b, pts, precision, face_margin=None):
    """bool [N,K]: points float32 [N,3] inside boxes float32 [K,7].  precision 0: fp64 product rounded to fp32
    (get_points_in_boxes_mask); 1: inverse rounded to fp32, fp32 product (Shape.get_points_in_box_bool_mask).  With `face_margin` no
    point may lie within that distance of a box's surface."""
    inv = _inverse_poses(b)
    if precision == 0:
        coords = (np.einsum("kij,nj->nki", inv[:, :, :3], pts.astype(np.float64)) + inv[None, :, :, 3]).astype(np.float32)
    else:
        inv32 = inv.astype(np.float32)
        coords = np.einsum("kij,nj->nki", inv32[:, :, :3], pts.astype(np.float32)) + inv32[None, :, :, 3]
    signed = np.abs(coords) - np.float32(0.5) * b[None, :, 3:6]  # < 0 on all three axes <=> inside
    if face_margin is not None and signed.size:
        near = np.abs(signed.max(axis=-1)) < face_margin
        assert not near.any(), ("a point within the margin of a box face", np.argwhere(near)[:4])
    return (signed < 0).all(axis=-1)


def _compose(pos, yaw):
    """Shape.get_poses: float64 [K,4,4] from positions [K,3] and headings [K]"""
    c, s = np.cos(yaw), np.sin(yaw)
    P = np.tile(np.eye(4), (len(yaw), 1, 1))
    P[:, 0, 0], P[:, 0, 1], P[:, 1, 0], P[:, 1, 1], P[:, :3, 3] = c, -s, s, c, pos
    return P


def prepare_tracker_frames_host(n_frames, n_box, boxes, conf, odom, clouds, counts, point_valid, flow, fov_clouds=None, fov_counts=None, *,
                                cap, bev_range_m, drop_boxes_on_bev_boundaries, min_points_in_box, align_predicted_boxes_using_flow,
                                is_flow_cluster_detector=False, no_align_for_displacement_below_m=0.1,
                                full_align_for_displacement_above_m=0.3, fov_min_points=None, margin=None, face_margin=None,
                                angle_margin=None, mean_flow=None):
    """numpy arrays shaped like the arguments of `prepare_tracker_frames` -> dict of numpy arrays named like the fields of
    `TrackerFrames`.  `margin`: raise when a quantity the alignment decides on -- the displacement against the two thresholds, the
    forward component against 0 where a flip is possible -- lies within it of its threshold; `face_margin` / `angle_margin`: the same
    for a point against a box's surface and against the two camera angles.  `mean_flow` [S,T,cap,3]: the device's means, row by row of
    the result, taken as given in place of the restatement's own (fp64 sums rounded to fp32)."""
    boxes, conf, odom = np.asarray(boxes, np.float32), np.asarray(conf, np.float32), np.asarray(odom, np.float64)
    S, T, P = boxes.shape[:3]
    fov_min_points = min_points_in_box if fov_min_points is None else fov_min_points
    align = bool(align_predicted_boxes_using_flow) and not is_flow_cluster_detector
    half_range = np.asarray(bev_range_m, np.float32) / np.float32(2)
    lo, hi = (np.float32(a / 180.0 * np.pi) for a in (KITTI_CAM_MIN_OPENING_ANGLE_DEG, KITTI_CAM_MAX_OPENING_ANGLE_DEG))
    res = {"n_det": np.zeros((S, T), np.int32), "boxes": np.zeros((S, T, cap, 7), np.float32), "rot": np.zeros((S, T, cap)),
           "conf": np.zeros((S, T, cap), np.float32), "velo": np.zeros((S, T, cap, 3)), "into_prev": np.zeros((S, T, cap, 4, 4)),
           "into_next": np.zeros((S, T, cap, 4, 4)), "in_fov": np.zeros((S, T, cap), np.uint8), "src": np.full((S, T, cap), -1, np.int32),
           "n_points": np.zeros((S, T, cap), np.int32), "mean_flow": np.zeros((S, T, cap, 3), np.float32),
           "dropped_bev": np.zeros((S, T), np.int32), "dropped_points": np.zeros((S, T), np.int32), "overflow": np.zeros(S, np.int32)}
    for s in range(S):
        for t in range(int(np.clip(n_frames[s], 0, T))):
            nb = int(np.clip(n_box[s][t], 0, P))
            b, cf = boxes[s, t, :nb], conf[s, t, :nb]
            n = int(np.clip(counts[s][t], 0, clouds.shape[2]))
            pts = np.asarray(clouds[s][t][:n, :3], np.float32)
            finite = np.isfinite(pts).all(axis=-1)
            # 1. BEV boundary: is_boxes_clearly_in_bev_range, fp32, dx on both axes
            bev_ok = np.ones(nb, bool)
            if drop_boxes_on_bev_boundaries:
                bev_ok = (np.abs(np.abs(b[:, :2]) - b[:, [3]] / np.float32(2)) < half_range).all(axis=-1)
            # 2. point count by the fp64-product test
            in64 = _inside(b, pts[finite], 0, face_margin)
            pts_ok = np.ones(nb, bool) if min_points_in_box <= 0 else in64.sum(axis=0) >= min_points_in_box
            keep = bev_ok & pts_ok
            res["dropped_bev"][s, t], res["dropped_points"][s, t] = (~bev_ok).sum(), (bev_ok & ~pts_ok).sum()
            # 3. annotated field of view: a flag
            in_fov = np.ones(nb, np.uint8)
            if fov_clouds is not None:
                m = int(np.clip(fov_counts[s][t], 0, fov_clouds.shape[2]))
                fp = np.asarray(fov_clouds[s][t][:m, :3], np.float32)
                fp = fp[np.isfinite(fp).all(axis=-1)]
                ang = np.arctan2(fp[:, 1], fp[:, 0])
                if angle_margin is not None:
                    assert (np.abs(ang - lo) > angle_margin).all() and (np.abs(ang - hi) > angle_margin).all(), "a point within the margin of a camera angle"
                in_fov = (_inside(b, fp[(ang >= lo) & (ang <= hi)], 0, face_margin).sum(axis=0) >= fov_min_points).astype(np.uint8)
            # 4. mean flow by the fp32-product test; point_valid gates the flow, not the count
            in32 = _inside(b, pts[finite], 1, face_margin)
            n_pts = in32.sum(axis=0).astype(np.int32)
            fl = np.asarray(flow[s][t][:n], np.float64)[finite] * (np.asarray(point_valid[s][t][:n])[finite] != 0)[:, None]
            mean = ((in32.T.astype(np.float64) @ np.where(np.isfinite(fl), fl, 0.0)) / np.maximum(n_pts, 1)[:, None]).astype(np.float32)
            kept = np.where(keep)[0]
            res["overflow"][s] += max(0, len(kept) - cap)
            kept = kept[:cap]
            k = len(kept)
            if mean_flow is not None:
                mean[kept] = np.asarray(mean_flow[s][t][:k], np.float32)
            # 5. propagated poses: F(+-mean) P
            b, cf, in_fov, n_pts, mean = b[kept], cf[kept], in_fov[kept], n_pts[kept], mean[kept]
            pos, yaw = b[:, :3].astype(np.float64), b[:, 6].astype(np.float64)
            into_next, into_prev = _compose(pos + mean.astype(np.float64), yaw), _compose(pos + (-mean).astype(np.float64), yaw)
            # 6. alignment with the motion: soft_align_box_flip_orientation_with_motion_trafo
            rot, velo, yaw32 = yaw.copy(), np.zeros((k, 3)), b[:, 6].copy()
            if align and k:
                trans = (np.linalg.inv(_compose(pos, yaw)) @ odom[s, t] @ into_next)[:, :3, 3]
                disp = np.linalg.norm(trans[:, :2], axis=-1)
                if margin is not None:
                    for thr in (no_align_for_displacement_below_m, full_align_for_displacement_above_m):
                        assert (np.abs(disp - thr) > margin).all(), ("a displacement within the margin of a threshold", s, t, disp, thr)
                    can_flip = disp > no_align_for_displacement_below_m - margin
                    assert (np.abs(trans[can_flip, 0]) > margin).all(), ("a forward component within the margin of 0", s, t, trans[:, 0])
                flip = (trans[:, 0] < 0.0) & (disp > no_align_for_displacement_below_m)
                trans[flip, :2] = -trans[flip, :2]
                yaw32 = np.where(flip, yaw32 + np.float32(np.pi), yaw32).astype(np.float32)
                ratio = np.clip((disp - no_align_for_displacement_below_m) / (full_align_for_displacement_above_m - no_align_for_displacement_below_m),
                                0.0, 1.0)
                rot = yaw32.astype(np.float64) + ratio * np.arctan2(trans[:, 1], trans[:, 0])
                velo[:, 0] = disp
            # 7. the kept boxes, in their order, are the frame's first rows
            r = res
            r["n_det"][s, t] = k
            r["boxes"][s, t, :k, :6], r["boxes"][s, t, :k, 6], r["rot"][s, t, :k], r["conf"][s, t, :k] = b[:, :6], rot.astype(np.float32), rot, cf
            r["velo"][s, t, :k], r["into_prev"][s, t, :k], r["into_next"][s, t, :k] = velo, into_prev, into_next
            r["in_fov"][s, t, :k], r["src"][s, t, :k], r["n_points"][s, t, :k], r["mean_flow"][s, t, :k] = in_fov, kept, n_pts, mean
    return res


# ---- device ------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class TrackerFrames:
    """the result tables of `prepare_tracker_frames` (include/liso_frame_prep.h), device tensors, `cap` rows per frame; `n_frames`,
    `odom` and `raw_boxes` are the call's own arguments, kept for `track` and `to_raw_boxes_db`"""
    n_det: torch.Tensor
    boxes: torch.Tensor
    rot: torch.Tensor
    conf: torch.Tensor
    velo: torch.Tensor
    into_prev: torch.Tensor
    into_next: torch.Tensor
    in_fov: torch.Tensor
    src: torch.Tensor
    n_points: torch.Tensor
    mean_flow: torch.Tensor
    dropped_bev: torch.Tensor
    dropped_points: torch.Tensor
    overflow: torch.Tensor
    n_frames: torch.Tensor
    odom: torch.Tensor
    raw_boxes: torch.Tensor

    def track(self, threshold, cap) -> TrackedSequences:
        """the sequences' tracks: `track_sequences` on these tables (threshold = box_matching_threshold_m, cap = its rows per frame)"""
        return track_sequences(self.n_frames, self.n_det, self.boxes, self.conf, self.odom, self.into_prev, self.into_next, threshold, cap)

    def to_raw_boxes_db(self, sample_ids):
        """sample_ids[s][t]: the name of frame t of sequence s -> raw_boxes_db in the reference's layout (tracking.py:841-853): for every
        frame with a row in the annotated field of view, db[name] = {"lidar_T_box": float64 [n,4,4], "raw_box": the `__dict__` of a numpy
        Shape [n]} of those rows -- the boxes as detected, before the alignment turns them.  The one place that copies to the host."""
        S, T, cap = self.src.shape
        raw = self.raw_boxes.reshape(S, T, -1, 7).gather(2, self.src.clamp(min=0).long()[..., None].expand(-1, -1, -1, 7))
        packed = torch.cat([raw.double(), self.conf.double()[..., None], self.in_fov.double()[..., None]], dim=-1).reshape(-1)
        host = torch.cat([packed, self.n_det.double().reshape(-1)]).cpu().numpy()  # (fp32 and small integers: exact in fp64)
        rows, n_det = host[:S * T * cap * 9].reshape(S, T, cap, 9), host[S * T * cap * 9:].reshape(S, T).astype(np.int64)
        db = {}
        for s in range(S):
            for t in range(T):
                r = rows[s, t, :n_det[s, t]]
                r = r[r[:, 8] != 0].astype(np.float32)
                if len(r) == 0:
                    continue
                name = sample_ids[s][t]
                assert name not in db, f"overwriting occurs for {name}!"
                box = Shape(pos=r[:, :3].copy(), dims=r[:, 3:6].copy(), rot=r[:, 6:7].copy(), probs=r[:, 7:8].copy(), valid=np.ones(len(r), bool),
                            class_id=np.full((len(r), 1), UNKNOWN_CLASS_ID, np.int32))
                db[name] = {"lidar_T_box": box.get_poses(), "raw_box": box.__dict__}
        return db


@torch.no_grad()
def prepare_tracker_frames(n_frames, n_box, boxes, conf, odom, clouds, counts, point_valid, flow, fov_clouds=None, fov_counts=None, *, cap,
                           bev_range_m, drop_boxes_on_bev_boundaries, min_points_in_box, align_predicted_boxes_using_flow,
                           is_flow_cluster_detector=False, no_align_for_displacement_below_m=0.1, full_align_for_displacement_above_m=0.3,
                           fov_min_points=None) -> TrackerFrames:
    """n_frames int32 [S], n_box int32 [S,T], boxes float32 [S,T,P,7], conf float32 [S,T,P], odom float64 [S,T,4,4], clouds float32
    [S,T,N,C] with counts int32 [S,T], point_valid uint8 [S,T,N], flow float32 [S,T,N,3], optionally fov_clouds float32 [S,T,Nf,Cf] with
    fov_counts int32 [S,T] (device tensors, include/liso_frame_prep.h); the keyword arguments are the reference's configuration values
    (tracking_cfg.*, cfg.data.bev_range_m) and `cap`, the rows per frame of the result.  At most three launches, nothing is read back:
    the caller looks at `overflow` when it wants to know whether `cap` was enough."""
    L.require_cuda(n_frames, n_box, boxes, conf, odom, clouds, counts, point_valid, flow)
    S, T, P = boxes.shape[:3]
    N, C = clouds.shape[2:]
    assert boxes.shape == (S, T, P, 7) and boxes.dtype == torch.float32, (boxes.shape, boxes.dtype)
    assert conf.shape == (S, T, P) and conf.dtype == torch.float32, (conf.shape, conf.dtype)
    assert n_frames.shape == (S,) and n_box.shape == (S, T) and counts.shape == (S, T) and n_frames.dtype == n_box.dtype == counts.dtype == torch.int32
    assert odom.shape == (S, T, 4, 4) and odom.dtype == torch.float64, (odom.shape, odom.dtype)
    assert clouds.shape == (S, T, N, C) and clouds.dtype == torch.float32, (clouds.shape, clouds.dtype)
    assert point_valid.shape == (S, T, N) and flow.shape == (S, T, N, 3) and flow.dtype == torch.float32, (point_valid.shape, flow.shape, flow.dtype)
    assert len(bev_range_m) == 2, bev_range_m
    assert (fov_clouds is None) == (fov_counts is None), "fov_clouds and fov_counts come together"
    valid_u8 = point_valid.to(torch.uint8)
    n_frames, n_box, boxes, conf, odom, clouds, counts, valid_u8, flow = (v.contiguous() for v in (n_frames, n_box, boxes, conf, odom, clouds,
                                                                                                  counts, valid_u8, flow))
    Nf, Cf = -1, 0
    if fov_clouds is not None:
        L.require_cuda(fov_clouds, fov_counts)
        Nf, Cf = fov_clouds.shape[2:]
        assert fov_clouds.shape == (S, T, Nf, Cf) and fov_clouds.dtype == torch.float32, (fov_clouds.shape, fov_clouds.dtype)
        assert fov_counts.shape == (S, T) and fov_counts.dtype == torch.int32, (fov_counts.shape, fov_counts.dtype)
        fov_clouds, fov_counts = fov_clouds.contiguous(), fov_counts.contiguous()
    cap = int(cap)
    align = bool(align_predicted_boxes_using_flow) and not is_flow_cluster_detector
    if align:
        assert no_align_for_displacement_below_m < full_align_for_displacement_above_m, (no_align_for_displacement_below_m,
                                                                                         full_align_for_displacement_above_m)
    cfg = L.FramePrepCfg(S, T, P, cap, N, C, Nf, Cf, float(bev_range_m[0]), float(bev_range_m[1]), int(bool(drop_boxes_on_bev_boundaries)),
                       int(min_points_in_box), int(min_points_in_box if fov_min_points is None else fov_min_points), int(align),
                       float(no_align_for_displacement_below_m), float(full_align_for_displacement_above_m))
    ws_bytes = int(L.lib().liso_frame_prep_workspace_bytes(ctypes.byref(cfg)))
    if ws_bytes == 0:
        raise L.LisoHipError(f"prepare_tracker_frames: sizes refused (S={S}, T={T}, P={P}, cap={cap}, N={N}, C={C}; 1 <= P <= {MAX_BOX}, "
                             f"T, cap >= 1, S * T <= 65535, C >= 3)")
    dev = boxes.device
    new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)  # noqa: E731
    f32, f64, i32 = torch.float32, torch.float64, torch.int32
    out = {"n_det": new((S, T), i32), "boxes": new((S, T, cap, 7), f32), "rot": new((S, T, cap), f64), "conf": new((S, T, cap), f32),
           "velo": new((S, T, cap, 3), f64), "into_prev": new((S, T, cap, 4, 4), f64), "into_next": new((S, T, cap, 4, 4), f64),
           "in_fov": new((S, T, cap), torch.uint8), "src": new((S, T, cap), i32), "n_points": new((S, T, cap), i32),
           "mean_flow": new((S, T, cap, 3), f32), "dropped_bev": new((S, T), i32), "dropped_points": new((S, T), i32), "overflow": new((S,), i32)}
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    opt = lambda t: L.ptr(t) if t is not None else None  # noqa: E731
    if S > 0:
        with torch.cuda.device(dev):
            L.check(L.TIMER.launch("prepare_tracker_frames", lambda: L.lib().liso_prepare_tracker_frames(
                ctypes.byref(cfg), L.ptr(n_frames), L.ptr(n_box), L.ptr(boxes), L.ptr(conf), L.ptr(odom), L.ptr(clouds), L.ptr(counts),
                L.ptr(valid_u8), L.ptr(flow), opt(fov_clouds), opt(fov_counts), *[L.ptr(out[k]) for k in FIELDS], L.ptr(ws), ws_bytes,
                L.stream_ptr())), "prepare_tracker_frames")
    return TrackerFrames(**out, n_frames=n_frames, odom=odom, raw_boxes=boxes)
