"""The label side of `LidarDataset.assemble_sample_data` (reference liso/datasets/torch_dataset_commons.py:793-876):
`filter_objects_to_bev_non_empty` (:1013-1059), `get_object_velocity_in_obj_coords` (:1116-1145),
`create_true_where_ignore_region_mask` (:919-941), `draw_heat_regression_maps` (:190-339) in full, and `assemble_box_labels`, which
strings them together as the reference does.

Device tensors go through include/liso_label_prep.h (liso_amd/csrc/label_prep.hip) without a host synchronisation: boxes are a
padded `Shape` with `[B,K,.]` attributes and `valid [B,K]` (unbatched `[K]` is a batch of one), clouds `[B,N,C]` float32 with
`counts` int32 [B]; rows at or behind the count are never read.  Output shapes are fixed.  numpy arrays run the host path of this
file, which evaluates the same expressions in the same order.

Definitions shared by both paths (the header states them in full):
* contained points: the reference's `use_double_precision=False` branch -- the inverse pose in fp64, rounded to fp32, times the
  fp32 point, `|p_box| < 0.5 * dims` on all three axes.  The inverse is the closed form (R^T, -R^T t), not an LU factorisation.
* filter: kept = valid & has points & (0.5 * range >= |pos| on x and y) & (||pos|| < filter_range_m), evaluated in fp64.  Where the
  reference returns the kept boxes only, both paths here return the input's `[..,K]` layout compacted stably: kept boxes first, in
  their input order, `valid` marking them, every attribute of the slots behind them zero.
* `box_has_points_inside` indexes the INPUT slots of the call that computed it; feed it back only together with the same input.
* heat: per valid box exp(-(u^2 / (0.15 len) + v^2 / (0.15 wid)) / 2) in fp64 at the cell centres, u, v the offset in the box
  frame; slots with `valid` false take no part.  The reference drops them from the ground truth before it draws, but renders
  every slot of the mined boxes it is handed (:794-803), padding included; here `valid` decides in both cases.
"""
import ctypes
import math

import numpy as np
import torch

from liso_amd import _lib as L
from liso_amd.datasets.sample_prep import _mat4_mul, affine_inverse
from liso_amd.kabsch.shape_utils import Shape
from liso_amd.utils.bev_utils import get_metric_voxel_center_coords
from liso_amd.utils.device_args import as_u8, cloud3, counts_arg, is_np, opt_ptr as _p

_ATTRS = ("pos", "dims", "rot", "probs", "velo", "class_id", "difficulty")  # everything of a Shape that rides with `valid`
OCCUPANCY_THRESH = 0.01  # reference :212


# ---- host path -------------------------------------------------------------------------------------------------------------------
def box_has_points_host(pos, dims, rot, pcl):
    """numpy pos [K,3], dims [K,3], rot [K,1] and one cloud [N,>=3] float32 -> bool [K]"""
    K = pos.shape[0]
    pcl = np.asarray(pcl)
    if K == 0 or pcl.shape[0] == 0:
        return np.zeros(K, bool)
    x, y, z = (pos[:, c].astype(np.float64) for c in range(3))
    yaw = rot[:, 0].astype(np.float64)
    c, s = np.cos(yaw), np.sin(yaw)
    f32 = lambda v: v.astype(np.float32)[None]  # noqa: E731
    px, py, pz = (pcl[:, k].astype(np.float32)[:, None] for k in range(3))
    with np.errstate(invalid="ignore"):
        u = (f32(c) * px + f32(s) * py) + f32(-(c * x + s * y))
        v = (f32(-s) * px + f32(c) * py) + f32(-(c * y - s * x))
        w = pz + f32(-z)
        half = 0.5 * dims.astype(np.float64)[None]
        inside = (np.abs(u.astype(np.float64)) < half[..., 0]) & (np.abs(v.astype(np.float64)) < half[..., 1]) & \
                 (np.abs(w.astype(np.float64)) < half[..., 2])
    return inside.any(0)


def _filter_one_host(objects, pcl, bev_range_m, filter_bev, filter_range_m, has):
    if has is None:
        has = box_has_points_host(objects.pos, objects.dims, objects.rot, pcl)
    has = np.asarray(has, bool)
    assert has.shape == objects.valid.shape, (has.shape, objects.valid.shape)
    p = objects.pos.astype(np.float64)
    keep = objects.valid & has
    with np.errstate(invalid="ignore"):
        if filter_bev:
            keep = keep & (0.5 * float(bev_range_m[0]) >= np.abs(p[:, 0])) & (0.5 * float(bev_range_m[1]) >= np.abs(p[:, 1]))
        if filter_range_m is not None:
            keep = keep & (np.sqrt((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2]) < float(filter_range_m))
    n = int(keep.sum())
    out = {"valid": np.arange(keep.shape[0]) < n}
    for k in _ATTRS:
        v = getattr(objects, k)
        if v is not None:
            o = np.zeros_like(v)
            o[:n] = v[keep]
            out[k] = o
    return Shape(**out), has


def filter_objects_host(objects, pcl, counts=None, *, bev_range_m, filter_bev=True, filter_range_m=None, box_has_points_inside=None):
    """numpy `Shape` [K] with one cloud [N,C], or [B,K] with clouds [B,N,C] and `counts` -> (Shape, has_points), same layout"""
    if objects.valid.ndim == 1:
        n = pcl.shape[0] if counts is None else int(np.asarray(counts).reshape(-1)[0])
        return _filter_one_host(objects, pcl[:max(n, 0)], bev_range_m, filter_bev, filter_range_m, box_has_points_inside)
    res = []
    for b in range(objects.valid.shape[0]):
        n = pcl.shape[1] if counts is None else max(int(counts[b]), 0)
        res.append(_filter_one_host(objects[b], pcl[b, :n], bev_range_m, filter_bev, filter_range_m,
                                    None if box_has_points_inside is None else box_has_points_inside[b]))
    shape = Shape(**{k: np.stack([getattr(r[0], k) for r in res]) for k in _ATTRS + ("valid",)})
    return shape, np.stack([r[1] for r in res])


def object_velocity_host(odom_ta_tb, obj_pose_ta, obj_pose_tb):
    """numpy fp64: odom [4,4] with poses [K,4,4], or [B,4,4] with [B,K,4,4] -> [.., K, 3]"""
    O, A, Bm = (np.asarray(v, np.float64) for v in (odom_ta_tb, obj_pose_ta, obj_pose_tb))
    eye = np.eye(4)
    with np.errstate(invalid="ignore", divide="ignore"):
        M = (_mat4_mul(Bm, affine_inverse(A)) - eye) - (affine_inverse(O)[..., None, :, :] - eye)
        p = [A[..., 0, 3], A[..., 1, 3], 0.0, 1.0]
        f = [((M[..., r, 0] * p[0] + M[..., r, 1] * p[1]) + M[..., r, 2] * p[2]) + M[..., r, 3] * p[3] for r in range(3)]
        return np.stack([((A[..., r, 0] * f[0] + A[..., r, 1] * f[1]) + A[..., r, 2] * f[2]) + A[..., r, 3] * 0.0 for r in range(3)], -1)


def _cell_centers(grid_size, bev_range_m):
    H, W = int(grid_size[0]), int(grid_size[1])
    c = get_metric_voxel_center_coords(np.float64(bev_range_m[0]), np.float64(bev_range_m[1]), np.array([H, W]))
    return c[..., 0], c[..., 1]  # [H,W] each


def _ignore_mask_one_host(boxes, grid_size, bev_range_m):
    px, py = _cell_centers(grid_size, bev_range_m)
    mask = np.zeros(px.shape, bool)
    for k in np.flatnonzero(boxes.valid):
        x, y = float(boxes.pos[k, 0]), float(boxes.pos[k, 1])
        c, s = math.cos(float(boxes.rot[k, 0])), math.sin(float(boxes.rot[k, 0]))
        hx, hy = 0.5 * float(boxes.dims[k, 0]), 0.5 * float(boxes.dims[k, 1])
        u = (c * px + s * py) - (c * x + s * y)
        v = (c * py - s * px) - (c * y - s * x)
        mask |= (-hx < u) & (u < hx) & (-hy < v) & (v < hy)
    return mask


def _rot_channels(box_pred_cfg):
    method = box_pred_cfg.rotation_representation.method
    if method == "vector":
        return 2
    if method in ("direct", "class_bins"):
        return 1
    raise NotImplementedError(method)


def _log_dims(box_pred_cfg):
    method = box_pred_cfg.dimensions_representation.method
    if method == "predict_abs_size":
        return False
    if method == "predict_log_size":
        assert box_pred_cfg.activations.dims == "exp", box_pred_cfg.activations.dims
        return True
    raise NotImplementedError(method)


def _check_pos_method(box_pred_cfg):
    if box_pred_cfg.position_representation.method not in ("global_absolute", "local_relative_offset"):
        raise NotImplementedError(box_pred_cfg.position_representation.method)


def _draw_one_host(boxes, grid_size, bev_range_m, rot_ch, log_dims, scale, normalize_gaussian):
    H, W = int(grid_size[0]), int(grid_size[1])
    maps = {"probs": np.zeros((H, W, 1), np.float32), "dims": np.zeros((H, W, 3), np.float32), "pos": np.zeros((H, W, 3), np.float32),
            "rot": np.zeros((H, W, rot_ch), np.float32), "velo": np.zeros((H, W, 1), np.float32), "center_bool_mask": np.zeros((H, W), bool)}
    idx = np.flatnonzero(boxes.valid)
    if idx.size == 0:
        return maps
    assert boxes.velo.shape[-1] == 1, boxes.velo.shape
    px, py = _cell_centers(grid_size, bev_range_m)
    pos, dims, yaw = (getattr(boxes, k)[idx].astype(np.float64) for k in ("pos", "dims", "rot"))
    velo = boxes.velo[idx].astype(np.float64)
    c, s = np.cos(yaw[:, 0])[:, None, None], np.sin(yaw[:, 0])[:, None, None]
    dx, dy = px[None] - pos[:, 0, None, None], py[None] - pos[:, 1, None, None]
    u, v = dx * c + dy * s, dy * c - dx * s
    vl, vw = (0.15 * dims[:, 0])[:, None, None], (0.15 * dims[:, 1])[:, None, None]
    heat = np.exp(-((u * u) / vl + (v * v) / vw) / 2.0)
    if normalize_gaussian:
        two_pi = 2.0 * 3.141592653589793
        heat = heat / np.sqrt((two_pi * two_pi) * (vl * vw))
    else:
        heat = heat / np.maximum(heat.max(axis=(-1, -2), keepdims=True), 1e-5)
    occupied = heat > OCCUPANCY_THRESH
    scaled = heat if scale is None else np.asarray(scale, np.float64).reshape(-1)[idx][:, None, None] * heat
    best = scaled.max(0)
    win = ((scaled == best[None]) & occupied)[..., None].astype(np.float64)
    attr = {"dims": np.log(dims) if log_dims else dims, "pos": pos,
            "rot": np.concatenate([np.sin(yaw), np.cos(yaw)], -1) if rot_ch == 2 else yaw, "velo": velo}
    maps["probs"] = best[..., None].astype(np.float32)
    for k, a in attr.items():
        acc = np.zeros((H, W, a.shape[-1]))
        for q in range(idx.size):  # in box order, as the device adds them
            acc = acc + win[q] * a[q][None, None]
        maps[k] = acc.astype(np.float32)
    rng = np.array([float(bev_range_m[0]), float(bev_range_m[1])])
    cell = (((pos[:, :2] + 0.5 * rng) / rng) * np.array([float(H), float(W)])).astype(np.int32)
    cell = np.maximum(np.minimum(cell, np.array([H - 1, W - 1])), 0)
    maps["center_bool_mask"][cell[:, 0], cell[:, 1]] = True
    return maps


# ---- device path -----------------------------------------------------------------------------------------------------------------
class AttrJob(ctypes.Structure):
    """mirror of liso_box_attr_job (include/liso_label_prep.h)"""
    _fields_ = [("src", ctypes.c_void_p), ("dst", ctypes.c_void_p), ("row_bytes", ctypes.c_int)]


class FilterCfg(ctypes.Structure):
    """mirror of liso_box_filter_cfg"""
    _fields_ = [("batch", ctypes.c_int), ("n_boxes", ctypes.c_int), ("filter_bev", ctypes.c_int), ("filter_range", ctypes.c_int),
                ("range_x", ctypes.c_double), ("range_y", ctypes.c_double), ("filter_range_m", ctypes.c_double)]


class TargetsExCfg(ctypes.Structure):
    """mirror of liso_targets_ex_cfg"""
    _fields_ = [("batch", ctypes.c_int), ("n_boxes", ctypes.c_int), ("h", ctypes.c_int), ("w", ctypes.c_int), ("rot_channels", ctypes.c_int),
                ("log_dims", ctypes.c_int), ("normalize_gaussian", ctypes.c_int), ("reserved", ctypes.c_int), ("range_x", ctypes.c_double),
                ("range_y", ctypes.c_double)]


MAX_ATTRS = 8  # LISO_LABEL_MAX_ATTRS


def _device_shape(shape, name="boxes"):
    """a Shape of device tensors, [K] or [B,K] -> (the [B,K] view of it, whether it came unbatched)"""
    if not isinstance(shape, Shape) or not torch.is_tensor(shape.pos):
        raise L.LisoHipError(f"{name} must be a Shape of numpy arrays or of device tensors")
    L.require_cuda(shape.pos)
    unb = shape.valid.dim() == 1
    if shape.valid.dim() not in (1, 2) or shape.pos.shape[-1] != 3 or shape.dims.shape[-1] != 3:
        raise L.LisoHipError(f"{name} must be [K] or [B,K] with pos [..,3] and dims [..,3]")
    return (shape[None] if unb else shape), unb


def _geometry(s):
    """fp64 contiguous pos [B,K,3], dims [B,K,3], rot [B,K], valid uint8 [B,K] of a batched device Shape"""
    pos, dims = s.pos.to(torch.float64).contiguous(), s.dims.to(torch.float64).contiguous()
    rot = (s.rot[..., 0] if s.rot is not None and s.rot.shape[-1] > 0 else torch.zeros_like(s.pos[..., 0])).to(torch.float64).contiguous()
    return pos, dims, rot, as_u8(s.valid, convert=True)


def _cloud(pcl, counts, B):
    p3 = cloud3(pcl, allow_empty_batch=True)
    if p3.shape[0] != B:
        raise L.LisoHipError(f"pcl holds {p3.shape[0]} clouds for {B} box sets")
    return p3, counts_arg(counts, p3)


def box_has_points_flags(objects, pcl, counts=None):
    """device: uint32 [B,K], non-zero where the box holds a point of its cloud (entry 1 of include/liso_label_prep.h)"""
    s, _ = _device_shape(objects)
    B, K = s.valid.shape
    pos, dims, rot, _ = _geometry(s)
    p3, counts = _cloud(pcl, counts, B)
    flags = torch.empty((B, K), dtype=torch.int32, device=pos.device)
    with torch.cuda.device(pos.device):
        L.check(L.lib().liso_box_has_points_f32(B, K, p3.shape[1], p3.shape[2], _p(pos), _p(dims), _p(rot), _p(p3), _p(counts), _p(flags),
                                                L.stream_ptr()), "box has points")
    return flags


def _filter_device(objects, pcl, counts, bev_range_m, filter_bev, filter_range_m, has):
    s, unb = _device_shape(objects)
    B, K = s.valid.shape
    dev = s.pos.device
    pos, _, _, valid = _geometry(s)
    flags = None
    if has is None:
        flags = box_has_points_flags(s, pcl, counts)
    else:
        if not torch.is_tensor(has) or not has.is_cuda or has.numel() != B * K or has.dtype not in (torch.bool, torch.uint8):
            raise L.LisoHipError("box_has_points_inside must be a bool device tensor with the shape of objects.valid")
        has = as_u8(has.reshape(B, K))
    out, jobs, keep_alive = {}, (AttrJob * MAX_ATTRS)(), []
    n = 0
    for k in _ATTRS:
        v = getattr(s, k)
        if v is None:
            continue
        v = v.contiguous()
        row = v.shape[-1] * v.element_size()
        if v.dim() != 3 or tuple(v.shape[:2]) != (B, K) or row % 4:
            raise L.LisoHipError(f"attribute {k}: expected [B,K,c] with 4- or 8-byte elements, got {tuple(v.shape)} {v.dtype}")
        out[k] = torch.empty(tuple(v.shape), dtype=v.dtype, device=dev)
        keep_alive.append(v)
        jobs[n] = AttrJob(v.data_ptr(), out[k].data_ptr(), row)
        n += 1
    out_valid = torch.empty((B, K), dtype=torch.uint8, device=dev)
    has_out = torch.empty((B, K), dtype=torch.uint8, device=dev)
    cfg = FilterCfg(B, K, int(bool(filter_bev)), int(filter_range_m is not None), float(bev_range_m[0]), float(bev_range_m[1]),
                    float(filter_range_m) if filter_range_m is not None else 0.0)
    with torch.cuda.device(dev):
        L.check(L.lib().liso_filter_boxes(ctypes.byref(cfg), _p(pos), _p(valid), _p(flags), _p(has), jobs, n, _p(out_valid), _p(has_out),
                                          L.stream_ptr()), "filter boxes")
    res = Shape(valid=out_valid.view(torch.bool), **out)
    has_out = has_out.view(torch.bool)
    return (res[0], has_out[0]) if unb else (res, has_out)


def filter_objects_to_bev_non_empty(objects, pcl, counts=None, *, bev_range_m, filter_bev=True, filter_range_m=None,
                                    box_has_points_inside=None):
    """reference :1013-1059 -> (objects, box_has_points_inside).  `objects` keeps its `[..,K]` layout: the kept boxes first, in input
    order, `valid` marking them, the slots behind them zero.  `box_has_points_inside` (bool [..,K]) is returned in the slot order of
    the INPUT of this call and may be passed to a second call on the same input, as the reference's second call does.  A sample
    without a valid box comes back as padding only.  `pcl` is the cloud itself ([N,C] / [B,N,C], x y z first), not its homogeneous
    form."""
    if is_np(objects.pos):
        return filter_objects_host(objects, pcl, counts, bev_range_m=bev_range_m, filter_bev=filter_bev, filter_range_m=filter_range_m,
                                   box_has_points_inside=box_has_points_inside)
    return _filter_device(objects, pcl, counts, bev_range_m, filter_bev, filter_range_m, box_has_points_inside)


def object_velocity_in_obj_coords(odom_ta_tb, obj_pose_ta, obj_pose_tb):
    """reference :1116-1145 -- fp64 [B,K,3] (numpy: also [K,3] from an unbatched odometry): the non-rigid flow of every object's
    origin, rotated by its pose at ta; the source of `Shape.velo` for tracked ground truth"""
    if is_np(obj_pose_ta):
        return object_velocity_host(odom_ta_tb, obj_pose_ta, obj_pose_tb)
    for t in (odom_ta_tb, obj_pose_ta, obj_pose_tb):
        if not torch.is_tensor(t):
            raise L.LisoHipError("odometry and poses must all be numpy arrays or all be device tensors")
        L.require_cuda(t)
    unb = obj_pose_ta.dim() == 3
    A = (obj_pose_ta[None] if unb else obj_pose_ta).to(torch.float64).contiguous()
    Bm = (obj_pose_tb[None] if unb else obj_pose_tb).to(torch.float64).contiguous()
    O = odom_ta_tb.to(torch.float64).reshape(-1, 16).contiguous()
    if A.dim() != 4 or A.shape[-2:] != (4, 4) or A.shape != Bm.shape or O.shape[0] != A.shape[0]:
        raise L.LisoHipError(f"expected odom [B,4,4] and poses [B,K,4,4], got {tuple(odom_ta_tb.shape)} {tuple(obj_pose_ta.shape)} "
                             f"{tuple(obj_pose_tb.shape)}")
    B, K = A.shape[:2]
    out = torch.empty((B, K, 3), dtype=torch.float64, device=A.device)
    with torch.cuda.device(A.device):
        L.check(L.lib().liso_object_velocity_f64(B, K, _p(O), _p(A), _p(Bm), _p(out), L.stream_ptr()), "object velocity")
    return out[0] if unb else out


def create_true_where_ignore_region_mask(ignore_boxes, grid_size, bev_range_m):
    """reference :919-941 -- bool [H,W] / [B,H,W]: true where a cell centre lies strictly inside a valid ignore box"""
    H, W = int(grid_size[0]), int(grid_size[1])
    if is_np(ignore_boxes.pos):
        if ignore_boxes.valid.ndim == 1:
            return _ignore_mask_one_host(ignore_boxes, (H, W), bev_range_m)
        return np.stack([_ignore_mask_one_host(ignore_boxes[b], (H, W), bev_range_m) for b in range(ignore_boxes.valid.shape[0])])
    s, unb = _device_shape(ignore_boxes, "ignore_boxes")
    B, K = s.valid.shape
    pos, dims, rot, valid = _geometry(s)
    mask = torch.empty((B, H, W), dtype=torch.uint8, device=pos.device)
    with torch.cuda.device(pos.device):
        L.check(L.lib().liso_ignore_region_mask(B, K, H, W, float(bev_range_m[0]), float(bev_range_m[1]), _p(pos), _p(dims), _p(rot),
                                                _p(valid), _p(mask), L.stream_ptr()), "ignore region mask")
    mask = mask.view(torch.bool)
    return mask[0] if unb else mask


def draw_heat_regression_maps(boxes, grid_size, bev_range_m, box_pred_cfg, per_obj_prob_scale=None, normalize_gaussian=False):
    """reference :190-339 -- dict(probs [..,H,W,1], dims [..3], pos [..3], rot [..2 | 1], velo [..1] float32, center_bool_mask bool
    [..,H,W]) for a `Shape` [K] / [B,K]; `per_obj_prob_scale` [..,K,1].  The occupancy `heat > 0.01` is taken before the scale, the
    hottest box of a cell by the scaled heat."""
    rot_ch, log_dims = _rot_channels(box_pred_cfg), _log_dims(box_pred_cfg)
    _check_pos_method(box_pred_cfg)
    if per_obj_prob_scale is not None:
        assert not normalize_gaussian
        assert per_obj_prob_scale.shape[-1] == 1, per_obj_prob_scale.shape
    H, W = int(grid_size[0]), int(grid_size[1])
    if is_np(boxes.pos):
        if boxes.valid.ndim == 1:
            return _draw_one_host(boxes, (H, W), bev_range_m, rot_ch, log_dims, per_obj_prob_scale, normalize_gaussian)
        per = [_draw_one_host(boxes[b], (H, W), bev_range_m, rot_ch, log_dims,
                              None if per_obj_prob_scale is None else per_obj_prob_scale[b], normalize_gaussian)
               for b in range(boxes.valid.shape[0])]
        return {k: np.stack([m[k] for m in per]) for k in per[0]}
    s, unb = _device_shape(boxes)
    B, K = s.valid.shape
    pos, dims, rot, valid = _geometry(s)
    dev = pos.device
    if s.velo.shape[-1] != 1:
        raise L.LisoHipError(f"velo must be [..,K,1], got {tuple(s.velo.shape)}")
    velo = s.velo[..., 0].to(torch.float64).contiguous()
    scale = None
    if per_obj_prob_scale is not None:
        if not torch.is_tensor(per_obj_prob_scale) or per_obj_prob_scale.numel() != B * K:
            raise L.LisoHipError("per_obj_prob_scale must be a device tensor [..,K,1]")
        L.require_cuda(per_obj_prob_scale)
        scale = per_obj_prob_scale.reshape(B, K).to(torch.float64).contiguous()
    box_max = torch.empty((B, max(K, 1)), dtype=torch.float64, device=dev)
    out = {"probs": torch.empty((B, H, W, 1), dtype=torch.float32, device=dev), "dims": torch.empty((B, H, W, 3), dtype=torch.float32, device=dev),
           "pos": torch.empty((B, H, W, 3), dtype=torch.float32, device=dev),
           "rot": torch.empty((B, H, W, rot_ch), dtype=torch.float32, device=dev),
           "velo": torch.empty((B, H, W, 1), dtype=torch.float32, device=dev)}
    mask = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
    cfg = TargetsExCfg(B, K, H, W, rot_ch, int(log_dims), int(bool(normalize_gaussian)), 0, float(bev_range_m[0]), float(bev_range_m[1]))
    with torch.cuda.device(dev):
        L.check(L.lib().liso_render_center_targets_ex_f32(ctypes.byref(cfg), _p(pos), _p(dims), _p(rot), _p(velo), _p(scale), _p(valid),
                                                          _p(box_max), _p(out["probs"]), _p(out["dims"]), _p(out["pos"]), _p(out["rot"]),
                                                          _p(out["velo"]), _p(mask), L.stream_ptr()), "render center targets")
    out["center_bool_mask"] = mask.view(torch.bool)
    return {k: v[0] for k, v in out.items()} if unb else out


# ---- the label half of assemble_sample_data -----------------------------------------------------------------------------------------
def select_centermaps_target_confidence(cfg, gt_boxes):
    """reference :904-912"""
    target = cfg.loss.supervised.centermaps.confidence_target
    if target != "gaussian":
        raise NotImplementedError(target)
    return np.ones_like(gt_boxes.probs) if is_np(gt_boxes.probs) else torch.ones_like(gt_boxes.probs)


def assemble_box_labels(sample, *, cfg, gt_boxes, gt_object_is_movable=None, src_key="ta", target_key="tb", counts=None,
                        centermaps_grid_size=None, nusc_range_m=50.0):
    """reference :793-876 on a sample dictionary, in place, as one capturable call (no host synchronisation on device tensors).

    `sample[f"pcl_full_no_ground_{src_key}"]` is the cloud the boxes are tested against ([N,C] / [B,N,C] with `counts`).  `gt_boxes`
    is what the dataset's `extract_boxes_for_timestamp` returns and `gt_object_is_movable` its `object_is_movable` per box (bool
    [..,K]; None: every box); both stay with the caller because they are dataset specific.  Writes
      mined.boxes, mined.centermaps_{probs,dims,pos,rot,velo,center_bool_mask}   when `mined.objects_<src_key>` is present
      gt.boxes_nusc (non-empty, within `nusc_range_m`), gt.boxes (non-empty, inside the BEV range)
      gt.centermaps_*  and, with `gt.kitti_ignore_region_boxes_<src_key>`, gt.ignore_region_is_true_mask
    the maps only for centerpoint / transfusion with `loss.supervised.centermaps.active`, as the reference does."""
    name = cfg.network.name
    bev_range_m = np.asarray(cfg.data.bev_range_m, np.float32)
    if centermaps_grid_size is None:
        from liso_amd.networks.simple_net.simple_net import get_centermaps_output_grid_size

        centermaps_grid_size = get_centermaps_output_grid_size(cfg, np.array(cfg.data.img_grid_size))
    grid = None if centermaps_grid_size is None else (int(centermaps_grid_size[0]), int(centermaps_grid_size[1]))

    def target_grid():
        if grid is None:
            raise ValueError(f"no centermaps grid is defined for network {name!r}: pass centermaps_grid_size")
        return grid

    if "mined" in sample:
        mined_boxes = sample["mined"].pop(f"objects_{src_key}", None)
        if mined_boxes is not None:
            sample["mined"]["boxes"] = mined_boxes
            if name not in ("pointrcnn", "pointpillars"):
                ones = np.ones_like(mined_boxes.probs) if is_np(mined_boxes.probs) else torch.ones_like(mined_boxes.probs)
                for k, v in draw_heat_regression_maps(mined_boxes, target_grid(), bev_range_m, cfg.box_prediction, per_obj_prob_scale=ones).items():
                    sample["mined"][f"centermaps_{k}"] = v
        sample["mined"].pop(f"objects_{target_key}", None)
    gt = sample.setdefault("gt", {})
    boxes = gt_boxes.clone()
    if gt_object_is_movable is not None:
        boxes.valid = boxes.valid & gt_object_is_movable
    pcl = sample[f"pcl_full_no_ground_{src_key}"]
    gt["boxes_nusc"], has_points = filter_objects_to_bev_non_empty(boxes, pcl, counts, bev_range_m=bev_range_m, filter_bev=False,
                                                                  filter_range_m=nusc_range_m)
    gt["boxes"], _ = filter_objects_to_bev_non_empty(boxes, pcl, counts, bev_range_m=bev_range_m, box_has_points_inside=has_points)
    gt.pop("objects", None)
    if name in ("centerpoint", "transfusion") and cfg.loss.supervised.centermaps.active:
        scale = select_centermaps_target_confidence(cfg, gt["boxes"])
        for k, v in draw_heat_regression_maps(gt["boxes"], target_grid(), bev_range_m, cfg.box_prediction, per_obj_prob_scale=scale).items():
            gt[f"centermaps_{k}"] = v
        ignore = gt.get(f"kitti_ignore_region_boxes_{src_key}")
        if ignore is not None:
            gt["ignore_region_is_true_mask"] = create_true_where_ignore_region_mask(ignore, target_grid(), bev_range_m)
    return sample
