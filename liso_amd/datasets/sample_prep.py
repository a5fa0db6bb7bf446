"""Per-sample preparation between ground removal and the collated batch: the geometric augmentation of the reference's
`LidarDataset.augment_sample_content` (liso/datasets/torch_dataset_commons.py:1291-1483, :1870-1899) and the BEV half of
`assemble_sample_data` (:743-902): `pillarize_bev` (:1147-1163), `add_bev_flow` (:1200-1213),
`add_bev_ground_height_occupancy_maps` (:1215-1223) and the `moving_mask` expression (:776-792).

Device tensors go through include/liso_sample_prep.h (liso_amd/csrc/sample_prep.hip) without a host synchronisation, in the
collated layout: `pcl [B,N,C]` NaN-padded plus `counts` int32 [B] (unbatched `[N,C]` is a batch of one).  numpy arrays run the
host path of this file, which evaluates the same fp64 expressions in the same order; CPU tensors are refused where only a device
path exists.  Only the random draws of `get_augmentation_transform` stay on the host.

Definitions shared by both paths:
* transform: x' = ((T00*x + T01*y) + T02*z) + T03 in fp64, rounded once to fp32; flows take the linear part; rows with a NaN
  coordinate come out NaN, rows behind the count NaN in every channel.
* crop: coordinates `((p + 0.5*range) / range) * grid` in fp64 truncated to int32 (z: range 1000 m, grid 1), inside = in the grid
  on all axes and strictly inside the height interval; kept = inside and not dropped; kept rows first, in order.
* flow_bev: the per-cell mean.  The device sums fixed-point integers (order-independent, bitwise reproducible), the host sums in
  fp64; both lie within 2^-23 * max|v| of the exact mean.
"""
import ctypes
import math

import numpy as np
import torch

from liso_amd import _lib as L
from liso_amd.kabsch.shape_utils import Shape
from liso_amd.utils.device_args import as_u8, cloud3, counts_arg, is_np, opt_ptr as _p


# ---- the random transform (host) --------------------------------------------------------------------------------------------------
def get_augmentation_transform(max_symm_rot_deg, max_sensor_pos_offset_m, max_xy_scale_delta=None):
    """reference :1870-1899 -- fp64 [4,4] = translate * rotate-z * scale.  Draws np.random.rand() in the reference's order:
    rotation, offset angle, offset length, then (only when asked for) the xy scale."""
    delta_rot_deg = -max_symm_rot_deg + 2 * np.random.rand() * max_symm_rot_deg
    offset_angle = np.random.rand() * np.pi * 2.0
    offset_m = np.random.rand() * max_sensor_pos_offset_m
    offset = offset_m * np.array([np.cos(offset_angle), np.sin(offset_angle), 0.0])
    s = 1.0 if max_xy_scale_delta is None else 1.0 + max_xy_scale_delta * (2 * np.random.rand() - 1)
    a = np.deg2rad(delta_rot_deg)
    c, sn = math.cos(a), math.sin(a)
    return np.array([[c * s, -sn * s, 0.0, offset[0]], [sn * s, c * s, 0.0, offset[1]], [0.0, 0.0, 1.0, offset[2]], [0.0, 0.0, 0.0, 1.0]])


# ---- host path -------------------------------------------------------------------------------------------------------------------
def _lin3(T, v, w):
    """rows of T applied to the fp64 columns v [N,3]: ((T_r0*x + T_r1*y) + T_r2*z) [+ T_r3 when w] -> fp64 [N,3]"""
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    out = np.empty((v.shape[0], 3))
    for r in range(3):
        acc = (T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z
        out[:, r] = acc + T[r, 3] if w else acc
    return out


def transform_cloud_host(pcl, T, flow=None):
    """numpy [N,C] float32 (and flow [N,3]) under fp64 T [4,4] -> float32 arrays; see the module text"""
    pcl = np.asarray(pcl)
    T = np.asarray(T, np.float64)
    assert T.shape == (4, 4) and pcl.ndim == 2 and pcl.shape[1] >= 3, (T.shape, pcl.shape)
    bad = np.isnan(pcl[:, :3]).any(-1)
    out = pcl.astype(np.float32, copy=True)
    with np.errstate(invalid="ignore"):
        out[:, :3] = _lin3(T, pcl[:, :3].astype(np.float64), True).astype(np.float32)
    out[bad, :3] = np.nan
    if flow is None:
        return out
    with np.errstate(invalid="ignore"):
        fo = _lin3(T, np.asarray(flow)[:, :3].astype(np.float64), False).astype(np.float32)
    fo[bad] = np.nan
    return out, fo


def affine_inverse(M):
    """closed-form inverse of an affine fp64 [..,4,4]: adjugate of the 3x3 block over its determinant, and -A^-1 t"""
    M = np.asarray(M, np.float64)
    a, b, c, d, e, f, g, h, k = (M[..., i, j] for i in range(3) for j in range(3))
    cof = [e * k - f * h, c * h - b * k, b * f - c * e, f * g - d * k, a * k - c * g, c * d - a * f, d * h - e * g, b * g - a * h,
           a * e - b * d]
    det = (a * cof[0] + b * cof[3]) + c * cof[6]
    out = np.zeros_like(M)
    for r in range(3):
        for q in range(3):
            out[..., r, q] = cof[3 * r + q] / det
        out[..., r, 3] = -((out[..., r, 0] * M[..., 0, 3] + out[..., r, 1] * M[..., 1, 3]) + out[..., r, 2] * M[..., 2, 3])
    out[..., 3, 3] = 1.0
    return out


def _mat4_mul(A, B):
    out = np.empty(np.broadcast_shapes(A.shape, B.shape))
    for r in range(4):
        for c in range(4):
            out[..., r, c] = ((A[..., r, 0] * B[..., 0, c] + A[..., r, 1] * B[..., 1, c]) + A[..., r, 2] * B[..., 2, c]) + A[..., r, 3] * B[..., 3, c]
    return out


def transform_odometry_host(odom, T):
    """-> (T * O * T^-1, its inverse), fp64"""
    T = np.asarray(T, np.float64)
    new = _mat4_mul(_mat4_mul(T, np.asarray(odom, np.float64)), affine_inverse(T))
    return new, affine_inverse(new)


def transform_boxes_host(pos, rot, valid, T):
    """numpy pos [..,2|3], rot [..,1], valid [..] -> (pos', rot') in the dtypes they came in; invalid boxes untouched"""
    T = np.asarray(T, np.float64)
    p = np.zeros(pos.shape[:-1] + (3,))
    p[..., :pos.shape[-1]] = pos
    yaw = rot[..., 0].astype(np.float64)
    cs, sn = np.cos(yaw), np.sin(yaw)
    with np.errstate(invalid="ignore"):
        new = np.stack([((T[r, 0] * p[..., 0] + T[r, 1] * p[..., 1]) + T[r, 2] * p[..., 2]) + T[r, 3] for r in range(3)], -1)
        yaw_new = np.arctan2(T[1, 0] * cs + T[1, 1] * sn, T[0, 0] * cs + T[0, 1] * sn)
    keep = np.ones(pos.shape[:-1], bool) if valid is None else np.asarray(valid, bool)
    pos_out = np.where(keep[..., None], new[..., :pos.shape[-1]].astype(pos.dtype), pos)
    rot_out = np.where(keep[..., None], yaw_new[..., None].astype(rot.dtype), rot)
    return pos_out, rot_out


def pillar_coordinates_host(pcl, bev_range_m, img_grid_size, height_range_m=(-np.inf, np.inf)):
    """numpy [N,C] -> (coors int32 [N,2], inside bool [N]): `voxelize_sample` (reference :975-987) with NaN rows outside"""
    rng = np.asarray(bev_range_m, np.float32).astype(np.float64)
    grid = np.asarray(img_grid_size).astype(np.int64)
    hr = np.asarray(height_range_m, np.float32).astype(np.float64)
    p = np.asarray(pcl)[:, :3].astype(np.float64)
    bad = np.isnan(p).any(-1)
    with np.errstate(invalid="ignore"):
        c = np.stack([((p[:, 0] + 0.5 * rng[0]) / rng[0]) * grid[0], ((p[:, 1] + 0.5 * rng[1]) / rng[1]) * grid[1],
                      ((p[:, 2] + 0.5 * 1000.0) / 1000.0) * 1.0], -1)
        ok = np.isfinite(c) & (c > -2147483649.0) & (c < 2147483648.0)
        ci = np.where(ok, np.where(ok, c, 0.0).astype(np.int64), np.iinfo(np.int32).min).astype(np.int32)
        inside = ((0 <= ci).all(-1) & (ci[:, 0] < grid[0]) & (ci[:, 1] < grid[1]) & (ci[:, 2] < 1) & (hr[0] < p[:, 2]) & (p[:, 2] < hr[1]))
    return ci[:, :2], inside & ~bad


def bev_crop_host(pcl, *, bev_range_m, img_grid_size, height_range_m=(-np.inf, np.inf), flow=None, lidar_rows=None, attr=None, drop=None):
    """one numpy cloud [N,C] -> dict(pcl, pillar_coors, count, keep[, flow, lidar_rows, attr]): the kept rows only, in order"""
    coors, inside = pillar_coordinates_host(pcl, bev_range_m, img_grid_size, height_range_m)
    keep = inside if drop is None else inside & ~np.asarray(drop, bool)
    out = {"pcl": np.asarray(pcl)[keep], "pillar_coors": coors[keep], "count": int(keep.sum()), "keep": keep}
    for k, v in (("flow", flow), ("lidar_rows", lidar_rows), ("attr", attr)):
        if v is not None:
            out[k] = np.asarray(v)[keep]
    return out


def bev_point_maps_host(pillar_coors, img_grid_size, flow=None):
    """one numpy cloud's pillar_coors [n,2] -> (occupancy float32 [1,H,W], flow_bev float32 [H,W,3] or None)"""
    H, W = int(img_grid_size[0]), int(img_grid_size[1])
    cnt = np.zeros((H, W), np.int64)
    np.add.at(cnt, (pillar_coors[:, 0], pillar_coors[:, 1]), 1)
    occ = (cnt > 0).astype(np.float32)[None]
    if flow is None:
        return occ, None
    acc = np.zeros((H, W, 3))
    np.add.at(acc, (pillar_coors[:, 0], pillar_coors[:, 1]), np.asarray(flow, np.float64))
    return occ, (acc / np.maximum(cnt, 1)[..., None]).astype(np.float32)


def moving_mask_host(pcl, flow, odom_tb_ta, threshold_dt):
    """numpy: ||(odom_tb_ta - I) * (x, y, z, 1) - flow|| > threshold_dt in fp64 -> bool [n]"""
    M = np.asarray(odom_tb_ta, np.float64) - np.eye(4)
    d = _lin3(M, np.asarray(pcl)[:, :3].astype(np.float64), True) - np.asarray(flow, np.float64)
    return np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) > threshold_dt


# ---- device wrappers -------------------------------------------------------------------------------------------------------------
class BoxJob(ctypes.Structure):
    """mirror of liso_sample_box_job (include/liso_sample_prep.h)"""
    _fields_ = [("pos", ctypes.c_void_p), ("rot", ctypes.c_void_p), ("valid", ctypes.c_void_p), ("k", ctypes.c_int), ("pos_dim", ctypes.c_int),
                ("is_f64", ctypes.c_int)]


class OdomJob(ctypes.Structure):
    """mirror of liso_sample_odom_job"""
    _fields_ = [("in_", ctypes.c_void_p), ("out", ctypes.c_void_p), ("out_inv", ctypes.c_void_p)]


class CropCfg(ctypes.Structure):
    """mirror of liso_bev_crop_cfg"""
    _fields_ = [("batch", ctypes.c_int), ("n_max", ctypes.c_int), ("point_stride", ctypes.c_int), ("grid_x", ctypes.c_int),
                ("grid_y", ctypes.c_int), ("range_x", ctypes.c_double), ("range_y", ctypes.c_double), ("z_min", ctypes.c_double),
                ("z_max", ctypes.c_double)]


MAX_JOBS = 16  # LISO_SAMPLE_MAX_JOBS


def _rider(t, p3, dtype, tail, name):
    """an optional per-point array riding with the cloud p3: [.., N] + tail in `dtype` on the cloud's device -> [B, N] + tail"""
    if t is None:
        return None
    if not torch.is_tensor(t) or not t.is_cuda or t.device != p3.device:
        raise L.LisoHipError(f"{name} must be a tensor on the cloud's device (CPU tensor given?)")
    if t.dtype == torch.bool and dtype == torch.uint8:
        t = as_u8(t)
    want = tuple(p3.shape[:2]) + tail
    if t.dtype != dtype or t.numel() != int(np.prod(want)):
        raise L.LisoHipError(f"{name} must be {dtype} with shape {want}, got {t.dtype} {tuple(t.shape)}")
    return t.reshape(want).contiguous()


def _transform_arg(T, batch, device):
    """T as [4,4] or [B,4,4] (numpy or tensor) -> fp64 device tensor [B,16]; a device tensor of that layout is used as it is, so a
    captured graph can be fed a new transform by copying into it"""
    if not torch.is_tensor(T):
        T = torch.from_numpy(np.ascontiguousarray(np.asarray(T, np.float64)))
    if T.shape[-2:] != (4, 4) and T.shape[-1] != 16:
        raise L.LisoHipError(f"T must be [4,4] or [B,4,4], got {tuple(T.shape)}")
    T = T.to(device=device, dtype=torch.float64, non_blocking=True).reshape(-1, 16)
    if T.shape[0] == 1 and batch > 1:
        T = T.expand(batch, 16)
    if T.shape[0] != batch:
        raise L.LisoHipError(f"T holds {T.shape[0]} transforms for a batch of {batch}")
    return T.contiguous()


def transform_cloud_device(pcl, T, flow=None, counts=None, out=None, out_flow=None):
    """float32 device cloud [N,C] / [B,N,C] (and its flow [..,3]) under T -> new tensors, or written into `out` / `out_flow`
    (which may be the inputs: in place).  No host synchronisation."""
    p3 = cloud3(pcl)
    B, N, C = p3.shape
    f3 = _rider(flow, p3, torch.float32, (3,), "flow")
    counts = counts_arg(counts, p3)
    Tm = _transform_arg(T, B, p3.device)
    o3 = torch.empty_like(p3) if out is None else _rider(out, p3, torch.float32, (C,), "out")
    of3 = None if f3 is None else (torch.empty_like(f3) if out_flow is None else _rider(out_flow, p3, torch.float32, (3,), "out_flow"))
    with torch.cuda.device(p3.device):
        L.check(L.lib().liso_sample_transform_f32(B, N, C, L.ptr(Tm), _p(p3), _p(counts), _p(f3), _p(o3), _p(of3), L.stream_ptr()),
                "sample transform")
    o = o3 if pcl.dim() == 3 else o3[0]
    if flow is None:
        return o
    return o, (of3 if pcl.dim() == 3 else of3[0])


def transform_poses_device(T, boxes=(), odoms=(), batch=None):
    """one launch for the small tensors.  `boxes`: (pos, rot, valid) triples of contiguous device tensors [B,K,2|3], [B,K,1], bool
    [B,K] or None, changed in place; `odoms`: (in, out, out_inv) fp64 [B,4,4] device tensors (out may be in, out_inv may be None)."""
    boxes, odoms = list(boxes), list(odoms)
    if not boxes and not odoms:
        return
    if len(boxes) > MAX_JOBS or len(odoms) > MAX_JOBS:
        for s in range(0, max(len(boxes), len(odoms)), MAX_JOBS):
            transform_poses_device(T, boxes[s:s + MAX_JOBS], odoms[s:s + MAX_JOBS], batch)
        return
    first = boxes[0][0] if boxes else odoms[0][0]
    L.require_cuda(first)
    B = int(batch if batch is not None else first.shape[0])
    bj = (BoxJob * max(len(boxes), 1))()
    keep = []
    for j, (pos, rot, valid) in enumerate(boxes):
        L.require_cuda(pos, rot)
        if pos.dtype != rot.dtype or pos.dtype not in (torch.float32, torch.float64) or not pos.is_contiguous() or not rot.is_contiguous():
            raise L.LisoHipError("box pos / rot must be contiguous float32 or float64 tensors of one dtype")
        if pos.dim() != 3 or pos.shape[0] != B or pos.shape[-1] not in (2, 3) or rot.numel() != B * pos.shape[1]:
            raise L.LisoHipError(f"box pos must be [B,K,2|3] and rot [B,K,1], got {tuple(pos.shape)} {tuple(rot.shape)}")
        v = None
        if valid is not None:
            v = as_u8(valid) if valid.dtype == torch.bool else valid.contiguous()
            if v.dtype != torch.uint8 or v.numel() != B * pos.shape[1] or not v.is_cuda:
                raise L.LisoHipError("box valid must be a bool [B,K] device tensor")
            keep.append(v)
        bj[j] = BoxJob(pos.data_ptr(), rot.data_ptr(), v.data_ptr() if v is not None else None, pos.shape[1], pos.shape[-1],
                       int(pos.dtype == torch.float64))
    oj = (OdomJob * max(len(odoms), 1))()
    for j, (src, dst, inv) in enumerate(odoms):
        for t in (src, dst) + ((inv,) if inv is not None else ()):
            L.require_cuda(t)
            if t.dtype != torch.float64 or t.numel() != B * 16 or not t.is_contiguous():
                raise L.LisoHipError("odometries must be contiguous float64 [B,4,4] device tensors")
        oj[j] = OdomJob(src.data_ptr(), dst.data_ptr(), inv.data_ptr() if inv is not None else None)
    Tm = _transform_arg(T, B, first.device)
    with torch.cuda.device(first.device):
        L.check(L.lib().liso_sample_transform_poses_f64(B, L.ptr(Tm), bj, len(boxes), oj, len(odoms), L.stream_ptr()), "sample transform poses")


# ---- the reference's names --------------------------------------------------------------------------------------------------------
def transform_pcl_maybe_with_intensity(pcl, T, counts=None):
    """reference :1464-1483; any number of channels behind x, y, z is carried along"""
    if is_np(pcl):
        assert np.asarray(T).shape == (4, 4), np.asarray(T).shape
        return transform_cloud_host(pcl, T)
    return transform_cloud_device(pcl, T, counts=counts)


def transform_flow(flow, T):
    """reference :1369-1384 -- the linear part of T on a flow field [N,3] / [B,N,3]"""
    if is_np(flow):
        with np.errstate(invalid="ignore"):
            return _lin3(np.asarray(T, np.float64), flow[:, :3].astype(np.float64), False).astype(np.float32)
    if not torch.is_tensor(flow) or flow.shape[-1] != 3:
        raise L.LisoHipError("flow must be a [N, 3] or [B, N, 3] tensor")
    L.require_cuda(flow)
    # the flow rows are their own "cloud": linear part only, so the kernel's flow slot takes them and the cloud slot a copy
    f3 = (flow if flow.dim() == 3 else flow[None]).contiguous()
    Tm = _transform_arg(T, f3.shape[0], f3.device).clone().view(-1, 4, 4)
    Tm[:, :3, 3] = 0.0
    out = transform_cloud_device(f3, Tm)
    return out if flow.dim() == 3 else out[0]


def transform_odometry(odom, T):
    """reference :1347-1365 -- (T * O * T^-1, its inverse)"""
    if is_np(odom):
        return transform_odometry_host(odom, T)
    L.require_cuda(odom)
    o3 = (odom if odom.dim() == 3 else odom[None]).to(torch.float64).contiguous()
    new, inv = torch.empty_like(o3), torch.empty_like(o3)
    transform_poses_device(T, odoms=[(o3, new, inv)])
    return (new, inv) if odom.dim() == 3 else (new[0], inv[0])


def transform_boxes(shape: Shape, T):
    """reference :1435-1462 -- a copy of `shape` with pos / rot under T, in the dtypes they came in; invalid boxes untouched"""
    out = shape.clone()
    if is_np(shape.pos):
        out.pos, out.rot = transform_boxes_host(shape.pos, shape.rot, shape.valid, T)
        return out
    L.require_cuda(shape.pos)
    unb = shape.pos.dim() == 2
    pos = (out.pos[None] if unb else out.pos).contiguous()
    rot = (out.rot[None] if unb else out.rot).to(pos.dtype).contiguous()
    valid = (out.valid[None] if unb else out.valid).contiguous()
    transform_poses_device(T, boxes=[(pos, rot, valid)])
    out.pos, out.rot = (pos[0], rot[0]) if unb else (pos, rot)
    return out


def augment_sample_content(sample_content, src_key, target_key, dataset_name, *, cfg, T=None):
    """reference :1291-1433 for a dictionary of device tensors (unbatched or collated); returns T.  Clouds and flows are
    [N,C] / [B,N,C] float32, odometries fp64 [4,4] / [B,4,4], objects `Shape`s.  `T`: [4,4] / [B,4,4]; drawn when None."""
    for k in (f"pcl_full_no_ground_{src_key}", f"pcl_full_w_ground_{src_key}", f"pcl_full_no_ground_{target_key}",
              f"pcl_full_w_ground_{target_key}"):
        assert k not in sample_content, "will not be augmented!"
    if T is None:
        aug = cfg.data.augmentation
        T = get_augmentation_transform(max_symm_rot_deg=aug.rotation.max_rot_deg,
                                       max_sensor_pos_offset_m=aug.translation.max_sensor_pos_offset_m, max_xy_scale_delta=None)
    sc = sample_content
    if "pcl_tx" in sc:
        assert "flow_t0_tx" not in sc, "not augmented, add below!"
    for k in (f"pcl_{src_key}", f"pcl_{target_key}", "pcl_tx"):
        if k in sc:
            sc[k] = transform_pcl_maybe_with_intensity(sc[k], T)
    odoms = []
    for source in {"gt", cfg.data.odom_source}:
        sub = sc.get(source, {})
        for fwd, rev in (("odom_t0_tx", "odom_tx_t0"), (f"odom_{src_key}_{target_key}", f"odom_{target_key}_{src_key}")):
            if fwd in sub and not any(sub is s and fwd == f for s, f, _ in odoms):
                odoms.append((sub, fwd, rev))
    for source in {"gt", cfg.data.flow_source}:
        if source in sc:
            for k in (f"flow_{src_key}_{target_key}", f"flow_{target_key}_{src_key}"):
                if k in sc[source]:
                    sc[source][k] = transform_flow(sc[source][k], T)
    boxes = []
    if dataset_name in ("kitti", "nuscenes", "kitti_object", "waymo", "av2"):
        gt_keys = [f"{kind}_{t}" for t in ("t0", "t1", "t2") for kind in ("objects", "boxes")]
        if dataset_name == "kitti_object":
            gt_keys = [f"{kind}_{t}" for t in ("t0", "t1", "t2") for kind in ("objects", "kitti_ignore_region_boxes")]
        boxes += [(sc["gt"], k) for k in gt_keys if k in sc.get("gt", {}) and isinstance(sc["gt"][k], Shape)]
        for k in gt_keys:  # kitti_object keeps its objects as a dictionary of poses (reference :1392-1398)
            v = sc.get("gt", {}).get(k)
            if isinstance(v, dict) and "poses" in v:
                Tp = np.asarray(T, np.float64) if is_np(v["poses"]) else _transform_arg(T, 1, v["poses"].device).view(4, 4)
                v["poses"] = Tp @ v["poses"]
    else:
        raise NotImplementedError(dataset_name)
    if "mined" in sc:
        boxes += [(sc["mined"], f"{kind}_{t}") for t in ("t0", "t1", "t2") for kind in ("objects", "boxes") if f"{kind}_{t}" in sc["mined"]]
    if any(is_np(sub[k]) for sub, k, _ in odoms) or any(is_np(sub[k].pos) for sub, k in boxes):
        for sub, fwd, rev in odoms:
            sub[fwd], sub[rev] = transform_odometry(sub[fwd], T)
        for sub, k in boxes:
            sub[k] = transform_boxes(sub[k], T)
        return T
    # the small tensors: one launch
    box_jobs, odom_jobs, batch = [], [], None
    for sub, fwd, rev in odoms:
        o = sub[fwd]
        o3 = (o if o.dim() == 3 else o[None]).to(torch.float64).contiguous()
        new, inv = torch.empty_like(o3), torch.empty_like(o3)
        odom_jobs.append((o3, new, inv))
        sub[fwd], sub[rev] = (new, inv) if o.dim() == 3 else (new[0], inv[0])
        batch = o3.shape[0]
    for sub, k in boxes:
        s = sub[k].clone()
        unb = s.pos.dim() == 2
        pos = (s.pos[None] if unb else s.pos).contiguous()
        rot = (s.rot[None] if unb else s.rot).to(pos.dtype).contiguous()
        box_jobs.append((pos, rot, (s.valid[None] if unb else s.valid).contiguous()))
        s.pos, s.rot = (pos[0], rot[0]) if unb else (pos, rot)
        sub[k] = s
        batch = pos.shape[0]
    transform_poses_device(T, box_jobs, odom_jobs, batch)
    return T


# ---- crop and maps over the collated layout ---------------------------------------------------------------------------------------
def _grid(img_grid_size):
    g = np.asarray(img_grid_size).astype(np.int64).reshape(-1)
    return int(g[0]), int(g[1])


def pillarize_bev(pcl, counts=None, *, bev_range_m, img_grid_size, height_range_m=(-np.inf, np.inf), flow=None, lidar_rows=None,
                  attr=None, drop=None):
    """reference :1147-1163 (and, through `drop`, the removal of :1165-1185 in the same compaction).  Device: pcl [N,C] / [B,N,C]
    float32, flow [..,3] float32, lidar_rows int32, attr uint8 / bool, drop bool -> dict(pcl, counts int32 [B], pillar_coors int32
    [..,2], and flow / lidar_rows / attr when given), kept rows first, paddings NaN / -1 / 0.  numpy: one cloud [N,C] -> the kept
    rows only (`bev_crop_host`)."""
    if is_np(pcl):
        return bev_crop_host(pcl, bev_range_m=bev_range_m, img_grid_size=img_grid_size, height_range_m=height_range_m, flow=flow,
                             lidar_rows=lidar_rows, attr=attr, drop=drop)
    p3 = cloud3(pcl)
    B, N, C = p3.shape
    counts = counts_arg(counts, p3)
    f3 = _rider(flow, p3, torch.float32, (3,), "flow")
    rows = _rider(lidar_rows, p3, torch.int32, (), "lidar_rows")
    was_bool = attr is not None and attr.dtype == torch.bool
    at = _rider(attr, p3, torch.uint8, (), "attr")
    dr = _rider(drop, p3, torch.uint8, (), "drop")
    rng = np.asarray(bev_range_m, np.float32).astype(np.float64)
    hr = np.asarray(height_range_m, np.float32).astype(np.float64)
    gx, gy = _grid(img_grid_size)
    cfg = CropCfg(B, N, C, gx, gy, float(rng[0]), float(rng[1]), float(hr[0]), float(hr[1]))
    dev = p3.device
    out = {"pcl": torch.empty_like(p3), "counts": torch.empty((B,), dtype=torch.int32, device=dev),
           "pillar_coors": torch.empty((B, N, 2), dtype=torch.int32, device=dev)}
    if f3 is not None:
        out["flow"] = torch.empty_like(f3)
    if rows is not None:
        out["lidar_rows"] = torch.empty_like(rows)
    if at is not None:
        out["attr"] = torch.empty_like(at)
    lib = L.lib()
    ws_bytes = lib.liso_bev_crop_workspace_bytes(B, N)
    ws = torch.empty(max(ws_bytes, 256), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        L.check(lib.liso_bev_crop_f32(ctypes.byref(cfg), _p(p3), _p(counts), _p(dr), _p(f3), _p(rows), _p(at), _p(out["pcl"]),
                                      _p(out.get("flow")), _p(out.get("lidar_rows")), _p(out.get("attr")), _p(out["pillar_coors"]),
                                      L.ptr(out["counts"]), L.ptr(ws) if N else None, ws_bytes, L.stream_ptr()), "bev crop")
    if was_bool:
        out["attr"] = out["attr"].view(torch.bool)
    if pcl.dim() == 2:
        out = {k: (v if k == "counts" else v[0]) for k, v in out.items()}
    return out


def bev_point_maps(pillar_coors, counts, img_grid_size, *, pcl=None, flow=None, flow2=None, odom_tb_ta=None, threshold_dt=None,
                   want_occupancy=True):
    """the maps and the moving mask of compacted device rows, one call (include/liso_sample_prep.h, entry 4) ->
    dict(occupancy_f32 [B,1,H,W], flow_bev [B,H,W,3], flow_bev2, moving_mask bool [B,N]) with the entries that were asked for"""
    if not torch.is_tensor(pillar_coors):
        raise L.LisoHipError("pillar_coors must be a device tensor")
    L.require_cuda(pillar_coors)
    if pillar_coors.dtype != torch.int32 or pillar_coors.shape[-1] != 2 or pillar_coors.dim() not in (2, 3):
        raise L.LisoHipError("pillar_coors must be int32 [N,2] or [B,N,2]")
    unb = pillar_coors.dim() == 2
    co = (pillar_coors[None] if unb else pillar_coors).contiguous()
    B, N = co.shape[:2]
    dev = co.device
    counts = counts_arg(counts, co)
    H, W = _grid(img_grid_size)
    f0 = _rider(flow, co, torch.float32, (3,), "flow")
    f1 = _rider(flow2, co, torch.float32, (3,), "flow2")
    if f1 is not None and f0 is None:
        raise L.LisoHipError("flow2 without flow")
    want_mask = odom_tb_ta is not None
    p3, od, C = None, None, 3
    if want_mask:
        if pcl is None or f0 is None or threshold_dt is None:
            raise L.LisoHipError("the moving mask needs pcl, flow, odom_tb_ta and threshold_dt")
        p3 = cloud3(pcl)
        C = p3.shape[2]
        if tuple(p3.shape[:2]) != (B, N):
            raise L.LisoHipError("pcl and pillar_coors disagree in shape")
        L.require_cuda(odom_tb_ta)
        od = odom_tb_ta.to(torch.float64).reshape(-1, 16).contiguous()
        if od.shape[0] != B:
            raise L.LisoHipError("odom_tb_ta must be [B,4,4]")
    res = {}
    if want_occupancy:
        res["occupancy_f32"] = torch.empty((B, 1, H, W), dtype=torch.float32, device=dev)
    if f0 is not None:
        res["flow_bev"] = torch.empty((B, H, W, 3), dtype=torch.float32, device=dev)
    if f1 is not None:
        res["flow_bev2"] = torch.empty((B, H, W, 3), dtype=torch.float32, device=dev)
    mask = torch.empty((B, N), dtype=torch.uint8, device=dev) if want_mask else None
    lib = L.lib()
    ws_bytes = lib.liso_bev_point_maps_workspace_bytes(B, H, W, (f0 is not None) + (f1 is not None))
    if ws_bytes == 0:
        raise L.LisoHipError(f"bev point maps: grid {H} x {W} refused")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        L.check(lib.liso_bev_point_maps_f32(B, N, C, H, W, _p(p3), _p(counts), _p(co), _p(f0), _p(f1), _p(od),
                                            float(threshold_dt) if want_mask else 0.0, _p(res.get("occupancy_f32")), _p(res.get("flow_bev")),
                                            _p(res.get("flow_bev2")), _p(mask), L.ptr(ws), ws_bytes, L.stream_ptr()), "bev point maps")
    if want_mask:
        res["moving_mask"] = mask.view(torch.bool)
    if unb:
        res = {k: v[0] for k, v in res.items()}
    return res


def add_bev_flow(pillar_coors, flow, img_grid_size, counts=None):
    """reference :1200-1213 -- float32 [H,W,3] / [B,H,W,3]: the per-cell mean of `flow`, 0 in empty cells"""
    if is_np(pillar_coors):
        return bev_point_maps_host(pillar_coors, img_grid_size, flow)[1]
    return bev_point_maps(pillar_coors, counts, img_grid_size, flow=flow, want_occupancy=False)["flow_bev"]


def add_bev_ground_height_occupancy_maps(pillar_coors, img_grid_size, counts=None):
    """reference :1215-1223 -- float32 [1,H,W] / [B,1,H,W]: 1 where a pillar has a point"""
    if is_np(pillar_coors):
        return bev_point_maps_host(pillar_coors, img_grid_size)[0]
    return bev_point_maps(pillar_coors, counts, img_grid_size)["occupancy_f32"]


def moving_mask(pcl, flow, odom_tb_ta, threshold_dt, counts=None, pillar_coors=None):
    """reference :776-792 -- bool [N] / [B,N]; False behind the count"""
    if is_np(pcl):
        return moving_mask_host(pcl, flow, odom_tb_ta, threshold_dt)
    L.require_cuda(pcl)
    if pillar_coors is None:
        pillar_coors = torch.zeros(tuple(pcl.shape[:-1]) + (2,), dtype=torch.int32, device=pcl.device)
    od = odom_tb_ta if odom_tb_ta.dim() == 3 or pcl.dim() == 2 else odom_tb_ta[None]
    return bev_point_maps(pillar_coors, counts, (1, 1), pcl=pcl, flow=flow, odom_tb_ta=od, threshold_dt=threshold_dt,
                          want_occupancy=False)["moving_mask"]


def height_range_of(cfg):
    """reference :498-503"""
    if getattr(cfg.data, "limit_pillar_height", False):
        return np.array(cfg.data.pillar_height_range_m, np.float32)
    return np.array([-np.inf, np.inf], np.float32)


def assemble_bev_sample(pcl, counts=None, *, flow=None, lidar_rows=None, drop=None, odom_tb_ta=None, dt=None, cfg):
    """crop + compaction + maps + moving mask of a collated device batch in one call, capturable in a hipGraph ->
    dict(pcl_ta = {pcl, pcl_is_valid, pillar_coors} as `collate_list_data` lays it out, counts, occupancy_f32, and, with `flow`,
    flow_ta_tb / flow_bev_ta_tb, with `lidar_rows` lidar_rows_ta, with `odom_tb_ta` and `dt` moving_mask)."""
    grid = cfg.data.img_grid_size
    crop = pillarize_bev(pcl, counts, bev_range_m=cfg.data.bev_range_m, img_grid_size=grid, height_range_m=height_range_of(cfg), flow=flow,
                         lidar_rows=lidar_rows, drop=drop)
    want_mask = odom_tb_ta is not None and dt is not None and flow is not None
    maps = bev_point_maps(crop["pillar_coors"], crop["counts"], grid, pcl=crop["pcl"] if want_mask else None, flow=crop.get("flow"),
                          odom_tb_ta=odom_tb_ta if want_mask else None,
                          threshold_dt=float(cfg.data.non_rigid_flow_threshold_mps) * float(dt) if want_mask else None)
    N = crop["pcl"].shape[-2]
    valid = torch.arange(N, device=crop["pcl"].device, dtype=torch.int32) < (crop["counts"][:, None] if pcl.dim() == 3 else crop["counts"])
    out = {"pcl_ta": {"pcl": crop["pcl"], "pcl_is_valid": valid, "pillar_coors": crop["pillar_coors"]}, "counts": crop["counts"],
           "occupancy_f32": maps["occupancy_f32"]}
    if "flow" in crop:
        out["flow_ta_tb"], out["flow_bev_ta_tb"] = crop["flow"], maps["flow_bev"]
    if "lidar_rows" in crop:
        out["lidar_rows_ta"] = crop["lidar_rows"]
    if want_mask:
        out["moving_mask"] = maps["moving_mask"]
    return out
