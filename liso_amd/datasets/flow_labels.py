"""The per-point ground truth the dataset builders derive from annotated, tracked boxes: the scene flow `flow_ta_tb`, the track id /
annotation index and the box slot of every point, and the point count of every box.  One call for many directed sweep pairs.

Replaces the builders' per-box numpy loops (reference liso/datasets/kitti/create_kitti_tracking.py:14-17, :340-387;
liso/datasets/nuscenes/create.py:229-238, :301-366, :392-429; liso/datasets/argoverse2/create.py:216-228, :357-383), which state
one computation three times with three overlap rules: later box wins (KITTI, nuScenes; `LAST`), first box wins (AV2; `FIRST`), the
id for every containing box but the flow only for boxes present at tb (KITTI), membership gated by the point's semantic class with
an ungated count (nuScenes), an in/out flow updated once per category (AV2; `keep_flow`).

Device tensors go through include/liso_flow_labels.h (liso_amd/csrc/flow_labels.hip): two launches per call whatever the number
of jobs and boxes, no host synchronisation.  numpy arrays run the host path of this file, which performs the same operations in
the same order and agrees with the device bit for bit, labels and flow.  The header states the expressions in full; in short, with
points widened from fp32 to fp64 and `rinv(M) = [R^T | -R^T t]` in closed form:
  A = rinv(pose_a), D = pose_b A - I, S = rinv(odom) - I;  inside: |A p| < size / 2 on all three axes (strict);
  flow = D p of the winning box that exists at tb, else S p (or what `flow` held, with `keep_flow`), rounded to fp32 once.
Points are read as fp32: a float64 cloud is rounded first, on both paths.
"""
import ctypes
from typing import NamedTuple

import numpy as np
import torch

from liso_amd import _lib as L
from liso_amd.kabsch.shape_utils import Shape
from liso_amd.utils.device_args import as_u8, cloud3, counts_arg, is_np, opt_ptr as _p

LAST, FIRST = 0, 1  # LISO_OVERLAP_*
MAX_BOXES = 4096    # LISO_FLOW_LABELS_MAX_BOXES
CHUNK = 128         # LISO_FLOW_LABELS_CHUNK
DUMMY_TRACK_ID = 65535  # np.iinfo(np.uint16).max, reference create_kitti_tracking.py:350
ALL_DIRECTIONS = ((0, 1), (1, 0), (0, 2), (2, 0), (1, 2), (2, 1))


class FlowLabelsCfg(ctypes.Structure):
    """mirror of liso_flow_labels_cfg"""
    _fields_ = [("n_jobs", ctypes.c_int), ("n_clouds", ctypes.c_int), ("n_boxes", ctypes.c_int), ("n_max", ctypes.c_int),
                ("point_stride", ctypes.c_int), ("overlap", ctypes.c_int), ("keep_flow", ctypes.c_int), ("no_label", ctypes.c_int)]


class FlowLabels(NamedTuple):
    flow: object         # float32 [J, n_max, 3]
    point_label: object  # int32 [J, n_max] or None
    point_box: object    # int32 [J, n_max] or None
    count: object        # int32 [J, K] or None


# ---- host path -------------------------------------------------------------------------------------------------------------------
def rigid_inverse_host(M):
    """fp64 [.., 4, 4] rigid poses -> [R^T | -R^T t] in the header's operation order"""
    M = np.asarray(M, np.float64)
    out = np.zeros_like(M)
    for r in range(3):
        for c in range(3):
            out[..., r, c] = M[..., c, r]
        out[..., r, 3] = -((M[..., 0, r] * M[..., 0, 3] + M[..., 1, r] * M[..., 1, 3]) + M[..., 2, r] * M[..., 2, 3])
    out[..., 3, 3] = 1.0
    return out


def box_motion_host(pose_a, pose_b):
    """-> (A, D): A = rinv(pose_a), D = pose_b A - I, rows 0..2 as the header writes them"""
    A, Pb = rigid_inverse_host(pose_a), np.asarray(pose_b, np.float64)
    D = np.zeros_like(A)
    for r in range(3):
        for c in range(3):
            D[..., r, c] = ((Pb[..., r, 0] * A[..., 0, c] + Pb[..., r, 1] * A[..., 1, c]) + Pb[..., r, 2] * A[..., 2, c]) - (1.0 if r == c else 0.0)
        D[..., r, 3] = ((Pb[..., r, 0] * A[..., 0, 3] + Pb[..., r, 1] * A[..., 1, 3]) + Pb[..., r, 2] * A[..., 2, 3]) + Pb[..., r, 3]
    return A, D


def odometry_flow_matrix_host(odom):
    S = rigid_inverse_host(odom)
    for r in range(3):
        S[..., r, r] = S[..., r, r] - 1.0
    return S


def _apply(M, x, y, z):
    """rows 0..2 of the 4x4 `M` applied to (x, y, z, 1): fp64 [n, 3]"""
    return np.stack([((M[r, 0] * x + M[r, 1] * y) + M[r, 2] * z) + M[r, 3] for r in range(3)], -1)


def _inside(A, size, x, y, z):
    p = _apply(A, x, y, z)
    half = np.asarray(size, np.float64) / 2.0
    return (np.abs(p[:, 0]) < half[0]) & (np.abs(p[:, 1]) < half[1]) & (np.abs(p[:, 2]) < half[2])


def flow_labels_host(pcl, counts, cloud_of, odom, pose_a, pose_b, size, valid, has_b, label, box_class=None, point_class=None, *,
                     no_label=-1, overlap=LAST, keep_flow=False, flow=None):
    """The numpy restatement of liso_flow_labels_f32: the same operations in the same order.  pcl [C,n_max,>=3], counts [C] or None,
    cloud_of [J], odom [J,4,4], box tables [J,K,.] -> FlowLabels of numpy arrays.  With `keep_flow`, `flow` float32 [J,n_max,3] is
    updated in place and returned."""
    pcl = np.asarray(pcl)
    C, N = pcl.shape[:2]
    J, K = np.asarray(valid).shape
    if (box_class is None) != (point_class is None):
        raise ValueError("box_class and point_class come together")
    if overlap not in (LAST, FIRST):
        raise ValueError(f"overlap must be LAST or FIRST, got {overlap}")
    if keep_flow:
        if flow is None or flow.dtype != np.float32 or flow.shape != (J, N, 3):
            raise ValueError("keep_flow needs flow float32 [J, n_max, 3]")
    else:
        flow = np.empty((J, N, 3), np.float32)
    point_label = np.full((J, N), no_label, np.int32)
    point_box = np.full((J, N), -1, np.int32)
    count = np.zeros((J, K), np.int32)
    A_all, D_all = box_motion_host(np.asarray(pose_a, np.float64).reshape(J, K, 4, 4), np.asarray(pose_b, np.float64).reshape(J, K, 4, 4))
    S_all = odometry_flow_matrix_host(np.asarray(odom, np.float64).reshape(J, 4, 4))
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(J):
            c = int(cloud_of[j])
            rows = 0 if not 0 <= c < C else (N if counts is None else min(max(int(counts[c]), 0), N))
            xyz = pcl[c, :rows, :3].astype(np.float32) if rows else np.zeros((0, 3), np.float32)
            live = np.flatnonzero(np.isfinite(xyz).all(-1))
            x, y, z = (xyz[live, a].astype(np.float64) for a in range(3))
            box = np.full(live.size, -1, np.int64)
            flow_box = np.full(live.size, -1, np.int64)
            for k in range(K):
                if not valid[j, k]:
                    continue
                inside = _inside(A_all[j, k], size[j, k], x, y, z)
                count[j, k] = np.count_nonzero(inside)
                member = inside
                if box_class is not None and box_class[j, k] >= 0:
                    member = inside & (np.asarray(point_class)[c, live] == box_class[j, k])
                take = member if overlap == LAST else member & (box < 0)
                box[take] = k
                if has_b[j, k]:
                    take = member if overlap == LAST else member & (flow_box < 0)
                    flow_box[take] = k
            dead = np.ones(N, bool)
            dead[live] = False
            flow[j, dead] = np.nan
            won = box >= 0
            point_box[j, live[won]] = box[won]
            point_label[j, live[won]] = np.asarray(label)[j, box[won]]
            rigid = flow_box < 0
            if not keep_flow:
                flow[j, live[rigid]] = _apply(S_all[j], x[rigid], y[rigid], z[rigid]).astype(np.float32)
            for k in np.unique(flow_box[~rigid]):
                m = flow_box == k
                flow[j, live[m]] = _apply(D_all[j, k], x[m], y[m], z[m]).astype(np.float32)
    return FlowLabels(flow, point_label, point_box, count)


# ---- device path -----------------------------------------------------------------------------------------------------------------
def workspace_bytes(n_jobs, n_boxes):
    return int(L.lib().liso_flow_labels_workspace_bytes(int(n_jobs), int(n_boxes)))


def _table(t, shape, dtype, name):
    if not torch.is_tensor(t) or tuple(t.shape) != shape:
        raise L.LisoHipError(f"{name} must be a device tensor of shape {shape}, got {tuple(t.shape) if torch.is_tensor(t) else type(t)}")
    L.require_cuda(t)
    if dtype == torch.uint8:
        return as_u8(t, convert=True)
    return t.to(dtype).contiguous()


def flow_labels(pcl, counts, cloud_of, odom, pose_a, pose_b, size, valid, has_b, label, box_class=None, point_class=None, *, no_label=-1,
                overlap=LAST, keep_flow=False, flow=None, want_label=True, want_box=True, want_count=True, workspace=None):
    """liso_flow_labels_f32 on device tensors: pcl float32 [C,n_max,>=3], counts int32 [C] or None, cloud_of int32 [J], odom [J,4,4],
    pose_a / pose_b [J,K,4,4], size [J,K,3], valid / has_b bool [J,K], label int32 [J,K], optionally box_class int32 [J,K] with
    point_class int32 [C,n_max].  -> FlowLabels of device tensors (the outputs not wanted are None).  With `keep_flow`, `flow`
    float32 [J,n_max,3] is the in/out array.  No host read: the call can be captured in a hipGraph."""
    p3 = cloud3(pcl)
    C, N, stride = p3.shape
    counts = counts_arg(counts, p3)
    dev = p3.device
    if not torch.is_tensor(valid) or valid.dim() != 2:
        raise L.LisoHipError("valid must be a [J, K] device tensor")
    J, K = valid.shape
    if K > MAX_BOXES:
        raise L.LisoHipError(f"{K} boxes per job: at most {MAX_BOXES} (LISO_FLOW_LABELS_MAX_BOXES)")
    if (box_class is None) != (point_class is None):
        raise L.LisoHipError("box_class and point_class come together")
    cloud_of = _table(cloud_of, (J,), torch.int32, "cloud_of")
    odom = _table(odom, (J, 4, 4), torch.float64, "odom")
    pose_a, pose_b = _table(pose_a, (J, K, 4, 4), torch.float64, "pose_a"), _table(pose_b, (J, K, 4, 4), torch.float64, "pose_b")
    size = _table(size, (J, K, 3), torch.float64, "size")
    valid, has_b = _table(valid, (J, K), torch.uint8, "valid"), _table(has_b, (J, K), torch.uint8, "has_b")
    label = _table(label, (J, K), torch.int32, "label")
    if box_class is not None:
        box_class, point_class = _table(box_class, (J, K), torch.int32, "box_class"), _table(point_class, (C, N), torch.int32, "point_class")
        if K == 0 or N == 0:  # nothing to gate, and an empty table has no address to hand over
            box_class = point_class = None
    if keep_flow:
        if not torch.is_tensor(flow) or flow.dtype != torch.float32 or tuple(flow.shape) != (J, N, 3) or not flow.is_contiguous() or flow.device != dev:
            raise L.LisoHipError("keep_flow needs flow: a contiguous float32 [J, n_max, 3] tensor on the cloud's device")
    else:
        flow = torch.empty((J, N, 3), dtype=torch.float32, device=dev)
    point_label = torch.empty((J, N), dtype=torch.int32, device=dev) if want_label else None
    point_box = torch.empty((J, N), dtype=torch.int32, device=dev) if want_box else None
    count = torch.empty((J, K), dtype=torch.int32, device=dev) if want_count else None
    need = workspace_bytes(J, K)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    elif workspace.numel() * workspace.element_size() < need or workspace.device != dev:
        raise L.LisoHipError(f"workspace: {need} bytes on the cloud's device are needed")
    cfg = FlowLabelsCfg(J, C, K, N, stride, int(overlap), int(bool(keep_flow)), int(no_label))
    with torch.cuda.device(dev):
        L.check(L.lib().liso_flow_labels_f32(ctypes.byref(cfg), _p(p3), _p(counts), _p(cloud_of), _p(odom), _p(pose_a), _p(pose_b), _p(size),
                                             _p(valid), _p(has_b), _p(label), _p(box_class), _p(point_class), _p(flow), _p(point_label),
                                             _p(point_box), _p(count), L.ptr(workspace), workspace.numel() * workspace.element_size(),
                                             L.stream_ptr()), "flow labels")
    return FlowLabels(flow, point_label, point_box, count)


# ---- the builders' functions, by their names and keyword signatures ---------------------------------------------------------------
def _one_cloud(pcl_homog):
    """[N, >=3] points of either kind -> the float32 [1, N, C] cloud both paths read"""
    if is_np(pcl_homog):
        return np.ascontiguousarray(pcl_homog, np.float32)[None]
    L.require_cuda(pcl_homog)
    return pcl_homog.to(torch.float32).contiguous()[None]


def _xp(x):
    return np if is_np(x) else torch


def _one_job(pcl_homog, odom, pose_a, pose_b, size, valid, has_b, label, **kw):
    """one job over one cloud, numpy or device"""
    cloud = _one_cloud(pcl_homog)
    if is_np(cloud):
        fn, cloud_of = flow_labels_host, np.zeros(1, np.int32)
        valid, has_b, label = (np.asarray(v)[None] for v in (valid, has_b, label))
    else:
        fn, cloud_of = flow_labels, torch.zeros(1, dtype=torch.int32, device=cloud.device)
        valid, has_b, label = valid[None], has_b[None], label[None]
    return fn(cloud, None, cloud_of, odom[None], pose_a[None], pose_b[None], size[None], valid, has_b, label, **kw)


def get_points_in_box_mask(pcl_homog, lidar_T_obj, obj_size):
    """reference create_kitti_tracking.py:14-17 -- bool [N]: the point lies strictly inside the box"""
    xp = _xp(pcl_homog)
    if xp is np:
        one, eye = np.ones(1, bool), np.eye(4)
        label = np.zeros(1, np.int32)
        pose, size = np.asarray(lidar_T_obj, np.float64)[None], np.asarray(obj_size, np.float64).reshape(1, 3)
    else:
        dev = pcl_homog.device
        one, eye = torch.ones(1, dtype=torch.bool, device=dev), torch.eye(4, dtype=torch.float64, device=dev)
        label = torch.zeros(1, dtype=torch.int32, device=dev)
        pose, size = lidar_T_obj.to(torch.float64)[None], obj_size.to(torch.float64).reshape(1, 3)
    res = _one_job(pcl_homog, eye, pose, pose, size, one, one, label)
    return res.point_box[0] >= 0


def extract_lidar_flow_ta_tb(*, pcl_homog_ta, lidar_Tta_obj, obj_dims_ta, track_ids_ta, track_ids_tb, lidar_Ttb_obj, odom_ta_tb):
    """reference create_kitti_tracking.py:340-387 -> (flow float32 [N,3], track_ids_mask uint16 [N], 65535 where no box holds the
    point).  The partner of a box is the first box at tb with its track id (`track_id in track_ids_tb`, `np.argwhere(..)[0, 0]`),
    looked up without a host read on the device path."""
    xp = _xp(pcl_homog_ta)
    K, Kb = len(track_ids_ta), len(track_ids_tb)
    same = track_ids_ta[:, None] == track_ids_tb[None, :]  # [K, Kb]
    if xp is np:
        has_b = same.any(1) if Kb else np.zeros(K, bool)
        pose_a = np.asarray(lidar_Tta_obj, np.float64).reshape(K, 4, 4)
        pose_b = np.asarray(lidar_Ttb_obj, np.float64).reshape(Kb, 4, 4)[same.argmax(1)] if Kb else pose_a
        valid, label = np.ones(K, bool), np.asarray(track_ids_ta).astype(np.int32)
        size = np.asarray(obj_dims_ta, np.float64).reshape(K, 3)
    else:
        dev = pcl_homog_ta.device
        has_b = same.any(1) if Kb else torch.zeros(K, dtype=torch.bool, device=dev)
        pose_a = lidar_Tta_obj.to(torch.float64).reshape(K, 4, 4)
        pose_b = lidar_Ttb_obj.to(torch.float64).reshape(Kb, 4, 4)[same.to(torch.uint8).argmax(1)] if Kb else pose_a
        valid, label = torch.ones(K, dtype=torch.bool, device=dev), track_ids_ta.to(torch.int32)
        size = obj_dims_ta.to(torch.float64).reshape(K, 3)
    res = _one_job(pcl_homog_ta, odom_ta_tb, pose_a, pose_b, size, valid, has_b, label, no_label=DUMMY_TRACK_ID)
    ids = res.point_label[0]
    # (the low 16 bits of the int32, as uint16)
    ids = ids.astype(np.uint16) if xp is np else ids.to(torch.int16).view(torch.uint16)
    return res.flow[0], ids


def update_dynamic_flow(homog_pcl_ta, flow_ta_tb, matched_boxes_of_cat_ta, matched_boxes_of_cat_tb):
    """reference argoverse2/create.py:357-383 -- the flow of the points inside the matched boxes of one category, written into
    `flow_ta_tb` [N,3] in place (first containing box wins; every other point keeps its value) and returned.  Boxes are `Shape`s
    [K] whose slot k at ta and at tb is one object.  The device path wants `flow_ta_tb` float32 and contiguous."""
    a, b = matched_boxes_of_cat_ta, matched_boxes_of_cat_tb
    if not isinstance(a, Shape) or not isinstance(b, Shape) or a.valid.shape != b.valid.shape:
        raise ValueError("boxes at ta and tb must be Shapes of the same [K]")
    if is_np(homog_pcl_ta):
        pose_a, pose_b = a.get_poses(), b.get_poses()
        K = a.valid.shape[0]
        eye, label = np.eye(4), np.arange(K, dtype=np.int32)
        flow32 = np.ascontiguousarray(flow_ta_tb, np.float32)[None]
        both = a.valid & b.valid
        res = _one_job(homog_pcl_ta, eye, pose_a, pose_b, np.asarray(a.dims, np.float64), both, both, label, overlap=FIRST, keep_flow=True,
                       flow=flow32)
        if not np.shares_memory(res.flow, flow_ta_tb):
            won = res.point_box[0] >= 0  # (a float64 array takes the fp32 values of the points that changed)
            flow_ta_tb[won] = res.flow[0][won]
        return flow_ta_tb
    if not torch.is_tensor(flow_ta_tb) or flow_ta_tb.dtype != torch.float32 or not flow_ta_tb.is_contiguous():
        raise L.LisoHipError("flow_ta_tb must be a contiguous float32 device tensor [N, 3]")
    dev = flow_ta_tb.device
    pose_a, pose_b = a.get_poses(check_finite=False), b.get_poses(check_finite=False)
    K = a.valid.shape[0]
    eye, label = torch.eye(4, dtype=torch.float64, device=dev), torch.arange(K, dtype=torch.int32, device=dev)
    both = a.valid & b.valid
    _one_job(homog_pcl_ta, eye, pose_a, pose_b, a.dims.to(torch.float64), both, both, label, overlap=FIRST, keep_flow=True,
             flow=flow_ta_tb[None], want_label=False, want_box=False, want_count=False)
    return flow_ta_tb


def sample_jobs(clouds, poses_per_time, sizes, labels, odoms, directions=ALL_DIRECTIONS, *, counts=None, present=None, box_class=None,
                point_class=None):
    """The job tables of batched samples (see `sample_flow_labels`) -> (the arguments of `flow_labels` / `flow_labels_host` by name,
    the directions in use: those whose times the samples hold).  Job b * D + d is direction d of sample b; the sweeps are not copied."""
    xp = _xp(clouds)
    B, T, N = clouds.shape[:3]
    K = sizes.shape[1]
    dirs = [(int(a), int(b)) for a, b in directions if a < T and b < T]
    D = len(dirs)
    if D == 0 or tuple(odoms.shape[:2]) != (B, D):
        raise ValueError(f"odoms must hold one [4,4] per direction: expected [{B},{D},4,4], got {tuple(odoms.shape)}")
    stack = lambda parts: xp.stack(parts, 1).reshape((B * D,) + tuple(parts[0].shape[1:]))  # noqa: E731
    if present is None:
        present = np.ones((B, T, K), bool) if xp is np else torch.ones((B, T, K), dtype=torch.bool, device=clouds.device)
    sample = np.arange(B, dtype=np.int32) if xp is np else torch.arange(B, dtype=torch.int32, device=clouds.device)
    args = dict(
        pcl=clouds.reshape((B * T, N) + tuple(clouds.shape[3:])), counts=None if counts is None else counts.reshape(B * T),
        cloud_of=stack([sample * T + a for a, _ in dirs]), odom=odoms.reshape(B * D, 4, 4),
        pose_a=stack([poses_per_time[:, a] for a, _ in dirs]), pose_b=stack([poses_per_time[:, b] for _, b in dirs]),
        size=stack([sizes] * D), valid=stack([present[:, a] for a, _ in dirs]), has_b=stack([present[:, b] for _, b in dirs]),
        label=stack([labels] * D))
    if box_class is not None:
        per_direction = box_class.ndim == 3  # [B,D,K]: a gate of its own per direction (a negative class: no gate)
        args["box_class"] = box_class.reshape(B * D, K) if per_direction else stack([box_class] * D)
        args["point_class"] = point_class.reshape(B * T, N)
    return args, dirs


def sample_flow_labels(clouds, poses_per_time, sizes, labels, odoms, directions=ALL_DIRECTIONS, *, counts=None, present=None, box_class=None,
                       point_class=None, no_label=DUMMY_TRACK_ID, overlap=LAST):
    """The directed jobs of padded samples as ONE call.  For B samples of T sweeps and K box slots:
      clouds [B,T,n_max,C] float32 (counts int32 [B,T]), poses_per_time fp64 [B,T,K,4,4] (the pose of box k at every time),
      present bool [B,T,K] (the box exists at that time; None: everywhere), sizes [B,K,3], labels int32 [B,K],
      odoms [B,D,4,4]: odom_ta_tb of every direction, directions D pairs (a, b) of time indices,
      box_class int32 [B,K] (or [B,D,K], per direction; negative: not gated) with point_class int32 [B,T,n_max] (nuScenes'
      semantic gate, which the builder applies at t0 only), or neither.
    Unbatched inputs ([T,n_max,C] ...) are a batch of one.  Returns the keys the builders write, [B, ...] (or unbatched):
    `flow_t{a}_t{b}` float32 [n_max,3] per direction and, per source time a, `track_ids_mask_t{a}` int32 [n_max] (`no_label` where
    no box holds the point), `point_box_t{a}` int32 [n_max] and `num_lidar_pts_t{a}` int32 [K]."""
    unb = clouds.ndim == 3
    if unb:
        add = lambda v: None if v is None else v[None]  # noqa: E731
        clouds, poses_per_time, sizes, labels, odoms, counts, present, box_class, point_class = (
            add(v) for v in (clouds, poses_per_time, sizes, labels, odoms, counts, present, box_class, point_class))
    args, dirs = sample_jobs(clouds, poses_per_time, sizes, labels, odoms, directions, counts=counts, present=present, box_class=box_class,
                             point_class=point_class)
    B, D = clouds.shape[0], len(dirs)
    res = (flow_labels_host if is_np(clouds) else flow_labels)(**args, no_label=no_label, overlap=overlap)
    out = {}
    view = lambda v, d: v.reshape((B, D) + tuple(v.shape[1:]))[:, d]  # noqa: E731
    for d, (a, b) in enumerate(dirs):
        out[f"flow_t{a}_t{b}"] = view(res.flow, d)
        if f"track_ids_mask_t{a}" not in out:  # the same for every direction that starts at a
            out[f"track_ids_mask_t{a}"], out[f"point_box_t{a}"] = view(res.point_label, d), view(res.point_box, d)
            out[f"num_lidar_pts_t{a}"] = view(res.count, d)
    return {k: v[0] for k, v in out.items()} if unb else out
