"""Lidar odometry on the device (include/liso_odometry.h, csrc/odometry.hip).

* `lidar_odometry`     all frames of many padded sequences in one call -> `LidarOdometry` (no synchronisation, graph-capturable)
* `OdometryWorkspace`  the three stages one by one on a workspace whose tables can be looked at (tests, per-stage timing, `KissICP`)
* `relative_poses`     inv(a) b for stacks of poses
* `correct_kitti_scan_device`
"""
import collections
import ctypes
import dataclasses

import numpy as np
import torch

from liso_amd import _lib as L
from liso_amd.odometry.config import resolve_params

VOXEL_POINTS, KEY_HALF_SPAN, N_LAYOUT = 20, 1 << 20, 16  # LISO_ODOM_VOXEL_POINTS, LISO_ODOM_KEY_HALF_SPAN, LISO_ODOM_N_LAYOUT
LAYOUT = ("frame_ds", "n_ds", "source", "n_src", "map_keys", "map_count", "map_points", "n_map_voxels", "sse", "n_err")
WorldPoses = collections.namedtuple("WorldPoses", "w_T_sensor odom")


def make_cfg(S, F, N, C, map_voxels, **params):
    """-> (liso_odometry_cfg, bytes of workspace); raises when the sizes or parameters are refused"""
    p = resolve_params(**params)
    map_voxels = int(map_voxels)
    if map_voxels < 64 or map_voxels & (map_voxels - 1):
        raise L.LisoHipError(f"lidar odometry: map_voxels={map_voxels} is not a power of two >= 64")
    cfg = L.OdometryCfg(S, F, N, C, map_voxels, p["max_points_per_voxel"], p["max_num_iterations"], p["max_range"], p["min_range"],
                        p["voxel_size"], p["initial_threshold"], p["min_motion_th"], p["convergence_criterion"])
    ws_bytes = int(L.lib().liso_odometry_workspace_bytes(ctypes.byref(cfg)))
    if ws_bytes == 0:
        raise L.LisoHipError(f"lidar odometry: sizes refused (S={S}, F={F}, N={N}, C={C}, map_voxels={map_voxels}, {p}; F, N >= 1, C in "
                             f"(3, 4), max_range / (0.5 voxel_size) < {KEY_HALF_SPAN})")
    return cfg, ws_bytes


def _check_inputs(clouds, counts, n_frames):
    L.require_cuda(clouds, n_frames, *([] if counts is None else [counts]))
    S, F, N, C = clouds.shape
    assert clouds.dtype == torch.float32, clouds.dtype
    assert n_frames.shape == (S,) and n_frames.dtype == torch.int32, (n_frames.shape, n_frames.dtype)
    assert counts is None or (counts.shape == (S, F) and counts.dtype == torch.int32), (counts.shape, counts.dtype)
    return S, F, N, C


def relative_poses(a, b):
    """inv(a) b for float64 device tensors [..., 4, 4] of affine matrices"""
    L.require_cuda(a, b)
    assert a.shape == b.shape and a.shape[-2:] == (4, 4) and a.dtype == b.dtype == torch.float64, (a.shape, b.shape, a.dtype, b.dtype)
    a, b = a.contiguous(), b.contiguous()
    out = torch.empty(a.shape, dtype=torch.float64, device=a.device)
    with torch.cuda.device(a.device):
        L.check(L.lib().liso_odometry_relative_f64(a.numel() // 16, L.ptr(a), L.ptr(b), L.ptr(out), L.stream_ptr()), "odometry_relative")
    return out


@dataclasses.dataclass
class LidarOdometry:
    """the result tables of `lidar_odometry`, device tensors: poses float64 [S,F,4,4] (w_T_lidar, identity at and beyond n_frames), sigma
    float64 [S,F], n_source / n_iterations / converged int32 [S,F], map_overflow int32 [S]; `n_frames` is the call's own argument"""
    poses: torch.Tensor
    sigma: torch.Tensor
    n_source: torch.Tensor
    n_iterations: torch.Tensor
    converged: torch.Tensor
    map_overflow: torch.Tensor
    n_frames: torch.Tensor

    def odom(self, i, j):
        """inv(poses[:, i]) poses[:, j], float64 [S,4,4]: the motion that takes frame j's points into frame i"""
        return relative_poses(self.poses[:, i], self.poses[:, j])

    def kiss_odom_keys(self, i):
        """the six `kiss_odom_*` entries of the sample that starts at frame i (create_kitti_raw.py:159-173), each float64 [S,4,4]"""
        t = (i, i + 1, i + 2)
        return {f"kiss_odom_t{a}_t{b}": self.odom(t[a], t[b]) for a, b in ((0, 1), (1, 0), (0, 2), (2, 0), (1, 2), (2, 1))}

    def world_poses(self):
        """what the sequence tracker and the track mining take: `w_T_sensor` float64 [S,F,4,4] (the poses; frame 0 is the identity) and
        `odom` float64 [S,F,4,4] with odom[:, t] = inv(poses[:, t]) poses[:, t + 1], the identity for the last frame"""
        odom = relative_poses(self.poses, torch.cat([self.poses[:, 1:], self.poses[:, -1:]], dim=1))
        odom[:, -1] = torch.eye(4, dtype=torch.float64, device=odom.device)
        return WorldPoses(self.poses, odom)


@torch.no_grad()
def lidar_odometry(clouds, counts, n_frames, *, map_voxels, **params) -> LidarOdometry:
    """clouds float32 [S,F,N,C] (C 3 or 4), counts int32 [S,F] or None, n_frames int32 [S] (device tensors); `map_voxels`: slots of a
    sequence's map table, a power of two; the other keyword arguments are KISSConfig's parameters (config.DEFAULTS).  3 F + 9
    launches, nothing is read back: the caller looks at `map_overflow` when it wants to know whether `map_voxels` was enough."""
    S, F, N, C = _check_inputs(clouds, counts, n_frames)
    cfg, ws_bytes = make_cfg(S, F, N, C, map_voxels, **params)
    dev = clouds.device
    clouds, n_frames = clouds.contiguous(), n_frames.contiguous()
    counts = None if counts is None else counts.contiguous()
    new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)  # noqa: E731
    out = LidarOdometry(new((S, F, 4, 4), torch.float64), new((S, F), torch.float64), new((S, F), torch.int32), new((S, F), torch.int32),
                        new((S, F), torch.int32), new((S,), torch.int32), n_frames)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    if S > 0:
        with torch.cuda.device(dev):
            L.check(L.TIMER.launch("lidar_odometry", lambda: L.lib().liso_odometry_sequences(
                ctypes.byref(cfg), L.ptr(clouds), None if counts is None else L.ptr(counts), L.ptr(n_frames), L.ptr(out.poses), L.ptr(out.sigma),
                L.ptr(out.n_source), L.ptr(out.n_iterations), L.ptr(out.converged), L.ptr(out.map_overflow), L.ptr(ws), ws_bytes,
                L.stream_ptr())), "lidar_odometry")
    return out


class OdometryWorkspace:
    """The stages of include/liso_odometry.h one at a time for S sequences of up to F frames of up to N rows of C floats.  The result
    tensors (`poses`, `sigma`, `n_source`, `n_iterations`, `converged`, `map_overflow`) and the workspace belong to the object;
    `table(name)` views a workspace table (LAYOUT), `map_voxels_of(s, frame)` reads a sequence's map as the host restatement keeps it."""

    def __init__(self, S, F, N, C, device, *, map_voxels, **params):
        self.cfg, self.ws_bytes = make_cfg(S, F, N, C, map_voxels, **params)
        self.S, self.F, self.N, self.C, self.V, self.device = S, F, N, C, int(map_voxels), torch.device(device)
        new = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device=self.device)  # noqa: E731
        self.poses = torch.eye(4, dtype=torch.float64, device=self.device).repeat(S, F, 1, 1)
        self.sigma, self.n_source = new((S, F), torch.float64), new((S, F), torch.int32)
        self.n_iterations, self.converged, self.map_overflow = new((S, F), torch.int32), new((S, F), torch.int32), new((S,), torch.int32)
        self.ws = torch.zeros(self.ws_bytes, dtype=torch.uint8, device=self.device)
        offsets = (ctypes.c_size_t * N_LAYOUT)()
        L.check(L.lib().liso_odometry_workspace_layout(ctypes.byref(self.cfg), offsets), "odometry_workspace_layout")
        self.offsets = dict(zip(LAYOUT, offsets))

    def _call(self, what, fn, *args):
        with torch.cuda.device(self.device):
            L.check(L.TIMER.launch(what, lambda: fn(ctypes.byref(self.cfg), *args, L.ptr(self.ws), self.ws_bytes, L.stream_ptr())), what)

    def preprocess(self, frame, clouds, counts, n_frames, cfg=None, n_source=None):
        """range filter and the two downsamples of frame `frame` of clouds float32 [S,F,N,C] -> the workspace's frame_ds and source"""
        S, F, N, C = _check_inputs(clouds, counts, n_frames)
        assert (S, N, C) == (self.S, self.N, self.C) and clouds.is_contiguous(), (clouds.shape, self.S, self.N, self.C)
        cfg, n_source = self.cfg if cfg is None else cfg, self.n_source if n_source is None else n_source
        assert F == cfg.max_frames and n_source.shape == (S, F), (F, cfg.max_frames, n_source.shape)
        with torch.cuda.device(self.device):
            L.check(L.TIMER.launch("odometry_preprocess", lambda: L.lib().liso_odometry_preprocess(
                ctypes.byref(cfg), int(frame), L.ptr(clouds), None if counts is None else L.ptr(counts), L.ptr(n_frames), L.ptr(n_source),
                L.ptr(self.ws), self.ws_bytes, L.stream_ptr())), "odometry_preprocess")

    def register(self, frame, n_frames, guess=None, sigma=None):
        """frame `frame`'s source against the map; guess float64 [S,4,4] and sigma float64 [S] given together or not at all"""
        L.require_cuda(n_frames, *([] if guess is None else [guess, sigma]))
        if guess is not None:
            assert guess.shape == (self.S, 4, 4) and sigma.shape == (self.S,) and guess.dtype == sigma.dtype == torch.float64
            guess, sigma = guess.contiguous(), sigma.contiguous()
        self._call("odometry_register", L.lib().liso_odometry_register, int(frame), L.ptr(n_frames), None if guess is None else L.ptr(guess),
                   None if sigma is None else L.ptr(sigma), L.ptr(self.poses), L.ptr(self.sigma), L.ptr(self.n_iterations),
                   L.ptr(self.converged))

    def map_update(self, frame, n_frames, poses=None):
        """frame_ds moved by poses[:, frame] (default: the object's own) into the map"""
        poses = self.poses if poses is None else poses
        L.require_cuda(n_frames, poses)
        assert poses.shape == (self.S, self.F, 4, 4) and poses.dtype == torch.float64 and poses.is_contiguous(), (poses.shape, poses.dtype)
        self._call("odometry_map_update", L.lib().liso_odometry_map_update, int(frame), L.ptr(n_frames), L.ptr(poses), L.ptr(self.map_overflow))

    def table(self, name):
        S, N, V = self.S, self.N, self.V
        shape, dtype = {"frame_ds": ((S, N, 3), torch.float32), "n_ds": ((S,), torch.int32), "source": ((S, N, 3), torch.float32),
                        "n_src": ((S,), torch.int32), "map_keys": ((S, 2, V), torch.int64), "map_count": ((S, 2, V), torch.int32),
                        "map_points": ((S, 2, V, VOXEL_POINTS, 3), torch.float32), "n_map_voxels": ((S,), torch.int32),
                        "sse": ((S,), torch.float64), "n_err": ((S,), torch.int32)}[name]
        nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        return self.ws[self.offsets[name]:self.offsets[name] + nbytes].view(dtype).view(shape)

    def frame_ds(self, s):
        return self.table("frame_ds")[s, :int(self.table("n_ds")[s])].cpu().numpy()

    def source(self, s):
        return self.table("source")[s, :int(self.table("n_src")[s])].cpu().numpy()

    def map_voxels_of(self, s, frame):
        """{packed key (host.pack_keys) -> float32 [k,3] in stored order} of sequence s after the map update of frame `frame`"""
        t = frame & 1
        keys, count, points = (self.table(k)[s, t].cpu().numpy() for k in ("map_keys", "map_count", "map_points"))
        used = np.nonzero(keys)[0]
        assert (keys[used] < 0).all(), "a key without its occupied bit"
        return {int(keys[i] & 0x7FFFFFFFFFFFFFFF): points[i, :count[i]].copy() for i in used}


def correct_kitti_scan_device(points):
    """float64 device tensor [n,3] -> the corrected sweep, a new tensor"""
    L.require_cuda(points)
    assert points.dim() == 2 and points.shape[1] == 3 and points.dtype == torch.float64, (points.shape, points.dtype)
    points = points.contiguous()
    out = torch.empty_like(points)
    with torch.cuda.device(points.device):
        L.check(L.lib().liso_correct_kitti_scan_f64(points.shape[0], L.ptr(points), L.ptr(out), L.stream_ptr()), "correct_kitti_scan")
    return out
