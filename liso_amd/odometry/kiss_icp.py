"""`KissICP`: the odometry behind kiss_icp's pipeline interface (`register_frame`, `.poses`), so that the reference's dataset builders
run with an import swap.  numpy sweeps take the host restatement; CUDA tensors take the device stages with S = 1."""
import ctypes

import numpy as np
import torch

from liso_amd import _lib as L
from liso_amd.odometry.config import KISSConfig
from liso_amd.odometry.device import OdometryWorkspace
from liso_amd.odometry.host import HostOdometry


class KissICP:
    """`register_frame(frame, timestamps=None)` estimates the pose of the next sweep ([n, >=3]: x, y, z first; any float type, taken
    as float32); `poses` is the list of w_T_lidar so far, float64 [4,4] numpy arrays (the device path reads them back when asked).
    `max_points` and `map_voxels` size the device path: rows per sweep and slots of the map table (a power of two)."""

    def __init__(self, config: KISSConfig = None, max_points=1 << 18, map_voxels=1 << 18):
        self.config = KISSConfig() if config is None else config
        self.max_points, self.map_voxels = int(max_points), int(map_voxels)
        self._host = self._dev = None
        self._n = 0

    def register_frame(self, frame, timestamps=None):
        if isinstance(frame, torch.Tensor) and frame.is_cuda:
            assert self._host is None, "a sequence stays on the path its first sweep took"
            return self._register_device(frame)
        assert self._dev is None, "a sequence stays on the path its first sweep took"
        if self._host is None:
            self._host = HostOdometry(**self.config.params())
        self._n += 1
        return self._host.step(np.asarray(frame.cpu() if isinstance(frame, torch.Tensor) else frame)[:, :3].astype(np.float32))

    def _register_device(self, frame):
        assert frame.dim() == 2 and frame.shape[1] >= 3 and frame.shape[0] <= self.max_points, (frame.shape, self.max_points)
        if self._dev is None or self._n >= self._dev.F:  # (the tables do not depend on F: more room for poses, the same workspace)
            F = 64 if self._dev is None else 2 * self._dev.F
            grown = OdometryWorkspace(1, F, self.max_points, 3, frame.device, map_voxels=self.map_voxels, **self.config.params())
            if self._dev is not None:
                for k in ("poses", "sigma", "n_source", "n_iterations", "converged"):
                    getattr(grown, k)[:, :self._dev.F] = getattr(self._dev, k)
                grown.map_overflow, grown.ws = self._dev.map_overflow, self._dev.ws
            self._dev = grown
            # the sweep's own buffers: one frame of one sequence
            self._one = L.OdometryCfg(*[getattr(grown.cfg, k) for k, _ in L.OdometryCfg._fields_])
            self._one.max_frames = 1
            assert L.lib().liso_odometry_workspace_bytes(ctypes.byref(self._one)) == grown.ws_bytes
            self._cloud = torch.empty((1, 1, self.max_points, 3), dtype=torch.float32, device=frame.device)
            self._count = torch.empty((1, 1), dtype=torch.int32, device=frame.device)
            self._n_src = torch.empty((1, 1), dtype=torch.int32, device=frame.device)
            self._ones = torch.ones(1, dtype=torch.int32, device=frame.device)
        d, f = self._dev, self._n
        n = frame.shape[0]
        self._cloud[0, 0, :n] = frame[:, :3].to(torch.float32)
        self._count.fill_(n)
        all_frames = torch.full((1,), f + 1, dtype=torch.int32, device=frame.device)
        d.preprocess(0, self._cloud, self._count, self._ones, cfg=self._one, n_source=self._n_src)
        d.n_source[:, f] = self._n_src[:, 0]
        d.register(f, all_frames)
        d.map_update(f, all_frames)
        self._n += 1
        return d.poses[0, f]

    @property
    def poses(self):
        if self._dev is not None:
            return list(self._dev.poses[0, :self._n].cpu().numpy())
        return [] if self._host is None else list(self._host.poses)

    def device_result(self):
        """the device path's tables so far, as `LidarOdometry`'s fields are laid out (S = 1, the frames registered)"""
        d, n = self._dev, self._n
        return {k: getattr(d, k)[:, :n] for k in ("poses", "sigma", "n_source", "n_iterations", "converged")} | {"map_overflow": d.map_overflow}
