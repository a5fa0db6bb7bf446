"""Lidar odometry: w_T_lidar for every sweep of a sequence, from the sweeps alone (include/liso_odometry.h).

The reference's dataset builders take these poses from the third-party `kiss_icp` package and store them as `kiss_odom_*`; its
training configuration selects them (`odom_source: "kiss_icp"`).  Here the same pipeline is stated once in numpy / fp64 (`host.py`,
the yardstick) and run on the device for many padded sequences at a time (`device.py`).  Parity with the package itself is unpinned:
DESIGN.md lists the choices that are this package's own.
"""
from liso_amd.odometry.config import DEFAULTS, KISSConfig, resolve_params  # noqa: F401
from liso_amd.odometry.device import (LidarOdometry, OdometryWorkspace, correct_kitti_scan_device, lidar_odometry,  # noqa: F401
                                      relative_poses)
from liso_amd.odometry.host import (HostOdometry, correct_kitti_scan_host, exp_se3, lidar_odometry_host, voxel_down_sample)  # noqa: F401
from liso_amd.odometry.kiss_icp import KissICP  # noqa: F401


def correct_kitti_scan(points):
    """KITTI's vertical-angle correction of a sweep float64 [n,3] (create_kitti_raw.py:30-36): a CUDA tensor takes the device path and
    comes back as a tensor, anything else the host path and comes back as a numpy array"""
    import torch

    if isinstance(points, torch.Tensor) and points.is_cuda:
        return correct_kitti_scan_device(points)
    return correct_kitti_scan_host(points)
