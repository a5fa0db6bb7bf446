"""KITTI's lidar row and column of every point (reference liso/datasets/kitti/kitti_range_image_projection_helper.py:4-29, used by
`add_lidar_rows_to_kitti_sample`, liso/datasets/torch_dataset_commons.py:78-86): a row starts wherever the flipped azimuth jumps
back by more than the threshold between two points that follow one another in the file; the column is the azimuth's bin.

numpy clouds [N,>=2] run the host path, which is the reference's own numpy (float32 `arctan2`).  Device tensors [N,C] or a padded
batch [B,N,C] with `counts` go through liso_kitti_rows_cols_f32 (include/liso_flow_labels.h): one launch, no host read.  The device
evaluates atan2 in fp64 and rounds to fp32, so an azimuth can differ from numpy's in its last bit; the integer outputs differ only
for a point whose azimuth difference lies within a few ulp of the threshold or whose column value lies within a few ulp of an
integer.  Entries at or behind a cloud's count are -1 (255 after the uint8 cast of `add_lidar_rows_to_kitti_sample`).
"""
import numpy as np
import torch

from liso_amd import _lib as L
from liso_amd.utils.device_args import cloud3, counts_arg, is_np, opt_ptr as _p

JUMP_THRESHOLD = -0.005  # reference :5
NUM_COLUMNS = 2000       # reference :19


def rows_cols_device(pointcloud, counts=None, threshold=JUMP_THRESHOLD, auto_correct=False, num_columns=NUM_COLUMNS, want_rows=True,
                     want_cols=True):
    """device cloud [N,C] / [B,N,C] float32 -> (rows, cols) int32 [N] / [B,N]; what is not wanted is None"""
    p3 = cloud3(pointcloud)
    B, N, stride = p3.shape
    counts = counts_arg(counts, p3)
    rows = torch.empty((B, N), dtype=torch.int32, device=p3.device) if want_rows else None
    cols = torch.empty((B, N), dtype=torch.int32, device=p3.device) if want_cols else None
    if N > 0:
        with torch.cuda.device(p3.device):
            L.check(L.lib().liso_kitti_rows_cols_f32(B, N, stride, _p(p3), _p(counts), float(threshold), int(bool(auto_correct)),
                                                     int(num_columns), _p(rows), _p(cols), L.stream_ptr()), "kitti rows and columns")
    if pointcloud.dim() == 2:
        rows, cols = (None if v is None else v[0] for v in (rows, cols))
    return rows, cols


def find_jumps(pointcloud, threshold=JUMP_THRESHOLD, auto_correct=False, counts=None):
    """reference :4-16 -- int32 row of every point"""
    if not is_np(pointcloud):
        return rows_cols_device(pointcloud, counts, threshold, auto_correct, want_cols=False)[0]
    azimuth_flipped = -np.arctan2(pointcloud[:, 1], -pointcloud[:, 0])
    jumps = np.argwhere(np.ediff1d(azimuth_flipped) < threshold)
    rows = np.zeros(shape=azimuth_flipped.shape, dtype=np.int32)
    rows[jumps + 1] = 1
    rows = np.cumsum(rows, dtype=np.int32)
    if rows.size and rows[-1] < 63 and auto_correct:
        rows += 63 - rows[-1]
    return rows


def find_cols(pointcloud, num_columns=NUM_COLUMNS, counts=None):
    """reference :19-23 -- int32 column of every point"""
    if not is_np(pointcloud):
        return rows_cols_device(pointcloud, counts, num_columns=num_columns, want_rows=False)[1]
    azimuth = np.arctan2(pointcloud[:, 1], pointcloud[:, 0])
    with np.errstate(invalid="ignore"):
        return ((num_columns - 1) * (np.pi - azimuth) / (2 * np.pi)).astype(np.int32)


def kitti_pcl_projection_get_rows_cols(pointcloud, num_columns=NUM_COLUMNS, counts=None):
    """reference :26-29 -> (rows, cols)"""
    if not is_np(pointcloud):
        return rows_cols_device(pointcloud, counts, num_columns=num_columns)
    return find_jumps(pointcloud), find_cols(pointcloud, num_columns=num_columns)


def add_lidar_rows_to_kitti_sample(sample_content, time_keys, pcl_key="pcl_"):
    """reference torch_dataset_commons.py:78-86 -- `lidar_rows_<tk>` uint8 for every `pcl_<tk>` of the sample, in place.  A device
    cloud may be a padded batch; its `counts_<tk>` (int32 [B]) is used when the sample holds one."""
    for tk in time_keys:
        key = f"pcl_{tk}"
        if key in sample_content:
            pcl = sample_content[key]
            if is_np(pcl):
                sample_content[f"lidar_rows_{tk}"] = kitti_pcl_projection_get_rows_cols(pcl)[0].astype(np.uint8)
            else:
                rows = find_jumps(pcl, counts=sample_content.get(f"counts_{tk}"))
                sample_content[f"lidar_rows_{tk}"] = rows.to(torch.uint8)
