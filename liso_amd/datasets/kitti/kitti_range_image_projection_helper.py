"""The reference's liso/datasets/kitti/kitti_range_image_projection_helper.py under its module path
(liso_amd/datasets/range_projection.py)."""
from liso_amd.datasets.range_projection import find_cols, find_jumps, kitti_pcl_projection_get_rows_cols  # noqa: F401
