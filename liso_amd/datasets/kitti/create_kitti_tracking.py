"""The label functions of the reference's liso/datasets/kitti/create_kitti_tracking.py (:14-17, :340-387), under its module path:
numpy arrays run the host path, device tensors the kernel (liso_amd/datasets/flow_labels.py)."""
from liso_amd.datasets.flow_labels import extract_lidar_flow_ta_tb, get_points_in_box_mask  # noqa: F401
