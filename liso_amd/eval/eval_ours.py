"""Mirror of the one function of liso/eval/eval_ours.py that the tracking path calls (tracking.py:821-835)."""
import numpy as np
import torch

from liso_amd.kabsch.shape_utils import Shape
from liso_amd.networks.flow_cluster_detector.flow_cluster_detector import fit_bev_box_z_and_height_using_points_in_box


@torch.no_grad()
def count_box_points_in_kitti_annotated_fov(pred_boxes: Shape, pcl):
    """reference :96-116 -- points of `pcl` [N,>=3] (device) inside each of the unbatched boxes [K] and inside the opening angle of
    KITTI's camera, the only region KITTI annotates.  For a whole sequence at once: liso_amd.tracker.frame_prep."""
    kitti_cam_min_opening_angle__deg = -41.95
    kitti_cam_max_opening_angle__deg = 40.16
    angles = torch.atan2(pcl[:, 1], pcl[:, 0])
    min_angle = kitti_cam_min_opening_angle__deg / 180.0 * np.pi
    max_angle = kitti_cam_max_opening_angle__deg / 180.0 * np.pi
    pcl_in_cam_fov = pcl[(angles >= min_angle) & (angles <= max_angle)]
    num_pts_in_box, _, _ = fit_bev_box_z_and_height_using_points_in_box(pcl_in_cam_fov[:, :3], pred_boxes, box_height=1000.0)
    return num_pts_in_box
