"""Mirror of liso/eval/eval_ours.py: the helper the tracking path calls (tracking.py:821-835) and `run_val` (:120-757), the
detector's validation pass, with all the matching on the device (liso_amd/eval/det_validation.py)."""
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


KITTI_CAM_OPENING_ANGLE_DEG = (-41.95, 40.16)  # reference :98-99
MIN_NUM_PTS_PER_BOX = 10  # reference :390


@torch.no_grad()
def kitti_annotated_fov_mask(pred_boxes: Shape, pcl_full_w_ground):
    """run_val :386-403 for a padded batch, without a host read: which of the boxes [B,P] hold at least 10 points of
    `pcl_full_w_ground` [B,N,>=3] that lie inside the opening angle of KITTI's camera, with the box height set to 1000 as
    `count_box_points_in_kitti_annotated_fov` does.  Built from the batched `points_in_boxes`; nothing is indexed by a boolean mask:
    the points outside the angle are replaced by NaN rows, which are inside no box (the kernel's own `point_valid` argument gates only
    its flow sum, include/liso_tracking.h).  The inside test is that kernel's, not fit_box_z's."""
    from liso_amd.tracker.box_points import dense_boxes, points_in_boxes

    pts = pcl_full_w_ground[..., :3].float()
    angles = torch.atan2(pts[..., 1], pts[..., 0])
    lo, hi = (a / 180.0 * np.pi for a in KITTI_CAM_OPENING_ANGLE_DEG)
    in_fov = (angles >= lo) & (angles <= hi)
    pts = torch.where(in_fov[..., None], pts, float("nan")).contiguous()
    boxes7 = dense_boxes(pred_boxes).clone()
    boxes7[..., 5] = 1000.0
    boxes7 = torch.where(pred_boxes.valid[..., None], boxes7, torch.zeros_like(boxes7))  # (padding rows hold NaN)
    return points_in_boxes(boxes7, pts)["count"] >= MIN_NUM_PTS_PER_BOX


def _log_val_images(cfg, writer, writer_prefix, step, batch, pred):
    from liso_amd.visu.bbox_image import log_box_movement
    from liso_amd.visu.pcl_image import create_occupancy_pcl_image

    canvas = batch.get("occupancy_f32_ta")
    if canvas is None:
        canvas = torch.stack([create_occupancy_pcl_image(p, cfg.data.bev_range_m, cfg.data.img_grid_size) for p in batch["pcls"]]).permute(0, 3, 1, 2)
    log_box_movement(cfg=cfg, writer=writer, global_step=step, sample_data_a={"occupancy_f32_ta": canvas, "gt": {"boxes": batch["gt_boxes"]}},
                     sample_data_b={"occupancy_f32_ta": batch.get("occupancy_f32_tb"), "gt": {"boxes": batch.get("gt_boxes_tb")}}, pred_boxes=pred,
                     writer_prefix=writer_prefix)


@torch.no_grad()
def run_val(cfg, val_batches, box_predictor, writer_prefix: str = "", max_num_steps=None, logit_threshold=-1.0e32, dataset_kind="kitti",
            movable_class_names=("car", "pedestrian", "cyclist"), class_idxs=None, class_frequencies=None, generator=None,
            filter_to_kitti_annotated_fov=None, validator=None, waymo_metrics=False, nuscenes_metrics=False, sigmoid_scores=None,
            image_writer=None, num_image_steps=0):
    """The detector's validation pass (reference :120-757).  Per batch of `val_batches` -- dictionaries with `pcls` (the list of
    clouds the detector takes), `gt_boxes` and `benchmark_gt_boxes` (padded Shapes [B,G*] on the device) and optionally
    `pcl_full_w_ground` [B,N,>=3] -- it runs `box_predictor.predict_boxes` with run_val's defaults (:361-386), the optional KITTI rule
    (:386-403; default: whenever dataset_kind == "kitti" and the batch has `pcl_full_w_ground`) and
    `DetectionValidator.update_batch`; no host read until the final `compute()`.  -> the metric dictionary under the reference's
    tags `<writer_prefix>final_result/...`.  The caller sets the network's mode (`DetectorTrainer.eval_model` does).

    Class transfer (:406-447) draws every prediction's class on the device from `generator` (`class_frequencies`: the dataset's
    movable_class_frequencies -> torch.multinomial; else torch.randint), not from numpy's global state.
    waymo_metrics=True adds the reference's Waymo-style L1 / L2 collections (`WaymoObjectDetectionMetrics`, :249-255, 741-747; tags
    `<writer_prefix>final_result/WAYMO/detection_metrics/<lo>_<hi>m<criterion>/overall/<L1|L2>/AP@0.4`, ...: the reference writes no
    separator before the criterion), matched by optimal assignment on the device in one more launch per ground-truth set, and makes
    dataset_kind="waymo" buildable (`DetectionValidator.for_run_val`).  With the default the result's keys are unchanged.
    nuscenes_metrics=True adds the reference's nuScenes detection metrics (`NuscenesObjectDetectionMetrics`, :209, 493-519, 729-740;
    liso_amd/eval/nuscenes_metrics.py) for any dataset kind: `<writer_prefix>final_result/NUSC_OFFICIAL/detection_metrics/mAP`,
    `/mATE` ... `/mAAE`, `/NDS`, `/movable/AP` ..., one more launch per batch, and makes dataset_kind="nuscenes" buildable with its
    per-class collection under `.../NUSC_OFFICIAL/per_class/detection_metrics/`.  `sigmoid_scores`: these collections read the fp32
    sigmoid of the scores; default: the reference's rule (:494-509) for the detector trained here,
    cfg.box_prediction.activations.probs == "none" (pass False for a predictor whose scores are probabilities already, as the
    reference does for its flow-cluster detector).  With the default the result's keys and values are unchanged.
    image_writer (any object with `add_images(tag, array, global_step=, dataformats=)`) with num_image_steps > 0: each of the first
    `num_image_steps` batches also makes the box-movement picture (reference :615-625; liso_amd/visu/bbox_image.py
    `log_box_movement`) of its ground truth and the predictions the metrics see, on the device, under
    `<writer_prefix>RECONSTRUCTION_TARGETS_t0_t1` with the batch's index as the step.  The canvas is the batch's `occupancy_f32_ta`
    [B,1,H,W] when it carries one, else the occupancy image of its clouds on cfg.data.img_grid_size.  A batch that also carries
    `occupancy_f32_tb` (and `gt_boxes_tb`) gets the third canvas, the next sweep's ground truth over this one's in light blue.  With the defaults nothing is
    drawn: the result and the launches of a batch are unchanged.
    Out of scope: flow metrics (liso_amd/slim/validation.py has them), the range-view image, PDFs, exports and TensorBoard writers."""
    from liso_amd.eval.det_validation import DetectionValidator

    moving = cfg.get("validation", {}).get("obj_is_moving_velocity_thresh", 0.1)  # reference :145-149
    if validator is None:
        if class_idxs is None:
            class_idxs = tuple(range(len(movable_class_names)))
        if sigmoid_scores is None:
            sigmoid_scores = cfg.get("box_prediction", {}).get("activations", {}).get("probs") == "none"
        validator = DetectionValidator.for_run_val(dataset_kind, movable_class_names, class_idxs, moving, class_frequencies, generator,
                                                   waymo_metrics=waymo_metrics, nuscenes_metrics=nuscenes_metrics,
                                                   sigmoid_scores=bool(sigmoid_scores))
    for val_step, batch in enumerate(val_batches):
        if max_num_steps is not None and val_step > max_num_steps:  # (the reference's own off-by-one, :260)
            break
        pred, _, counts = box_predictor.predict_boxes(None, batch["pcls"], logit_threshold=logit_threshold)
        full = batch.get("pcl_full_w_ground")
        use_fov = (dataset_kind == "kitti" and full is not None) if filter_to_kitti_annotated_fov is None else filter_to_kitti_annotated_fov
        if use_fov:
            pred.valid = pred.valid & kitti_annotated_fov_mask(pred, full)
        validator.update_batch(batch["gt_boxes"], batch.get("benchmark_gt_boxes"), pred)
        if image_writer is not None and val_step < num_image_steps:
            _log_val_images(cfg, image_writer, writer_prefix, val_step, batch, pred)
    return validator.compute(writer_prefix)
