"""BoxLearner: network selector + activations + decode.  Mirror of liso/networks/simple_net/simple_net.py:28-151
for the CenterPoint-pillar path (the other selectable networks are out of scope)."""
from typing import Dict, Tuple

import numpy as np
import torch

from liso_amd.kabsch.output_modification import maybe_flatten_anchors_except_for, output_modification
from liso_amd.kabsch.shape_utils import Shape
from liso_amd.networks.simple_net.centerpoint_net import CenterPointStyleNet
from liso_amd.networks.simple_net.simple_net_utils import allowed_activations
from liso_amd.utils.bev_utils import get_metric_voxel_center_coords


def get_centermaps_output_grid_size(cfg, output_grid_size):
    """liso/datasets/torch_dataset_commons.py:106-130 (centerpoint branch)"""
    if cfg.network.name != "centerpoint":
        return None
    ds = 4 if cfg.network.centerpoint.use_baseline_parameters else 8
    if cfg.network.centerpoint.reduce_receptive_field == 1:
        ds //= 2
    elif cfg.network.centerpoint.reduce_receptive_field != 0:
        raise NotImplementedError()
    return output_grid_size // ds


class BoxLearner(torch.nn.Module):
    def __init__(self, cfg) -> None:
        super().__init__()
        self.cfg = cfg
        self.activations = {k: allowed_activations[v] for k, v in cfg.box_prediction.activations.items()}
        if cfg.network.name != "centerpoint":
            raise NotImplementedError(f"{cfg.network.name}: only the centerpoint network is on the hot path")
        self.model = CenterPointStyleNet(cfg)
        shape = get_centermaps_output_grid_size(cfg, np.array(cfg.data.img_grid_size))
        # a non-trainable Parameter, hence part of the state_dict (reference :59-68)
        self.pillar_center_coors_m = torch.nn.parameter.Parameter(
            torch.from_numpy(get_metric_voxel_center_coords(
                bev_range_x=cfg.data.bev_range_m[0], bev_range_y=cfg.data.bev_range_m[1],
                dataset_img_shape=shape).astype(np.float32)[..., 0:2]), requires_grad=False)

    def forward(self, img_t0, pcls_t0, gt_boxes=None, centermaps_gt=None, train=True, decode=True, canvas=None) -> Tuple[Shape, Dict]:
        """reference :70-109.  `decode=False` (extension): return the raw network maps only -- (None, None, raw, aux) --
        for callers that run activations + decode + loss fused (liso_amd.losses.fused_centerpoint)."""
        raw_box_vars, aux_outputs = self.model(img_t0, pcls_t0, canvas=canvas) if canvas is not None else self.model(img_t0, pcls_t0)
        if not decode:
            return None, None, raw_box_vars, aux_outputs
        decoded, activated = self.apply_all_output_modifications(raw_box_vars=raw_box_vars, gt_boxes=gt_boxes,
                                                                 centermaps_gt=centermaps_gt)
        flat = maybe_flatten_anchors_except_for({k: v.clone() for k, v in decoded.items()}, ())
        return Shape(**flat), decoded, activated, aux_outputs

    @torch.no_grad()
    def predict_boxes(self, img_t0, pcls_t0, *, overlap_threshold=None, pre_nms_max_boxes=None, post_nms_max_boxes=500,
                      logit_threshold=-1e32, sigmoid_probs=False, canvas=None):
        """Decoding forward (`train=False`) + batched rotated NMS on the device (liso_amd.utils.nms_iou.iou_based_nms_batched):
        (Shape [B,P], keep_idx int64 [B,P], counts int32 [B]), P = post_nms_max_boxes, no host sync.  The module's mode is the
        caller's.
        The defaults are run_val's post-processing (liso/eval/eval_ours.py:361-386): slots with a logit below `logit_threshold`
        take no part, the boxes are ranked by sigmoid(probs) when `activations.probs == "none"` (by the probs otherwise), no
        pre-NMS cut, 500 boxes kept, raw probs returned.  `pre_nms_max_boxes=1000, post_nms_max_boxes=100, sigmoid_probs=True`
        is the tracker's (liso/tracker/tracking.py:710-740): the kept boxes carry the sigmoid probs (the tracker applies no
        logit threshold; the default -1e32 drops only slots whose logit is -inf or below -1e32).
        `overlap_threshold=None` reads cfg.nms_iou_threshold.  Ties in the ranking keep ascending slot index."""
        from liso_amd.utils.nms_iou import iou_based_nms_batched

        boxes, _, _, _ = self.forward(img_t0, pcls_t0, train=False, canvas=canvas)
        thr = self.cfg.nms_iou_threshold if overlap_threshold is None else overlap_threshold
        logits = boxes.probs[..., 0]
        key = torch.sigmoid(logits) if self.cfg.box_prediction.activations.probs == "none" else logits
        if sigmoid_probs and self.cfg.box_prediction.activations.probs == "none":
            boxes.probs = torch.sigmoid(boxes.probs)
        return iou_based_nms_batched(boxes, thr, pre_nms_max_boxes, post_nms_max_boxes, scores=key, logit_threshold=logit_threshold,
                                     threshold_values=logits)

    def apply_all_output_modifications(self, *, raw_box_vars, gt_boxes=None, centermaps_gt=None):
        """reference :111-151"""
        activated = {k: self.activations[k](v) for k, v in raw_box_vars.items()}
        decoded = output_modification({k: v.clone() for k, v in activated.items()}, self.cfg.box_prediction,
                                      self.cfg.data, "boxes", self.pillar_center_coors_m)
        return decoded, activated


def select_network(cfg, device):
    """reference :154-176 (centerpoint only)"""
    return BoxLearner(cfg).to(device)
