"""GPU: DetectorTrainer.summary_images -- a dictionary of device pictures beside the training step, which never calls it."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _kernel_launches(fn):
    from torch.profiler import ProfilerActivity, profile

    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "memcpy" not in e.name.lower()
               and "memset" not in e.name.lower())


def test_summary_images_beside_the_step():
    from liso_amd.datasets.synthetic import detector_batch
    from liso_amd.trainer import DetectorTrainer
    from liso_amd.utils.config import default_cfg

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    cfg = default_cfg(grid=64, bev_range_m=40.0)
    cfg.logging.max_log_img_batches = 2
    tr = DetectorTrainer(cfg, dev, total_steps=16)
    pcls, targets = detector_batch(3, 3, dev, n_points=4000, grid=64, bev_range_m=40.0)
    for _ in range(5):  # (the first steps pack weight panels and warm caches: their launch counts are not the step's)
        tr.step(pcls, targets)
    n_before = [_kernel_launches(lambda: tr.step(pcls, targets)) for _ in range(2)]
    assert n_before[0] == n_before[1], n_before  # the count has settled
    n_step = n_before[1]
    state = {k: v.clone() for k, v in tr.net.state_dict().items()}

    pics = tr.summary_images(pcls, targets)
    assert set(pics) == {"_post_nms_SHAPES_COMPARISON_PRED_GT", "TARGET_CENTER_HEATMAP"}
    boxes_pic, heat = pics["_post_nms_SHAPES_COMPARISON_PRED_GT"], pics["TARGET_CENTER_HEATMAP"]
    assert boxes_pic.is_cuda and boxes_pic.dtype == torch.float32 and tuple(boxes_pic.shape) == (2, 64, 64, 3)  # the first two of three samples
    assert heat.is_cuda and heat.dtype == torch.float32 and tuple(heat.shape) == (2, 16, 16, 1)
    assert torch.equal(heat, targets["probs"][:2])
    pic = boxes_pic.cpu().numpy()
    assert np.isfinite(pic).all() and pic.min() >= 0.0 and pic.max() <= 1.0
    assert ((pic[..., 2] > 0.39) & (pic[..., 2] < 0.41) & (pic[..., 1] >= 0.5)).sum() > 10, "predictions come in `summer` colours"
    assert tr.net.training  # the mode is the one it had
    for k, v in tr.net.state_dict().items():
        assert torch.equal(v, state[k]), k  # no parameter or buffer changed

    # given boxes are drawn as they are given: none valid leaves the occupancy image
    tr.net.eval()
    given, _, _ = tr.net.predict_boxes(None, pcls)
    tr.net.train()
    given.valid = torch.zeros_like(given.valid)
    empty = tr.summary_images(pcls, targets, pred_boxes=given)["_post_nms_SHAPES_COMPARISON_PRED_GT"].cpu().numpy()
    assert set(np.unique(empty).tolist()) <= {0.0, 1.0} and (empty[..., 0] == empty[..., 2]).all()

    # The step launches no more than before the pictures were made, and the same again from the second step on.  The first step
    # after them may launch fewer: the pictures' forward pass leaves the packed weight panels of the current weights in the version
    # cache of liso_amd/utils/conv_panels.py, which that step's forward pass then finds (measured on an MI355X with two warm-up
    # steps: 335 launches before, 315 in the first step after).
    n_after = [_kernel_launches(lambda: tr.step(pcls, targets)) for _ in range(2)]
    print(f"step launches: {n_before} before the pictures, {n_after} after")
    assert n_after[0] <= n_step and n_after[1] == n_step, (n_before, n_after)
