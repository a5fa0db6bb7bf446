"""GPU: run_val's opt-in pictures -- the box-movement image arrives under the reference's tag, and nothing changes without a writer."""
import numpy as np
import pytest
import torch

from tests.det_val_cases import pad_batch, scene

pytestmark = pytest.mark.gpu


class _Recorder:
    def __init__(self):
        self.calls = []

    def add_images(self, tag, array, global_step=None, dataformats=None):
        self.calls.append((tag, array, global_step, dataformats))


def _kernel_launches(fn):
    from torch.profiler import ProfilerActivity, profile

    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "memcpy" not in e.name.lower()
               and "memset" not in e.name.lower())


def test_run_val_images_are_opt_in():
    from liso_amd.datasets.synthetic import detector_batch
    from liso_amd.eval.eval_ours import run_val
    from liso_amd.trainer import DetectorTrainer
    from liso_amd.utils.config import default_cfg

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    tr = DetectorTrainer(default_cfg(grid=64, bev_range_m=40.0), dev, total_steps=4)
    pcls, _ = detector_batch(3, 2, dev, n_points=4000, grid=64, bev_range_m=40.0)
    g = np.random.default_rng(21)
    gts = [scene(g, n, 0, 3, spread=18.0)[0] for n in (14, 9)]
    bms = [{k: v[: len(v) // 2] for k, v in gt.items()} for gt in gts]
    batch = dict(pcls=pcls, gt_boxes=pad_batch(gts).to("cuda"), benchmark_gt_boxes=pad_batch(bms).to("cuda"))
    tr.net.eval()
    names = ("car", "ped", "cyc")

    def run(**kw):
        return run_val(tr.cfg, [batch, batch], tr.net, "val/", movable_class_names=names, generator=torch.Generator(device=dev).manual_seed(5), **kw)

    plain = run()
    rec = _Recorder()
    with_images = run(image_writer=rec, num_image_steps=1)
    assert plain.keys() == with_images.keys()
    for k, v in plain.items():
        w = with_images[k]
        assert (v == w) or (v != v and w != w), k  # the metric dictionary is equal
    assert len(rec.calls) == 1  # the first batch only
    tag, img, step, fmt = rec.calls[0]
    assert tag == "val/RECONSTRUCTION_TARGETS_t0_t1" and step == 0 and fmt == "NHWC"
    assert img.is_cuda and img.dtype == torch.float32 and tuple(img.shape) == (2, 2 * 64, 64, 3)  # NMS to 100 over NMS to 40
    pic = img.cpu().numpy()
    assert np.isfinite(pic).all() and pic.min() >= 0.0 and pic.max() <= 1.0
    red = (pic[..., 0] == 1.0) & (pic[..., 1] == 0.0) & (pic[..., 2] == 0.0)
    assert red.sum() > 0, "the ground truth is drawn in red (where the predictions have not drawn over it)"
    assert ((pic[..., 2] > 0.39) & (pic[..., 2] < 0.41) & (pic[..., 1] >= 0.5)).sum() > 20, "predictions come in `summer` colours"

    # a batch that carries a second sweep gets the third canvas
    rec3 = _Recorder()
    two_sweeps = dict(batch, occupancy_f32_tb=torch.zeros((2, 1, 64, 64), device=dev), gt_boxes_tb=batch["gt_boxes"])
    run_val(tr.cfg, [two_sweeps], tr.net, "val/", movable_class_names=names, generator=torch.Generator(device=dev).manual_seed(5),
            image_writer=rec3, num_image_steps=1)
    assert tuple(rec3.calls[0][1].shape) == (2, 3 * 64, 64, 3)
    third = rec3.calls[0][1][:, 2 * 64:].cpu().numpy()
    assert (np.isclose(third[..., 2], 0.96) & np.isclose(third[..., 0], 0.13)).sum() > 0  # this sweep's ground truth in light blue, drawn last

    # without a writer a batch launches what it launched before; a writer that draws nothing adds nothing either
    n_plain = _kernel_launches(run)
    n_off = _kernel_launches(lambda: run(image_writer=_Recorder(), num_image_steps=0))
    n_on = _kernel_launches(lambda: run(image_writer=_Recorder(), num_image_steps=1))
    print(f"run_val kernel launches for two batches: {n_plain} without pictures, {n_on} with one batch's pictures")
    assert n_plain == n_off and n_on > n_plain
