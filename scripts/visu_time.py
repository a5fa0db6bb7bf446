"""Times the summary pictures (liso_amd/visu) on the device: per picture the median of device events eager, the time per replay of
the picture captured in a hipGraph, the numpy host path on the same data and the kernel launches counted with torch.profiler.
Workload: two samples, 512 x 512 canvases over 100 m, 100 predicted and 30 ground-truth boxes per image, 120 000-point clouds.
Prints one JSON line.
    python scripts/visu_time.py [--iters 30] [--host-iters 2]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

from liso_amd.kabsch.shape_utils import Shape  # noqa: E402
from liso_amd.utils import graph_capture  # noqa: E402
from liso_amd.utils.config import to_attr  # noqa: E402
from liso_amd.visu import bbox_image as BI, flow_image as FI, pcl_image as PI  # noqa: E402

B, GRID, RANGE, N_PRED, N_GT, N = 2, 512, 100.0, 100, 30, 120_000
CFG = to_attr({"logging": {"max_log_img_batches": 4}, "data": {"bev_range_m": (RANGE, RANGE)}, "nms_iou_threshold": 0.1})


class _Sink:
    def add_images(self, *a, **k):
        pass


def boxes(g, K):
    pos = np.concatenate([g.uniform(-48, 48, (B, K, 2)), g.uniform(-1.5, -0.5, (B, K, 1))], -1).astype(np.float32)
    dims = np.stack([g.uniform(3, 5, (B, K)), g.uniform(1.5, 2.2, (B, K)), g.uniform(1.4, 1.9, (B, K))], -1).astype(np.float32)
    return Shape(pos=pos, dims=dims, rot=g.uniform(-np.pi, np.pi, (B, K, 1)).astype(np.float32), probs=g.random((B, K, 1)).astype(np.float32),
                 valid=g.random((B, K)) > 0.05)


def workload():
    g = np.random.default_rng(0)
    pcl = np.concatenate([g.uniform(-55, 55, (B, N, 2)), g.uniform(-3, 2, (B, N, 1)), g.uniform(0, 1, (B, N, 1))], -1).astype(np.float32)
    return {"pred": boxes(g, N_PRED), "gt": boxes(g, N_GT), "bg": boxes(g, 10), "pcl": pcl, "flow": g.normal(size=(B, 2, GRID, GRID)).astype(np.float32),
            "gray": (g.random((B, 1, GRID, GRID)) < 0.05).astype(np.float32)}


def to_device(w, dev):
    return {k: (v.to_tensor().to(dev) if isinstance(v, Shape) else torch.from_numpy(v).to(dev)) for k, v in w.items()}


def pictures(w, nms_on_host_input=None):
    """name -> callable; `nms_on_host_input`: the survivors the host path draws in place of running the NMS"""
    lo = np.array([-RANGE / 2, -RANGE / 2], np.float32)
    if not isinstance(w["pcl"], np.ndarray):
        lo = torch.from_numpy(lo).to(w["pcl"].device)
    hi = -lo
    a = {"occupancy_f32_ta": w["gray"], "gt": {"boxes": w["gt"]}}
    host = nms_on_host_input is not None

    def movement():
        if not host:
            return BI.log_box_movement(cfg=CFG, writer=_Sink(), global_step=0, sample_data_a=a, sample_data_b=a, pred_boxes=w["pred"],
                                       gt_background_boxes=w["bg"])
        imgs = [BI.draw_box_image(cfg=CFG, pred_boxes=p, gt_boxes=w["gt"], canvas_f32=w["gray"], gt_background_boxes=w["bg"]) for p in nms_on_host_input]
        imgs.append(BI.draw_box_image(cfg=CFG, pred_boxes=None, gt_boxes=w["gt"], canvas_f32=w["gray"], gt_background_boxes=w["bg"], gt_boxes_prev=w["gt"]))
        return np.concatenate(imgs, axis=1)

    return {
        "flow_wheel": lambda: FI.pytorch_create_flow_image(w["flow"]),
        "topdown_image": lambda: PI.create_topdown_f32_pcl_image_variable_extent(w["pcl"], w["pcl"][..., 3], lo, hi, (GRID, GRID)),
        "occupancy_image": lambda: PI.create_occupancy_pcl_image(w["pred"].pos, np.array([RANGE, RANGE]), (GRID, GRID), w["pred"].valid),
        "draw_box_image": lambda: BI.draw_box_image(cfg=CFG, pred_boxes=w["pred"], gt_boxes=w["gt"], canvas_f32=w["gray"], gt_background_boxes=w["bg"]),
        "log_box_movement_3_canvases": movement,
    }


def event_ms(fn, iters):
    times = []
    for _ in range(iters):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def kernel_launches(fn):
    from torch.profiler import ProfilerActivity, profile

    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "memcpy" not in e.name.lower()
               and "memset" not in e.name.lower())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--host-iters", type=int, default=2)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    w = workload()
    d = to_device(w, dev)
    # the host path has no NMS: it draws the device's survivors
    from liso_amd.utils.nms_iou import perform_nms_on_shapes_padded

    clamped = d["pred"].clone()
    clamped.dims = torch.clamp(clamped.dims, min=0.3, max=15.0)
    survivors = [perform_nms_on_shapes_padded(clamped, max_num_boxes=k, overlap_threshold=0.1, pre_nms_max_num_boxes=1000).numpy() for k in (100, 40)]
    out = {"workload": {"batch": B, "canvas": GRID, "pred_boxes": N_PRED, "gt_boxes": N_GT, "points": N}, "pictures": {}}
    host = pictures(w, survivors)
    stream = torch.cuda.Stream(dev)
    for name, fn in pictures(d).items():
        for _ in range(3):
            fn()
        row = {"eager_ms": round(event_ms(fn, args.iters), 4), "launches": kernel_launches(fn)}
        graph, _ = graph_capture.capture(fn, stream, warm_ups=2)
        torch.cuda.synchronize()
        row["graph_replay_ms"] = round(event_ms(graph.replay, args.iters), 4)
        t = []
        for _ in range(args.host_iters):
            t0 = time.perf_counter()
            host[name]()
            t.append(1e3 * (time.perf_counter() - t0))
        row["host_numpy_ms"] = round(statistics.median(t), 2)
        out["pictures"][name] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
