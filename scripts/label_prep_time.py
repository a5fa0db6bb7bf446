"""Times the label preparation (liso_amd/datasets/label_prep.py) on the device: medians of device events after warm-up for each
entry and for `assemble_box_labels` captured in a hipGraph, next to the numpy host path.  Workload: two samples, 64 boxes each,
120 000 points, a 128 x 128 target grid, 100 m range.  Prints one JSON line.
    python scripts/label_prep_time.py [--iters 50] [--host-iters 3]
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

from liso_amd.datasets import label_prep as P  # noqa: E402
from liso_amd.kabsch.shape_utils import Shape  # noqa: E402
from liso_amd.utils import graph_capture  # noqa: E402

B, K, N, GRID, RANGE = 2, 64, 120_000, 128, 100.0


class _Cfg(dict):
    __getattr__ = dict.__getitem__


BOX_CFG = _Cfg(dimensions_representation=_Cfg(method="predict_abs_size"), rotation_representation=_Cfg(method="vector"),
               position_representation=_Cfg(method="local_relative_offset"), activations=_Cfg(dims="softplus"))
CFG = _Cfg(network=_Cfg(name="centerpoint"), data=_Cfg(bev_range_m=(RANGE, RANGE), img_grid_size=(4 * GRID, 4 * GRID)), box_prediction=BOX_CFG,
           loss=_Cfg(supervised=_Cfg(centermaps=_Cfg(active=True, confidence_target="gaussian"))))


def workload():
    g = np.random.default_rng(0)
    pos = np.concatenate([g.uniform(-55, 55, (B, K, 2)), g.uniform(-1.5, -0.5, (B, K, 1))], -1)
    dims = np.stack([g.uniform(3, 5, (B, K)), g.uniform(1.5, 2.2, (B, K)), g.uniform(1.4, 1.9, (B, K))], -1)
    boxes = Shape(pos=pos, dims=dims, rot=g.uniform(-np.pi, np.pi, (B, K, 1)), probs=np.ones((B, K, 1)), velo=g.uniform(-5, 5, (B, K, 1)),
                  valid=g.uniform(size=(B, K)) > 0.1)
    pcl = np.concatenate([g.uniform(-60, 60, (B, N, 2)), g.uniform(-3, 2, (B, N, 1)), g.uniform(0, 1, (B, N, 1))], -1).astype(np.float32)
    ignore = Shape(pos=np.concatenate([g.uniform(-40, 40, (B, 4, 2)), np.zeros((B, 4, 1))], -1), dims=g.uniform(4, 12, (B, 4, 3)),
                   rot=g.uniform(-1, 1, (B, 4, 1)), probs=np.ones((B, 4, 1)))
    counts = np.array([N, N - 7000], np.int32)
    odom = np.stack([np.eye(4)] * B)
    return boxes, pcl, counts, ignore, odom


def entries(boxes, pcl, counts, ignore, odom):
    rng = (RANGE, RANGE)
    poses = boxes.get_poses()
    has = P.filter_objects_to_bev_non_empty(boxes, pcl, counts, bev_range_m=rng)[1]
    ones = np.ones_like(boxes.probs) if isinstance(boxes.probs, np.ndarray) else torch.ones_like(boxes.probs)

    def chain():
        sample = {"pcl_full_no_ground_ta": pcl, "mined": {"objects_ta": boxes}, "gt": {"kitti_ignore_region_boxes_ta": ignore}}
        P.assemble_box_labels(sample, cfg=CFG, gt_boxes=boxes, counts=counts, centermaps_grid_size=(GRID, GRID))
        return sample

    return {
        "filter_with_points": lambda: P.filter_objects_to_bev_non_empty(boxes, pcl, counts, bev_range_m=rng, filter_bev=False, filter_range_m=50.0),
        "filter_reusing_flags": lambda: P.filter_objects_to_bev_non_empty(boxes, pcl, counts, bev_range_m=rng, box_has_points_inside=has),
        "object_velocity": lambda: P.object_velocity_in_obj_coords(odom, poses, poses),
        "ignore_region_mask": lambda: P.create_true_where_ignore_region_mask(ignore, (GRID, GRID), rng),
        "draw_heat_regression_maps": lambda: P.draw_heat_regression_maps(boxes, (GRID, GRID), rng, BOX_CFG, per_obj_prob_scale=ones),
        "assemble_box_labels": chain,
    }


def device_ms(fn, iters):
    for _ in range(5):
        fn()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--host-iters", type=int, default=3)
    args = ap.parse_args()
    boxes, pcl, counts, ignore, odom = workload()
    result = {"workload": {"B": B, "K": K, "N": N, "grid": GRID}, "host_ms": {}, "device_ms": {}}
    for name, fn in entries(boxes, pcl, counts, ignore, odom).items():
        times = []
        for _ in range(args.host_iters):
            t = time.perf_counter()
            fn()
            times.append(1e3 * (time.perf_counter() - t))
        result["host_ms"][name] = round(statistics.median(times), 3)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    dboxes, dignore = (Shape(**{k: to(v) for k, v in s.__dict__.items()}) for s in (boxes, ignore))
    dev = entries(dboxes, to(pcl), to(counts), dignore, to(odom))
    for name, fn in dev.items():
        result["device_ms"][name] = round(device_ms(fn, args.iters), 4)
    stream = torch.cuda.Stream()
    graph, _ = graph_capture.capture(dev["assemble_box_labels"], stream, warm_ups=2)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        result["device_ms"]["assemble_box_labels_captured"] = round(device_ms(graph.replay, args.iters), 4)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
