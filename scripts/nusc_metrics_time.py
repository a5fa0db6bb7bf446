"""Times the nuScenes detection metrics of the validation pass (liso_amd/eval/nuscenes_metrics.py) on scripts/det_val_time.py's
workload: 64 frames, about 31 ground-truth boxes and about 99 post-NMS predictions per frame.
  * the device time of the one launch, liso_det_val_nusc_f32, alone (events around it, median), as one class and per class;
  * the validation pass end to end, `compute()` included, with the flag off and on (run_val's KITTI collections, then the same plus the
    as-one nuScenes collection), and a validator of the nuScenes collection alone;
  * the kernel launches per batch of the flag-on pass over the flag-off pass, counted with torch.profiler.
Prints one JSON line.
    python scripts/nusc_metrics_time.py [--iters 5] [--launch-iters 50]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
sys.path.insert(0, os.path.abspath(os.path.dirname(__file__)))

from det_val_time import CLASSES, F, event_ms, frame, kernel_launches  # noqa: E402

from liso_amd.eval.det_validation import Collection, DetectionValidator, pack_boxes  # noqa: E402
from liso_amd.eval.nuscenes_metrics import NuscenesObjectDetectionMetrics, nusc_match_packed  # noqa: E402
from liso_amd.kabsch.shape_utils import Shape  # noqa: E402

PER_CLASS = ("car", "pedestrian", "bicycle")


def validator(flag):
    return DetectionValidator.for_run_val("kitti", CLASSES, (0, 1, 2), moving_velocity_thresh=0.1, nuscenes_metrics=flag)


def launch_ms(gt, pred, as_one, iters):
    from liso_amd import det_nms as D

    m = NuscenesObjectDetectionMetrics(as_one, class_names=None if as_one else PER_CLASS)
    g, p = pack_boxes(gt), pack_boxes(pred)
    order = D.order(p["score"], None, p["valid"], None)[1]
    radius = m.radius_on(order.device)
    run = lambda: nusc_match_packed(g, p, order, radius, as_one)  # noqa: E731
    out = run()
    return event_ms(run, iters)[0], int(out["count"].sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--launch-iters", type=int, default=50)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = np.random.default_rng(0)
    frames = [frame(g) for _ in range(F)]
    gt, bm, pred = (Shape.from_list_of_shapes([s[i] for s in frames]).to(dev) for i in range(3))
    draws = torch.from_numpy(g.integers(0, 3, tuple(pred.valid.shape)).astype(np.int32)).to(dev)

    def full(flag):
        v = validator(flag)
        v.update_batch(gt, bm, pred, class_draws=draws)
        return v.compute("val/")

    def alone():
        v = DetectionValidator([Collection("final_result/NUSC_OFFICIAL/detection_metrics/", "gt", {}, "nusc")])
        v.update_batch(gt, None, pred)
        return v.compute("val/")

    def device_part(flag):
        validator(flag).update_batch(gt, bm, pred, class_draws=draws)
    full(True), alone()  # warm-up: library load, tables on the device
    one_ms, one_matches = launch_ms(gt, pred, True, args.launch_iters)
    cls_ms, cls_matches = launch_ms(gt, pred, False, args.launch_iters)
    off_ms, off = event_ms(lambda: full(False), args.iters)
    on_ms, on = event_ms(lambda: full(True), args.iters)
    alone_ms, res = event_ms(alone, args.iters)
    n_off, why = kernel_launches(lambda: device_part(False))
    n_on, why2 = kernel_launches(lambda: device_part(True))
    same = lambda a, b: (np.isnan(a) and np.isnan(b)) or a == b  # noqa: E731
    print(json.dumps({
        "frames": F, "gt_per_frame": round(float(gt.valid.sum()) / F, 1), "pred_per_frame": round(float(pred.valid.sum()) / F, 1),
        "nusc_launch_ms_as_one": round(one_ms, 4), "nusc_launch_ms_per_class": round(cls_ms, 4), "cells": F * 4,
        "matches_as_one": one_matches, "matches_per_class": cls_matches,
        "validator_flag_off_ms": round(off_ms, 2), "validator_flag_on_ms": round(on_ms, 2), "nusc_collection_alone_ms": round(alone_ms, 2),
        "launches_per_batch_flag_off": n_off, "launches_per_batch_flag_on": n_on, "launch_count_note": why or why2,
        "other_results_unchanged": all(same(on[k], w) for k, w in off.items()), "nusc_keys": len(set(on) - set(off)),
        "mAP": round(res["val/final_result/NUSC_OFFICIAL/detection_metrics/mAP"], 4),
        "NDS": round(res["val/final_result/NUSC_OFFICIAL/detection_metrics/NDS"], 4)}))


if __name__ == "__main__":
    main()
