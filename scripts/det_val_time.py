"""Times the detector's validation matching end to end, the final `compute()` included, on one validation set through two paths:
`DetectionValidator` (liso_amd/eval/det_validation.py: all frames and all metric collections matched in at most three launches per
ground-truth set, one host read) and the per-frame `ObjectDetectionMetrics.update` loop the package had before it (class transfer by
`slow_greedy_match_boxes_by_desending_confidence_by_dist`, then every collection's update), on the same data and the same class draws.
Workload: 64 frames, about 30 ground-truth boxes and about 100 post-NMS predictions per frame, run_val's KITTI collections (visible /
benchmark / waymo_cropped x 4 range bins x 2 criteria x 4 thresholds + 3 classes x 4 thresholds = 108 matchings per frame).
Device events around synchronised work; the kernel launches per frame of each path are counted with torch.profiler.
Prints one JSON line.
    python scripts/det_val_time.py [--iters 5] [--per-frame-iters 1]
--waymo times the Waymo-style L1 / L2 collections instead (run_val(..., waymo_metrics=True): four range bins on the benchmark ground
truth, matched by optimal assignment in one more launch): the validation pass with the flag off and on in the same run, the per-frame
`WaymoObjectDetectionMetrics.update` loop over the same frames (host scipy assignment), and the assignment launch's own device time.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

from liso_amd.eval.det_validation import DetectionValidator  # noqa: E402
from liso_amd.kabsch.box_groundtruth_matching import slow_greedy_match_boxes_by_desending_confidence_by_dist  # noqa: E402
from liso_amd.kabsch.shape_utils import Shape  # noqa: E402

F, N_GT, N_PRED, CLASSES = 64, 30, 100, ("car", "pedestrian", "cyclist")


def boxes(g, n):
    pos = np.concatenate([g.uniform(-55, 55, (n, 2)), g.uniform(-1.6, -0.4, (n, 1))], -1)
    dims = np.stack([g.uniform(2, 6, n), g.uniform(1, 2.5, n), g.uniform(1.2, 2.2, n)], -1)
    return pos, dims, g.uniform(-np.pi, np.pi, (n, 1))


def frame(g):
    """about N_GT ground-truth boxes, about N_PRED predictions (60 % of them jittered copies of ground-truth boxes, at most one per box)"""
    n_gt, n_pred = int(g.integers(N_GT - 8, N_GT + 9)), int(g.integers(N_PRED - 15, N_PRED + 16))
    (gp, gd, gr), (pp, pd, pr) = boxes(g, n_gt), boxes(g, n_pred)
    k = min(n_gt, int(0.6 * n_pred))
    sel = g.permutation(n_gt)[:k]
    pp[:k], pd[:k], pr[:k] = gp[sel] + g.normal(0, 0.25, (k, 3)), gd[sel] * g.uniform(0.85, 1.15, (k, 3)), gr[sel] + g.normal(0, 0.15, (k, 1))
    t = lambda a: torch.from_numpy(a.astype(np.float32))  # noqa: E731
    gt = Shape(pos=t(gp), dims=t(gd), rot=t(gr), probs=torch.ones(n_gt, 1), velo=t(g.uniform(0, 2.0, (n_gt, 1)) * (g.uniform(size=(n_gt, 1)) < 0.5)),
               class_id=torch.from_numpy(g.integers(0, 3, (n_gt, 1))), valid=torch.ones(n_gt, dtype=torch.bool))
    pred = Shape(pos=t(pp), dims=t(pd), rot=t(pr), probs=t(g.uniform(0.05, 1.0, (n_pred, 1))), velo=torch.zeros(n_pred, 1),
                 class_id=torch.from_numpy(g.integers(0, 3, (n_pred, 1))), valid=torch.ones(n_pred, dtype=torch.bool))
    return gt, gt[torch.from_numpy(g.uniform(size=n_gt) < 0.7)], pred


def new_validator(waymo=False):
    return DetectionValidator.for_run_val("kitti", CLASSES, (0, 1, 2), moving_velocity_thresh=0.1, waymo_metrics=waymo)


def batched_path(gt, bm, pred, draws, waymo=False):
    v = new_validator(waymo)
    v.update_batch(gt, bm, pred, class_draws=draws)
    return v.compute("val/")


def per_frame_path(gts, bms, preds, draws, frames=None):
    v = new_validator()
    for f in range(len(gts) if frames is None else frames):
        gt, pred = gts[f], preds[f].clone()
        idx_gt, idx_pred, _, _, _ = slow_greedy_match_boxes_by_desending_confidence_by_dist(
            gt.pos, pred.pos, non_batched_pred_confidence=torch.squeeze(pred.probs, dim=-1), matching_threshold=3.0, match_in_nd=2)
        pred.class_id = draws[f, : pred.valid.shape[0], None].to(pred.class_id.dtype)
        pred.class_id[torch.from_numpy(idx_pred).to(pred.pos.device)] = gt.class_id[torch.from_numpy(idx_gt).to(pred.pos.device)]
        for c, m in zip(v.collections, v.metrics):
            m.update(non_batched_gt_boxes=bms[f] if c.gt_set == "benchmark" else gt, non_batched_pred_boxes=pred)
    out = {}
    for c, m in zip(v.collections, v.metrics):
        out.update(m.compute("val/" + c.tag))
    return out


def waymo_per_frame_path(bms, preds):
    """the reference's way: every frame through every range bin's `update` (the overall class: no class transfer needed)"""
    from liso_amd.eval.det_validation import RANGE_BINS
    from liso_amd.eval.od_metrics import WaymoObjectDetectionMetrics

    ms = {f"val/final_result/WAYMO/detection_metrics/{int(lo)}_{int(hi)}m": WaymoObjectDetectionMetrics(min_eval_range_m=lo, max_eval_range_m=hi)
          for lo, hi in RANGE_BINS}
    for bm, pred in zip(bms, preds):
        for m in ms.values():
            m.update(non_batched_gt_boxes=bm, non_batched_pred_boxes=pred)
    out = {}
    for tag, m in ms.items():
        out.update(m.compute(tag))
    return out


def assign_launch_ms(bm, pred, iters=20):
    """device time of liso_det_val_assign_f32 alone on the benchmark set's jobs (events around the one launch, median)"""
    from liso_amd import _lib as L
    from liso_amd.eval.det_validation import JobTable, match_detections_packed, pack_boxes
    from liso_amd.utils.device_args import opt_ptr as _p

    at = new_validator(True).assign_tables["benchmark"]
    g, p = pack_boxes(bm), pack_boxes(pred)
    o = match_detections_packed(g, p, JobTable(), assign=at)
    ft, jt = at.device_tables(g["rows"].device)
    F, G = g["valid"].shape
    P = p["valid"].shape[1]

    def launch():
        L.check(L.lib().liso_det_val_assign_f32(F, G, P, _p(g["rows"]), _p(g["valid"]), _p(g["cls"]), _p(p["rows"]), _p(p["valid"]), _p(o["pred_class"]),
                                                _p(o["iou_bev"]), _p(o["iou_3d"]), at.criteria_mask, L.ptr(ft), len(at.filters), L.ptr(jt), len(at.jobs),
                                                _p(o["assign_count"]), _p(o["assign_pairs"]), _p(o["assign_gt_in"]), _p(o["assign_pred_in"]),
                                                L.stream_ptr()), "det_val assign")
    launch()
    return event_ms(launch, iters)[0], F * len(at.jobs)


def waymo_leg(args, gts, bms, preds, gt, bm, pred, draws):
    batched_path(gt, bm, pred, draws, True)  # warm-up
    waymo_per_frame_path(bms[:2], preds[:2])
    off_ms, off = event_ms(lambda: batched_path(gt, bm, pred, draws), args.iters)
    on_ms, on = event_ms(lambda: batched_path(gt, bm, pred, draws, True), args.iters)
    loop_ms, ref = event_ms(lambda: waymo_per_frame_path(bms, preds), args.per_frame_iters)
    a_ms, cells = assign_launch_ms(bm, pred)
    same = lambda a, b: (np.isnan(a) and np.isnan(b)) or a == b  # noqa: E731
    worst = max((abs(on[k] - w) for k, w in ref.items() if "AP@" in k and not (np.isnan(on[k]) and np.isnan(w))), default=0.0)
    print(json.dumps({
        "frames": F, "benchmark_gt_per_frame": round(float(bm.valid.sum()) / F, 1), "pred_per_frame": round(float(pred.valid.sum()) / F, 1),
        "validator_flag_off_ms": round(off_ms, 2), "validator_flag_on_ms": round(on_ms, 2), "waymo_per_frame_loop_ms": round(loop_ms, 1),
        "flag_on_not_slower_than_off_plus_loop": on_ms <= off_ms + loop_ms, "assign_launch_ms": round(a_ms, 4), "assign_cells": cells,
        "greedy_results_unchanged": all(same(on[k], w) for k, w in off.items()), "waymo_keys": len(ref),
        "waymo_keys_equal_per_frame_loop": set(ref) == set(on) - set(off), "max_abs_waymo_ap_difference": worst}))


def event_ms(fn, iters):
    times = []
    for _ in range(iters):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times), out


def kernel_launches(fn):
    """device kernels launched by fn(), all libraries, counted by torch.profiler; None (and why) where the profiler gives no device events"""
    try:
        from torch.profiler import ProfilerActivity, profile

        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "memcpy" not in e.name.lower()
                and "memset" not in e.name.lower())
        return (n or None), (None if n else "no device events recorded")
    except Exception as e:  # noqa: BLE001
        return None, repr(e)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--per-frame-iters", type=int, default=1)
    ap.add_argument("--waymo", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = np.random.default_rng(0)
    frames = [frame(g) for _ in range(F)]
    gts, bms, preds = ([s[i].to(dev) for s in frames] for i in range(3))
    gt, bm, pred = (Shape.from_list_of_shapes([s[i] for s in frames]).to(dev) for i in range(3))
    draws = torch.from_numpy(g.integers(0, 3, tuple(pred.valid.shape)).astype(np.int32)).to(dev)
    if args.waymo:
        gd = np.random.default_rng(1)  # Waymo difficulty levels, 0 and > 0 mixed (a generator of its own: the boxes above stay the same)
        for s in frames:
            for b in s[:2]:
                b.difficulty = torch.from_numpy((gd.integers(0, 3, (b.valid.shape[0], 1)) * (gd.uniform(size=(b.valid.shape[0], 1)) < 0.6)).astype(np.int32))
        gts, bms = ([s[i].clone().to(dev) for s in frames] for i in range(2))
        gt, bm = (Shape.from_list_of_shapes([s[i] for s in frames]).to(dev) for i in range(2))
        return waymo_leg(args, gts, bms, preds, gt, bm, pred, draws)
    batched_path(gt, bm, pred, draws)  # warm-up: library load, job tables on the device
    per_frame_path(gts, bms, preds, draws, frames=2)
    b_ms, b_out = event_ms(lambda: batched_path(gt, bm, pred, draws), args.iters)
    p_ms, p_out = event_ms(lambda: per_frame_path(gts, bms, preds, draws), args.per_frame_iters)
    ap_keys = [k for k in b_out if "AP@" in k]
    worst = max((abs(b_out[k] - p_out[k]) for k in ap_keys if not (np.isnan(b_out[k]) and np.isnan(p_out[k]))), default=0.0)

    def device_part():
        v = new_validator()
        v.update_batch(gt, bm, pred, class_draws=draws)
    d_ms, _ = event_ms(device_part, args.iters)
    b_n, b_why = kernel_launches(device_part)
    p_n, p_why = kernel_launches(lambda: per_frame_path(gts, bms, preds, draws, frames=4))
    print(json.dumps({
        "frames": F, "gt_per_frame": round(float(gt.valid.sum()) / F, 1), "pred_per_frame": round(float(pred.valid.sum()) / F, 1),
        "matchings_per_frame": sum(len(t.jobs) for t in new_validator().tables.values()),
        "validator_ms": round(b_ms, 2), "validator_device_part_ms": round(d_ms, 3), "per_frame_path_ms": round(p_ms, 1),
        "speedup": round(p_ms / b_ms, 1), "validator_launches_per_frame": None if b_n is None else round(b_n / F, 2),
        "per_frame_path_launches_per_frame": None if p_n is None else round(p_n / 4, 1), "launch_count_note": b_why or p_why,
        "ap_values": len(ap_keys), "max_abs_ap_difference": worst}))


if __name__ == "__main__":
    main()
