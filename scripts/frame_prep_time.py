"""Times frame preparation (liso_amd/tracker/frame_prep.py) on the device: medians of device events after warm-up for the batched call,
eager and per captured replay, next to the per-frame path on the same data -- `is_boxes_clearly_in_bev_range`,
`drop_boxes_with_too_few_points`, `fit_bev_box_z_and_height_using_points_in_box` on the points inside the camera angle,
`mean_flow_per_box`, two `propagate_boxes_forward_using_flow` and the padding of `DeviceFlowBasedBoxTracker.run_tracker`'s inputs, all
functions the package had before the batched call -- which reads the host in every frame and is timed on the wall clock behind a
synchronisation.  The per-frame path does not align the boxes with their motion (the package had no mirror of that step), so it does
less than the batched call.  Workload: one sequence of 20 sweeps of 120 000 points, 100 boxes per frame, field-of-view cloud included.
Prints one JSON line.
    python scripts/frame_prep_time.py [--iters 20] [--per-frame-iters 3]
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

from liso_amd.kabsch.shape_utils import Shape, is_boxes_clearly_in_bev_range  # noqa: E402
from liso_amd.networks.flow_cluster_detector.flow_cluster_detector import fit_bev_box_z_and_height_using_points_in_box  # noqa: E402
from liso_amd.tracker.device_tracker import _pad_frames  # noqa: E402
from liso_amd.tracker.frame_prep import prepare_tracker_frames  # noqa: E402
from liso_amd.tracker.tracking import drop_boxes_with_too_few_points, mean_flow_per_box, propagate_boxes_forward_using_flow  # noqa: E402
from liso_amd.utils import graph_capture  # noqa: E402

T, N, P, MIN_POINTS = 20, 120_000, 100, 5
CFG = dict(bev_range_m=(120.0, 120.0), drop_boxes_on_bev_boundaries=True, min_points_in_box=MIN_POINTS, align_predicted_boxes_using_flow=True)


def workload():
    g = np.random.default_rng(0)
    clouds = np.concatenate([g.uniform(-60, 60, (T, N, 2)), g.uniform(-3, 2, (T, N, 1)), g.uniform(0, 255, (T, N, 1))], -1).astype(np.float32)
    counts = g.integers(N - 8000, N + 1, T).astype(np.int32)
    boxes = np.zeros((1, T, P, 7), np.float32)
    cell = np.stack(np.divmod(np.arange(P), 10), axis=1) * 11.0 - 50.0
    for t in range(T):
        clouds[t, counts[t]:] = np.nan
        boxes[0, t, :, :2], boxes[0, t, :, 2] = cell + g.uniform(-1.0, 1.0, (P, 2)), g.uniform(-1.2, -0.8, P)
        boxes[0, t, :, 3:6] = np.stack([g.uniform(3.5, 5.0, P), g.uniform(1.6, 2.2, P), g.uniform(1.4, 1.9, P)], axis=1)
        boxes[0, t, :, 6] = g.uniform(-np.pi, np.pi, P)
        at = g.choice(int(counts[t]), (P, 40), replace=False)  # 40 returns inside every box but each tenth, which gets none
        for i in range(P):
            if i % 10 != 9:
                clouds[t, at[i], :3] = boxes[0, t, i, :3] + g.uniform(-0.6, 0.6, (40, 3))
    flow = g.normal(0.0, 0.3, (T, N, 3)).astype(np.float32)
    valid = (g.uniform(size=(T, N)) > 0.1).astype(np.uint8)
    odom = np.tile(np.eye(4), (T, 1, 1))
    odom[:, 0, 3] = g.uniform(0.3, 0.6, T)
    return {"n_frames": np.array([T], np.int32), "n_box": np.full((1, T), P, np.int32), "boxes": boxes,
            "conf": g.uniform(0.3, 1.0, (1, T, P)).astype(np.float32), "odom": odom[None], "clouds": clouds[None], "counts": counts[None],
            "point_valid": valid[None], "flow": flow[None], "fov_clouds": clouds[None].copy(), "fov_counts": counts[None].copy()}


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
    return round(statistics.median(times), 4)


def wall_ms(fn, iters):
    fn()
    times = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - t))
    return round(statistics.median(times), 3)


def per_frame_path(dev, counts_host):
    """the stage as the package could run it before: one frame at a time -> the padded inputs of track_sequences and the FOV flags"""
    lo, hi = -41.95 / 180.0 * np.pi, 40.16 / 180.0 * np.pi
    bev = torch.tensor(CFG["bev_range_m"], device="cuda")
    kept_boxes, into_next, into_prev, in_fov = [], [], [], []
    for t in range(T):
        n = int(counts_host[t])
        b, pcl = dev["boxes"][0, t], dev["clouds"][0, t, :n]
        boxes = Shape(pos=b[:, :3], dims=b[:, 3:6], rot=b[:, 6:7], probs=dev["conf"][0, t, :, None])
        boxes.valid = is_boxes_clearly_in_bev_range(boxes, bev)
        boxes = drop_boxes_with_too_few_points(boxes.drop_padding_boxes(), pcl, MIN_POINTS)
        full = dev["fov_clouds"][0, t, :n]
        angles = torch.atan2(full[:, 1], full[:, 0])
        num, _, _ = fit_bev_box_z_and_height_using_points_in_box(full[(angles >= lo) & (angles <= hi)][:, :3], boxes)
        cloud, valid, flow = pcl[None, :, :3], dev["point_valid"][0, t, :n][None], dev["flow"][0, t, :n][None]
        mean, _ = mean_flow_per_box(boxes[None], cloud, valid, flow)
        st1 = propagate_boxes_forward_using_flow(boxes[None], cloud, valid, flow, dev["odom"][0, t], "cuda", mean_flow=mean)[4]
        st0 = propagate_boxes_forward_using_flow(boxes[None], cloud, valid, -1.0 * flow, torch.linalg.inv(dev["odom"][0, t]), "cuda", mean_flow=-mean)[4]
        kept_boxes.append(torch.cat([boxes.pos, boxes.dims, boxes.rot], dim=-1)), into_next.append(st1[0]), into_prev.append(st0[0])
        in_fov.append((num >= MIN_POINTS).to(torch.uint8))
    return (torch.tensor([len(k) for k in kept_boxes], dtype=torch.int32).cuda(), _pad_frames(kept_boxes, P), _pad_frames(into_prev, P),
            _pad_frames(into_next, P), _pad_frames(in_fov, P))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--per-frame-iters", type=int, default=3)
    args = ap.parse_args()
    arrays = workload()
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in arrays.items()}
    call = lambda: prepare_tracker_frames(*[dev[k] for k in arrays], cap=P, **CFG)  # noqa: E731
    frames = call()
    n_det, n_old, boxes_old, prev_old, next_old, fov_old = (frames.n_det[0].cpu().numpy(), *per_frame_path(dev, arrays["counts"][0]))
    assert n_det.tolist() == n_old.tolist(), "the two paths disagree on the boxes per frame"
    assert torch.equal(frames.boxes[0, ..., :6], boxes_old[..., :6]) and torch.equal(frames.in_fov[0], fov_old)
    assert float((frames.into_next[0] - next_old).abs().max()) < 1e-9 and float((frames.into_prev[0] - prev_old).abs().max()) < 1e-9
    result = {"workload": {"sweeps": T, "points": N, "boxes_per_frame": P, "kept": int(n_det.sum()), "in_fov": int(frames.in_fov.sum()),
                           "dropped_bev": int(frames.dropped_bev.sum()), "dropped_points": int(frames.dropped_points.sum())},
              "eager_device_ms": device_ms(call, args.iters), "eager_wall_ms": wall_ms(call, args.iters)}
    stream = torch.cuda.Stream()
    graph, _ = graph_capture.capture(call, stream, warm_ups=2)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        result["captured_replay_device_ms"] = device_ms(graph.replay, args.iters)
    result["per_frame_path"] = {"wall_ms": wall_ms(lambda: per_frame_path(dev, arrays["counts"][0]), args.per_frame_iters), "aligns": False}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
