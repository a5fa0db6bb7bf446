"""Times track mining (liso_amd/tracker/track_mining.py) on the device: medians of device events after warm-up, per stage and for the
whole stage, eager and per captured replay, next to the existing per-track path on the same data -- `DeviceFlowBasedBoxTracker`'s
getters, `decide_keep_or_drop_box`, `perform_local_box_refinement`, the two `update_*` functions and a Python fold into a per-frame
dict -- which reads the host per track and is timed on the wall clock behind a synchronisation.  Workload: one sequence of 20 sweeps of
120 000 points with 15 objects seen in every sweep = 300 boxes (the shape of scripts/snippet_harvest_time.py), rectangle fit on.
Prints one JSON line.
    python scripts/track_mining_time.py [--iters 20] [--per-track-iters 3]
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
from liso_amd.tracker import track_mining as TM  # noqa: E402
from liso_amd.tracker.device_tracker import DeviceFlowBasedBoxTracker, track_sequences  # noqa: E402
from liso_amd.tracker.tracking import (decide_keep_or_drop_box, perform_local_box_refinement, update_sensor_boxes_from_world_boxes,  # noqa: E402
                                       update_world_boxes_from_sensor_boxes)
from liso_amd.utils import graph_capture  # noqa: E402
from liso_amd.utils.config import to_attr  # noqa: E402

T, N, TRACKS, DT, MAX_TRACKS = 20, 120_000, 15, 0.1, 16
CFG = dict(min_track_age=4, confidence_threshold_mined_boxes=0.3, min_track_obj_speed_mps=1.0, time_between_frames_s=DT,
           is_flow_cluster_detector=False, flow_cluster_detector_min_travel_dist_filter_m=3.0, fit_rot=True, fit_pos=True,
           fitting_dims_bloat_factor=1.2, min_dist_for_track_smoothing=5.0)


def compose(x, y, z, yaw):
    c, s, o, l = np.cos(yaw), np.sin(yaw), np.zeros_like(x), np.ones_like(x)
    return np.stack([np.stack([c, -s, o, x], -1), np.stack([s, c, o, y], -1), np.stack([o, o, l, z], -1), np.stack([o, o, o, l], -1)], -2)


def workload():
    g = np.random.default_rng(0)
    clouds = np.concatenate([g.uniform(-60, 60, (T, N, 2)), g.uniform(-3, 2, (T, N, 1)), g.uniform(0, 255, (T, N, 1))], -1).astype(np.float32)
    counts = g.integers(N - 8000, N + 1, T).astype(np.int32)
    for t in range(T):
        clouds[t, counts[t]:] = np.nan
    odom = compose(g.uniform(0.3, 0.6, T), g.uniform(-0.05, 0.05, T), np.zeros(T), g.uniform(-0.01, 0.01, T))
    W = [np.eye(4)]
    for t in range(T - 1):
        W.append(W[-1] @ odom[t])
    cell = np.stack(np.divmod(np.arange(TRACKS), 4), axis=1) * 22.0 - 33.0
    yaw, speed = g.uniform(-np.pi, np.pi, TRACKS), g.uniform(0.15, 0.45, TRACKS)
    dims = np.stack([g.uniform(3.5, 5.0, TRACKS), g.uniform(1.6, 2.2, TRACKS), g.uniform(1.4, 1.9, TRACKS)], axis=1)

    def poses(t_sensor, t_obj):
        at = cell + (speed * t_obj)[:, None] * np.stack([np.cos(yaw), np.sin(yaw)], axis=1)
        return np.linalg.inv(W[t_sensor]) @ compose(at[:, 0], at[:, 1], np.full(TRACKS, -0.9), yaw)

    boxes, into_prev, into_next = np.zeros((1, T, TRACKS, 7), np.float32), np.zeros((1, T, TRACKS, 4, 4)), np.zeros((1, T, TRACKS, 4, 4))
    for t in range(T):
        own = poses(t, t)
        boxes[0, t] = np.concatenate([own[:, :3, 3], dims * g.uniform(0.9, 1.0, (TRACKS, 3)), np.arctan2(own[:, 1, 0], own[:, 0, 0])[:, None] + 0.05], axis=1)
        into_prev[0, t], into_next[0, t] = poses(max(t - 1, 0), t - 1), poses(min(t + 1, T - 1), t + 1)
        for i in range(TRACKS):  # 300 returns on two edges of the object
            u = g.uniform(-0.5, 0.5, 300)
            edge = np.where(np.arange(300)[:, None] < 180, np.stack([u, np.full(300, -0.5)], 1), np.stack([np.full(300, 0.5), u], 1)) * dims[i, :2]
            at = g.choice(int(counts[t]), 300, replace=False)
            clouds[t, at, :2] = (np.concatenate([edge, np.zeros((300, 1)), np.ones((300, 1))], axis=1) @ own[i].T)[:, :2]
    conf = g.uniform(0.4, 1.0, (1, T, TRACKS)).astype(np.float32)
    return {"n_frames": np.array([T], np.int32), "n_det": np.full((1, T), TRACKS, np.int32), "boxes": boxes, "conf": conf, "odom": odom[None],
            "into_prev": into_prev, "into_next": into_next}, clouds[None], counts[None]


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


def per_track_path(tracker, clouds, counts):
    """the stage as the package could run it before: one track at a time from the tracker's getters -> {frame: [sensor boxes]}"""
    ref_cfg = to_attr({"data": {"tracking_cfg": {"fit_box_to_points": {"fit_rot": True, "fit_pos": True, "fitting_dims_bloat_factor": 1.2},
                                                 "flow_cluster_detector_min_travel_dist_filter_m": 3.0}}})
    tracker._host = None  # (the getters read the host again)
    ids, ages = tracker.get_ids_lengths_of_longest_tracks()
    world, sensor = tracker.get_boxes_in_world_coordinates(), tracker.get_boxes_in_sensor_coordinates_at_each_timestamp()
    w_T, sweeps = tracker.w_Ts_sti, [clouds[0, t, :int(counts[0, t])] for t in range(T)]
    db, launches = {}, 0
    for track_id, age in zip(ids.tolist(), ages.tolist()):
        if age < CFG["min_track_age"]:
            continue
        box_idxs, start = tracker.get_box_indices_start_time_for_track_id(track_id)
        box_idxs, start = box_idxs.tolist(), int(start)
        wseq = Shape.from_list_of_shapes([world[start + k][i] for k, i in enumerate(box_idxs)])
        if torch.median(wseq.probs) < CFG["confidence_threshold_mined_boxes"]:
            continue
        keep, dist = decide_keep_or_drop_box(tracking_cfg=ref_cfg.data.tracking_cfg, box_sequence_world_for_specific_track_id=wseq,
                                             min_track_obj_speed_mps=CFG["min_track_obj_speed_mps"], track_id=track_id, time_between_frames_s=DT,
                                             verbose=False, is_flow_cluster_detector=False)
        if not keep:
            continue
        sseq = Shape.from_list_of_shapes([sensor[start + k][i] for k, i in enumerate(box_idxs)])
        sseq = perform_local_box_refinement(ref_cfg, None, sweeps, sseq, age, start)
        launches += age
        wseq = update_world_boxes_from_sensor_boxes(box_sequence_sensor=sseq, box_sequence_world=wseq, w_T_sensor_ti=w_T[start:start + age])
        wseq.probs = torch.median(wseq.probs, dim=0).values * torch.ones_like(wseq.probs)
        wseq.velo = torch.ones_like(wseq.probs) * dist / (age * DT)
        sseq = update_sensor_boxes_from_world_boxes(box_sequence_world=wseq, box_sequence_sensor=sseq, w_T_sensor_ti=w_T[start:start + age])
        for k in range(age):
            db.setdefault(start + k, []).append((track_id, sseq[k]))
    return db, launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--per-track-iters", type=int, default=3)
    args = ap.parse_args()
    arrays, clouds, counts = workload()
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in arrays.items()}
    clouds, counts = torch.from_numpy(clouds).cuda(), torch.from_numpy(counts).cuda()
    tracked = track_sequences(**dev, threshold=2.0, cap=3 * TRACKS)
    select_args = {k: v for k, v in CFG.items() if not k.startswith("fit")}
    refine_args = dict(fit_rot=True, fit_pos=True, fitting_dims_bloat_factor=1.2, time_between_frames_s=DT)

    def whole(method, use=True):
        return TM.mine_tracked_sequences(tracked, dev["boxes"], dev["conf"], clouds, counts, max_tracks=MAX_TRACKS, cap_out=MAX_TRACKS,
                                         use_track_smoothing=use, track_smoothing_method=method, **CFG)

    mined = whole("jerk")
    verdict = mined.verdict.cpu().numpy()
    result = {"workload": {"sweeps": T, "points": N, "boxes": T * TRACKS, "tracks": int(mined.n_tracks[0]), "kept": int(((verdict & TM.KEPT) != 0).sum()),
                           "smoothed": int(((verdict & TM.SMOOTHED) != 0).sum()), "exported_rows": int(mined.frames.n_boxes.sum())}}
    sel = TM.select_tracks(tracked, dev["boxes"], dev["conf"], max_tracks=MAX_TRACKS, **select_args)
    ref = TM.refine_tracks(sel, tracked, clouds, counts, **refine_args)
    eager = {"select": device_ms(lambda: TM.select_tracks(tracked, dev["boxes"], dev["conf"], max_tracks=MAX_TRACKS, **select_args), args.iters),
             "refine": device_ms(lambda: TM.refine_tracks(sel, tracked, clouds, counts, **refine_args), args.iters),
             "smooth_jerk": device_ms(lambda: TM.smooth_tracks(sel, ref, track_smoothing_method="jerk", time_between_frames_s=DT), args.iters),
             "export": device_ms(lambda: TM.export_tracks(sel, ref, tracked, cap_out=MAX_TRACKS), args.iters),
             "whole_without_smoothing": device_ms(lambda: whole("none", False), args.iters), "whole_jerk": device_ms(lambda: whole("jerk"), args.iters)}
    result["eager_device_ms"] = eager
    result["eager_wall_ms"] = {"whole_without_smoothing": wall_ms(lambda: whole("none", False), args.iters)}
    captured = {}
    for name, fn in (("whole_without_smoothing", lambda: whole("none", False)), ("whole_jerk", lambda: whole("jerk"))):
        stream = torch.cuda.Stream()
        graph, _ = graph_capture.capture(fn, stream, warm_ups=2)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            captured[name] = device_ms(graph.replay, args.iters)
    result["captured_replay_device_ms"] = captured
    # the per-track path on the same data (no smoothing: compare with whole_without_smoothing)
    tracker = DeviceFlowBasedBoxTracker(use_propagated_boxes=True, box_matching_threshold_m=2.0)
    for t in range(T):
        b = dev["boxes"][0, t]
        tracker.update(Shape(pos=b[:, :3].clone(), dims=b[:, 3:6].clone(), rot=b[:, 6:7].clone(), probs=dev["conf"][0, t, :, None].clone(),
                             valid=torch.ones(TRACKS, dtype=torch.bool, device="cuda")), dev["into_next"][0, t], dev["into_prev"][0, t], dev["odom"][0, t])
    tracker.run_tracker()
    db, launches = per_track_path(tracker, clouds, counts)
    plain = whole("none", False)
    n_boxes = plain.frames.n_boxes[0].cpu().numpy()
    assert [len(db.get(t, [])) for t in range(T)] == n_boxes.tolist(), "the two paths disagree on the boxes per frame"
    # torch.quantile interpolates with fp32 rank arithmetic, the kernel with the fp64 fraction: the refined dims may differ in the last
    # fp32 bit, and a resized box's position then by that relative amount of its distance to the corner that stays in place
    worst = 0.0
    for t in range(T):
        assert plain.frames.track_id[0, t, :len(db[t])].tolist() == [track_id for track_id, _ in db[t]], t
        worst = max([worst] + [float((plain.frames.pos[0, t, i] - box.pos).abs().max()) for i, (_, box) in enumerate(db[t])])
    assert worst < 1e-5, worst
    result["per_track_path"] = {"wall_ms": wall_ms(lambda: per_track_path(tracker, clouds, counts), args.per_track_iters), "fit_launches": launches,
                                "batched_fit_launches": T, "max_abs_position_difference_m": worst}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
