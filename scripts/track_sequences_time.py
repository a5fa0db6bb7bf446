"""Times the sequence tracker on one batch of sequences, the same inputs both ways:
  host   : per sequence the `update` loop (one copy of every frame's device tensors to the host, as the mining chain does today) plus
           `run_tracker` of `FlowBasedBoxTracker`, wall clock;
  device : `track_sequences` (liso_amd/tracker/device_tracker.py) on the padded batch, eager and replayed as a hipGraph, medians of
           device events after warm-up; the eager figure also as wall clock including the final synchronisation.
Workload: 32 sequences x 40 frames x 60 objects on a jittered lattice, each missed in a quarter of its frames (tests/tracker_scenes.py
builds them: this script borrows the test suite's scene generator and so runs from a checkout, tests/ included).  Prints one JSON
line.
    python scripts/track_sequences_time.py [--sequences 32] [--frames 40] [--boxes 60] [--iters 30] [--host-iters 2]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import tracker_scenes as TS  # noqa: E402
from liso_amd.kabsch.shape_utils import Shape  # noqa: E402
from liso_amd.tracker.device_tracker import needed_capacity, track_sequences  # noqa: E402
from liso_amd.tracker.global_box_tracker import FlowBasedBoxTracker  # noqa: E402
from liso_amd.utils import graph_capture  # noqa: E402


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


def host_pass(dev_frames):
    """every sequence through the host class, its frames coming from the device"""
    counters = []
    for frames in dev_frames:
        tr = FlowBasedBoxTracker(use_propagated_boxes=True, box_matching_threshold_m=TS.THRESHOLD, tie_order="stable")
        for boxes, into_next, into_prev, odom in frames:
            tr.update(boxes, into_next, into_prev, odom, [None] * boxes.valid.shape[0])
        tr.run_tracker()
        counters.append(int(tr.max_track_id_counter))
    return counters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sequences", type=int, default=32)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--boxes", type=int, default=60)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--host-iters", type=int, default=2)
    args = ap.parse_args()
    scenes = [TS.make_scene(TS.random_vis(args.frames, args.boxes, 100 + s), 100 + s) for s in range(args.sequences)]
    arrays = TS.batch(scenes)
    cap = max(needed_capacity(s["n_det"]) for s in scenes)
    d = {k: torch.from_numpy(v).cuda() for k, v in arrays.items()}
    dev_frames = []
    for s, sc in enumerate(scenes):
        frames = []
        for t in range(args.frames):
            n = int(sc["n_det"][t])
            b = d["boxes"][s, t, :n]
            frames.append((Shape(pos=b[:, :3], dims=b[:, 3:6], rot=b[:, 6:7], probs=d["conf"][s, t, :n, None],
                                 valid=torch.ones(n, dtype=torch.bool, device="cuda")),
                           d["into_next"][s, t, :n], d["into_prev"][s, t, :n], d["odom"][s, t]))
        dev_frames.append(frames)
    torch.cuda.synchronize()
    times = []
    for _ in range(args.host_iters):
        t0 = time.perf_counter()
        counters = host_pass(dev_frames)
        times.append(1e3 * (time.perf_counter() - t0))
    call = lambda: track_sequences(**d, threshold=TS.THRESHOLD, cap=cap)  # noqa: E731
    res = call()
    assert int(res.overflow.sum()) == 0 and res.id_counter.tolist() == counters, "device and host tracker disagree"
    result = {"workload": {"sequences": args.sequences, "frames": args.frames, "boxes": args.boxes, "cap": cap,
                           "detections": int(arrays["n_det"].sum())},
              "host_ms": round(statistics.median(times), 1), "device_ms": {"eager": round(device_ms(call, args.iters), 4)}}
    walls = []
    for _ in range(args.iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        walls.append(1e3 * (time.perf_counter() - t0))
    result["device_ms"]["eager_wall"] = round(statistics.median(walls), 4)
    stream = torch.cuda.Stream()
    graph, _ = graph_capture.capture(call, stream, warm_ups=2)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        result["device_ms"]["captured"] = round(device_ms(graph.replay, args.iters), 4)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
