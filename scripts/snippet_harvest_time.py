"""Times the snippet cut (liso_amd/tracker/snippet_harvest.py) on the device: medians of device events after warm-up for the eager
call (count-only pass, one read of the total, full pass), for the call with a given capacity (no host read) and for that call
replayed as a hipGraph, next to the numpy host path on the same inputs.  Workload: one sequence of 20 sweeps of 120 000 points,
15 tracks seen in every sweep = 300 jobs.  Prints one JSON line.
    python scripts/snippet_harvest_time.py [--iters 30] [--host-iters 2]
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

from liso_amd.tracker import snippet_harvest as H  # noqa: E402
from liso_amd.utils import graph_capture  # noqa: E402

T, N, TRACKS = 20, 120_000, 15


def workload():
    g = np.random.default_rng(0)
    clouds = np.concatenate([g.uniform(-60, 60, (T, N, 2)), g.uniform(-3, 2, (T, N, 1)), g.uniform(0, 255, (T, N, 1))], -1).astype(np.float32)
    counts = g.integers(N - 8000, N + 1, T).astype(np.int32)
    job_cloud, boxes = [], []
    for _ in range(TRACKS):
        x0, y0, yaw, speed = g.uniform(-40, 40), g.uniform(-40, 40), g.uniform(-np.pi, np.pi), g.uniform(0, 1.0)
        dims = [g.uniform(3.5, 5.0), g.uniform(1.6, 2.2), g.uniform(1.4, 1.9)]
        for t in range(T):
            x, y = x0 + speed * t * np.cos(yaw), y0 + speed * t * np.sin(yaw)
            local = g.uniform(-0.5, 0.5, (300, 3)) * dims  # 300 returns on the object
            at = g.choice(int(counts[t]), 300, replace=False)
            clouds[t, at, 0] = x + np.cos(yaw) * local[:, 0] - np.sin(yaw) * local[:, 1]
            clouds[t, at, 1] = y + np.sin(yaw) * local[:, 0] + np.cos(yaw) * local[:, 1]
            clouds[t, at, 2] = -0.9 + local[:, 2]
            job_cloud.append(t)
            boxes.append([x, y, -0.9, *dims, yaw])
    lidar_rows = g.integers(0, 64, (T, N)).astype(np.int32)
    return clouds, counts, lidar_rows, np.array(job_cloud, np.int32), np.array(boxes, np.float32)


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
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--host-iters", type=int, default=2)
    args = ap.parse_args()
    clouds, counts, lidar_rows, job_cloud, boxes = workload()
    times = []
    for _ in range(args.host_iters):
        t = time.perf_counter()
        want = H.cut_box_snippets_host(clouds, counts, lidar_rows, job_cloud, boxes)
        times.append(1e3 * (time.perf_counter() - t))
    total = int(want[0][-1])
    result = {"workload": {"sweeps": T, "points": N, "jobs": len(job_cloud), "snippet_points": total},
              "host_ms": round(statistics.median(times), 2), "device_ms": {}}
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    d = [to(a) for a in (clouds, counts, lidar_rows, job_cloud, boxes)]
    got = H.cut_box_snippets(*d)
    assert np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[2].cpu().numpy(), want[2]), "device and host path disagree"
    result["device_ms"]["eager_sized_by_count_pass"] = round(device_ms(lambda: H.cut_box_snippets(*d), args.iters), 4)
    result["device_ms"]["eager_given_capacity"] = round(device_ms(lambda: H.cut_box_snippets(*d, capacity=total), args.iters), 4)
    stream = torch.cuda.Stream()
    graph, _ = graph_capture.capture(lambda: H.cut_box_snippets(*d, capacity=total), stream, warm_ups=2)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        result["device_ms"]["given_capacity_captured"] = round(device_ms(graph.replay, args.iters), 4)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
