"""Times the lidar odometry (liso_amd/odometry) on the device: 20 sweeps of 120 000 rays (64 rings x 1875 azimuths) of the
world-fixed scene of tests/odometry_scenes.py, spread threefold (a hall of 130 m x 70 m), with KISSConfig's defaults (max_range 100 m,
voxels of 1 m), for S = 1 and for S = 16 sequences (four trajectories, each four times).  Reports, per S: the eager call and a captured
replay (medians of device events after warm-up), the three stages summed over the frames (device events around the stage calls of
`OdometryWorkspace`), and what the ICP's cost rests on -- the mean source size and the mean iteration count; and the host
restatement's wall time on the first sweeps of one sequence.  Prints one JSON line.
    python scripts/odometry_time.py [--iters 3] [--host-frames 4] [--sequences 1,16]
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

import odometry_scenes as SC  # noqa: E402
from liso_amd.odometry import OdometryWorkspace, lidar_odometry, lidar_odometry_host  # noqa: E402
from liso_amd.utils import graph_capture  # noqa: E402

F, RINGS, AZIMUTHS, SPREAD, MAP_VOXELS = 20, 64, 1875, 3.0, 1 << 17
N = RINGS * AZIMUTHS
# start x, y, yaw; speed per frame (m); yaw rate per frame (degrees)
TRAJECTORIES = ((-40.0, 0.0, 0.05, 1.0, 0.6), (-30.0, -6.0, 0.3, 0.8, -0.8), (20.0, 4.0, 3.0, 1.2, 0.4), (-10.0, 10.0, -0.4, 0.6, 1.0))


def workload(n_traj):
    clouds, counts = np.full((n_traj, F, N, 3), np.nan, np.float32), np.zeros((n_traj, F), np.int32)
    for k, (x, y, yaw, speed, turn) in enumerate(TRAJECTORIES[:n_traj]):
        rng = np.random.default_rng(k)
        for f in range(F):
            pts = SC.sweep(SC._pose(x, y, yaw), f, rng, RINGS, AZIMUTHS, (-24.0, 4.0), SPREAD)
            clouds[k, f, :len(pts)], counts[k, f] = pts, len(pts)
            yaw += np.deg2rad(turn)
            x, y = x + speed * np.cos(yaw), y + speed * np.sin(yaw)
    return clouds, counts


def device_ms(fn, iters, warm=1):
    for _ in range(warm):
        fn()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return round(statistics.median(times), 3)


def stage_ms(clouds, counts, n_frames):
    """the stages one by one -> {stage: ms summed over the frames}"""
    S = clouds.shape[0]
    ws = OdometryWorkspace(S, F, N, 3, "cuda", map_voxels=MAP_VOXELS)
    events = {"preprocess": [], "register": [], "map_update": []}
    for f in range(F):
        for name, call in (("preprocess", lambda: ws.preprocess(f, clouds, counts, n_frames)), ("register", lambda: ws.register(f, n_frames)),
                           ("map_update", lambda: ws.map_update(f, n_frames))):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call()
            b.record()
            events[name].append((a, b))
    torch.cuda.synchronize()
    return {k: round(sum(a.elapsed_time(b) for a, b in v), 3) for k, v in events.items()}, ws


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--host-frames", type=int, default=4)
    ap.add_argument("--sequences", default="1,16")
    args = ap.parse_args()
    sizes = [int(s) for s in args.sequences.split(",")]
    clouds, counts = workload(min(max(sizes), len(TRAJECTORIES)))
    result = {"workload": {"sweeps": F, "rays": N, "mean_points": round(float(counts.mean()), 1), "map_voxels": MAP_VOXELS}}
    for S in sizes:
        pick = np.arange(S) % len(clouds)
        d_clouds, d_counts = torch.from_numpy(clouds[pick]).cuda(), torch.from_numpy(counts[pick]).cuda()
        n_frames = torch.full((S,), F, dtype=torch.int32, device="cuda")
        call = lambda: lidar_odometry(d_clouds, d_counts, n_frames, map_voxels=MAP_VOXELS)  # noqa: E731
        res = call()
        stages, ws = stage_ms(d_clouds, d_counts, n_frames)
        assert torch.equal(ws.poses, res.poses), "the stages one by one and the whole call disagree"
        row = {"eager_device_ms": device_ms(call, args.iters), "stages_ms": stages,
               "mean_source_points": round(float(res.n_source.double().mean()), 1),
               "mean_iterations": round(float(res.n_iterations[:, 1:].double().mean()), 2), "max_iterations": int(res.n_iterations.max()),
               "converged": int(res.converged.sum()), "frames": S * F, "map_overflow": int(res.map_overflow.sum()),
               "map_voxels_used": int(ws.table("n_map_voxels").max())}
        del ws
        stream = torch.cuda.Stream()
        graph, _ = graph_capture.capture(call, stream, warm_ups=1)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            row["captured_replay_device_ms"] = device_ms(graph.replay, args.iters)
        row["ms_per_frame_and_sequence"] = round(row["captured_replay_device_ms"] / (S * F), 3)
        result[f"S={S}"] = row
        del graph
    k = max(1, min(args.host_frames, F))
    t = time.perf_counter()
    host = lidar_odometry_host(clouds[:1, :k], counts[:1, :k], np.array([k], np.int32))
    result["host_path"] = {"sequences": 1, "frames": k, "wall_ms": round(1e3 * (time.perf_counter() - t), 1), "iterations": host["n_iterations"][0].tolist()}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
