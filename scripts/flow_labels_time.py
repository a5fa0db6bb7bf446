"""Times the flow labels (liso_amd/datasets/flow_labels.py) and KITTI's rows and columns (range_projection.py) on the device:
medians of device events after warm-up, eager and per replay when captured in a hipGraph, next to the numpy host path on the same
data.  Workload: the six directed jobs of two samples of three sweeps, 120 000 points per sweep, 50 boxes; the rows and columns of
one 120 000-point sweep.  The kernel launches of one call are counted with torch.profiler (all libraries, and this library's own:
the header fixes two and one); the capture shows that neither call reads on the host.  Prints one JSON line.
    python scripts/flow_labels_time.py [--iters 50] [--host-iters 1]
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

from liso_amd.datasets import flow_labels as F  # noqa: E402
from liso_amd.datasets import range_projection as R  # noqa: E402
from liso_amd.utils import graph_capture  # noqa: E402

B, T, K, N = 2, 3, 50, 120_000


def yaw_poses(xyz, yaw):
    P = np.tile(np.eye(4), xyz.shape[:-1] + (1, 1))
    P[..., 0, 0], P[..., 0, 1], P[..., 1, 0], P[..., 1, 1] = np.cos(yaw), -np.sin(yaw), np.sin(yaw), np.cos(yaw)
    P[..., :3, 3] = xyz
    return P


def workload():
    g = np.random.default_rng(0)
    clouds = np.concatenate([g.uniform(-60, 60, (B, T, N, 2)), g.uniform(-3, 2, (B, T, N, 1)), g.uniform(0, 1, (B, T, N, 1))], -1).astype(np.float32)
    counts = np.full((B, T), N, np.int32)
    counts[1, 2] = N - 7000
    xyz0 = np.concatenate([g.uniform(-55, 55, (B, 1, K, 2)), g.uniform(-1.5, -0.5, (B, 1, K, 1))], -1)
    xyz = xyz0 + np.arange(T)[None, :, None, None] * np.concatenate([g.uniform(-1, 1, (B, 1, K, 2)), np.zeros((B, 1, K, 1))], -1)
    yaw = g.uniform(-np.pi, np.pi, (B, 1, K)) + 0.02 * np.arange(T)[None, :, None]
    sizes = np.stack([g.uniform(3, 5, (B, K)), g.uniform(1.5, 2.2, (B, K)), g.uniform(1.4, 1.9, (B, K))], -1)
    odoms = yaw_poses(np.concatenate([g.uniform(0.5, 1.5, (B, 6, 1)), g.uniform(-0.1, 0.1, (B, 6, 2))], -1), g.uniform(-0.02, 0.02, (B, 6)))
    scan_az = np.sort(g.uniform(-3.1, 3.1, (64, N // 64)), -1).reshape(-1)
    rho = g.uniform(4, 60, scan_az.shape[0])
    sweep = np.stack([-np.cos(scan_az) * rho, -np.sin(scan_az) * rho, g.uniform(-2, 1, scan_az.shape[0]), rho], -1).astype(np.float32)
    return dict(clouds=clouds, counts=counts, poses_per_time=yaw_poses(xyz, yaw), present=g.uniform(size=(B, T, K)) > 0.1, sizes=sizes,
                labels=g.integers(0, 5000, (B, K)).astype(np.int32), odoms=odoms), sweep


def entries(w, sweep):
    """`sample_flow_labels` assembles the job tables (stacking, a dozen small copies) and calls `flow_labels`; `flow_labels` is the
    call alone, on tables assembled beforehand"""
    jobs, _ = F.sample_jobs(**w)
    fn = F.flow_labels_host if isinstance(sweep, np.ndarray) else F.flow_labels
    return {"sample_flow_labels": lambda: F.sample_flow_labels(**w), "flow_labels": lambda: fn(**jobs, no_label=F.DUMMY_TRACK_ID),
            "kitti_rows_cols": lambda: R.kitti_pcl_projection_get_rows_cols(sweep)}


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


def kernel_launches(fn):
    """device kernels launched by one fn(), all libraries, counted by torch.profiler (as scripts/det_val_time.py does); None where
    the profiler gives no device events"""
    from torch.profiler import ProfilerActivity, profile

    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "memcpy" not in e.name.lower()
             and "memset" not in e.name.lower()]
    return {"all": len(names) or None, "this_library": sum("flow_" in n or "rows_cols" in n for n in names) or None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--host-iters", type=int, default=1)
    args = ap.parse_args()
    w, sweep = workload()
    result = {"workload": {"samples": B, "sweeps": T, "jobs": B * 6, "K": K, "N": N, "rows_cols_N": int(sweep.shape[0])},
              "launches_per_call": {}, "host_ms": {}, "device_ms": {}, "captured_ms": {}}
    for name, fn in entries(w, sweep).items():
        times = []
        for _ in range(args.host_iters):
            t = time.perf_counter()
            fn()
            times.append(1e3 * (time.perf_counter() - t))
        result["host_ms"][name] = round(statistics.median(times), 3)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    dev = entries({k: to(v) for k, v in w.items()}, to(sweep))
    stream = torch.cuda.Stream()
    for name, fn in dev.items():
        result["device_ms"][name] = round(device_ms(fn, args.iters), 4)
        result["launches_per_call"][name] = kernel_launches(fn)
        graph, _ = graph_capture.capture(fn, stream, warm_ups=2)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            result["captured_ms"][name] = round(device_ms(graph.replay, args.iters), 4)
        torch.cuda.synchronize()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
