"""Sample preparation timing (include/liso_sample_prep.h): two 120k-point sweeps with flow, the batch the fused iteration feeds.
python scripts/sample_prep_time.py [reps]   -> one JSON line each for
    entry   every entry point on its own: device events around `reps` calls after 3 untimed ones, median and min, and the achieved
            bytes/s against the algorithmic traffic (each input row read once, each output row written once)
    chain   augment_sample_content -> assemble_bev_sample captured once through graph_capture.capture, events around each replay
    host    the package's numpy host path on the same inputs (wall clock, one CPU core)
One process, one stream."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GRID, RANGE, THRESHOLD_DT = (640, 640), (100.0, 100.0), 0.05


class Cfg(dict):
    __getattr__ = dict.__getitem__


CFG = Cfg(data=Cfg(odom_source="gt", flow_source="gt", bev_range_m=RANGE, img_grid_size=GRID, limit_pillar_height=False,
                   non_rigid_flow_threshold_mps=0.5))


def timed(fn, reps):
    import torch

    for _ in range(3):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) for a, b in ev)
    return {"median_ms": round(t[len(t) // 2], 4), "min_ms": round(t[0], 4), "max_ms": round(t[-1], 4)}


def main():
    import numpy as np
    import torch

    from liso_amd.datasets import sample_prep as S
    from liso_amd.datasets.synthetic import make_scene, render
    from liso_amd.utils import graph_capture

    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    dev = torch.device("cuda:0")
    pcl = torch.stack([render(make_scene(s, dev)[0], dev, s)[0] for s in range(2)]).contiguous()  # [2, 120000, 4]
    B, N, C = pcl.shape
    flow = torch.randn(B, N, 3, device=dev)
    rows = torch.randint(0, 64, (B, N), device=dev, dtype=torch.int32)
    drop = torch.rand(B, N, device=dev) < 0.3
    np.random.seed(0)
    T = torch.from_numpy(np.stack([S.get_augmentation_transform(90.0, 5.0) for _ in range(B)])).to(dev)
    odom = torch.eye(4, dtype=torch.float64, device=dev).repeat(B, 1, 1)
    odom[:, 0, 3] = 1.0
    H, W = GRID

    def report(name, fn, nbytes):
        r = timed(fn, reps)
        r.update({"mode": "entry", "call": name, "B": B, "N": N, "algorithmic_MB": round(nbytes / 1e6, 2),
                  "GB_per_s": round(nbytes / r["median_ms"] / 1e6, 1)})
        print(json.dumps(r), flush=True)

    report("liso_sample_transform_f32", lambda: S.transform_cloud_device(pcl, T, flow=flow), 2 * B * N * (C + 3) * 4)
    crop_kw = dict(bev_range_m=RANGE, img_grid_size=GRID, flow=flow, lidar_rows=rows, drop=drop)
    crop = S.pillarize_bev(pcl, **crop_kw)
    kept = int(crop["counts"].sum())
    report("liso_bev_crop_f32", lambda: S.pillarize_bev(pcl, **crop_kw),
           B * N * ((C + 3) * 4 + 4 + 1) + B * N * ((C + 3) * 4 + 4 + 8))
    maps = lambda: S.bev_point_maps(crop["pillar_coors"], crop["counts"], GRID, pcl=crop["pcl"], flow=crop["flow"], odom_tb_ta=odom,  # noqa: E731
                                    threshold_dt=THRESHOLD_DT)
    report("liso_bev_point_maps_f32", maps, kept * (C * 4 + 12 + 8 + 1) + B * H * W * 16)
    boxes = [(torch.randn(B, 64, 3, device=dev, dtype=torch.float64), torch.randn(B, 64, 1, device=dev, dtype=torch.float64), None)]
    inv, new = torch.empty_like(odom), torch.empty_like(odom)
    report("liso_sample_transform_poses_f64", lambda: S.transform_poses_device(T, boxes, [(odom, new, inv)]), B * (64 * 4 * 8 * 2 + 3 * 128))

    static = [pcl.clone(), flow.clone(), T.clone()]

    def chain():
        sample = {"pcl_t0": static[0], "pcl_t1": static[0], "gt": {"flow_t0_t1": static[1], "odom_t0_t1": odom}}
        S.augment_sample_content(sample, "t0", "t1", "waymo", cfg=CFG, T=static[2])
        return S.assemble_bev_sample(sample["pcl_t0"], None, flow=sample["gt"]["flow_t0_t1"], lidar_rows=rows, drop=drop,
                                     odom_tb_ta=sample["gt"]["odom_t1_t0"], dt=0.1, cfg=CFG)

    r = timed(chain, reps)
    r.update({"mode": "chain", "how": "eager", "B": B, "N": N})
    print(json.dumps(r), flush=True)
    stream = torch.cuda.Stream()
    graph, _ = graph_capture.capture(chain, stream, warm_ups=2)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        r = timed(graph.replay, reps)
    r.update({"mode": "chain", "how": "captured", "B": B, "N": N, "kept_rows": kept})
    print(json.dumps(r), flush=True)

    p, f, rw, dr, Tn, od = pcl[0].cpu().numpy(), flow[0].cpu().numpy(), rows[0].cpu().numpy(), drop[0].cpu().numpy(), T[0].cpu().numpy(), odom[0].cpu().numpy()
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        tp, tf = S.transform_cloud_host(p, Tn, f)
        c = S.bev_crop_host(tp, bev_range_m=RANGE, img_grid_size=GRID, flow=tf, lidar_rows=rw, drop=dr)
        S.bev_point_maps_host(c["pillar_coors"], GRID, c["flow"])
        S.moving_mask_host(c["pcl"], c["flow"], od, THRESHOLD_DT)
        times.append(1000 * (time.perf_counter() - t0))
    print(json.dumps({"mode": "host", "N": N, "sweeps": 1, "numpy_host_path_ms": round(sorted(times)[1], 1)}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
