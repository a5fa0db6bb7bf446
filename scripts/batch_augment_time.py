"""Box-snippet augmentation of a batch with device draws (liso_amd/datasets/batch_augmentation.py) against the per-sweep path
(`BoxAugmenter.create_augmented_sample_from_box_snippet_db`, reference_draws=False) on the same sweeps, in the same run, alternating.
Workload: B = 4 sweeps of 120k points, 512^2 BEV over 100 m, a database of 300 snippets / ~100k points, the reference's augmentation
block (<= 15 objects, point drop-out 0.25).  Device events around each timed piece, after warm-up; medians.  Prints one JSON line.
    python scripts/batch_augment_time.py [--rounds 30]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def kernel_launches(fn):
    """device kernels launched by one fn(), all libraries, counted by torch.profiler; None where it gives no device events"""
    from torch.profiler import ProfilerActivity, profile

    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "memcpy" not in e.name.lower()
             and "memset" not in e.name.lower()]
    return len(names) or None


def event_ms(fn, repeat=1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(repeat):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / repeat


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    args = ap.parse_args()
    from liso_amd.datasets import batch_augmentation as BA
    from liso_amd.datasets.box_augmentation import BoxAugmenter, BoxSnippetDb
    from liso_amd.datasets.sample_prep import assemble_bev_sample
    from liso_amd.datasets.synthetic import slim_pair
    from liso_amd.kabsch.shape_utils import Shape
    from liso_amd.utils import graph_capture
    from liso_amd.utils.config import default_cfg, to_attr

    dev = torch.device("cuda:0")
    B, G, R, N, M = 4, 512, 100.0, 120000, 300
    cfg = default_cfg(grid=G, bev_range_m=R)
    cfg.data.limit_pillar_height = False
    cfg.data.flow_source, cfg.data.train_on_box_source = "slim_flow", "mined"
    cfg.data.augmentation = to_attr({"boxes": {"active": True, "max_num_objs": 15, "min_artificial_obj_velo": 1.0,
                                               "max_artificial_obj_velo": 3.0, "max_scale_delta": 0.2, "max_points_dropout": 0.25,
                                               "use_raydrop_augm": False}})
    clouds = []
    for b in range(B):
        s0, _ = slim_pair(3 + b, dev, n_points=N, grid=G, bev_range_m=R)
        clouds.append(s0["pcl_ta"]["pcl"][0][s0["pcl_ta"]["pcl_is_valid"][0]][:, :4].contiguous())
    n_max = max(c.shape[0] for c in clouds)
    pcl = torch.full((B, n_max, 4), float("nan"), device=dev)
    for b, c in enumerate(clouds):
        pcl[b, :c.shape[0]] = c
    counts = torch.tensor([c.shape[0] for c in clouds], dtype=torch.int32, device=dev)
    flow = torch.zeros((B, n_max, 3), device=dev)
    batch = assemble_bev_sample(pcl, counts, flow=flow, cfg=cfg)
    batch["pcl_full_w_ground_ta"] = {"pcl": pcl, "counts": counts}
    batch["pcl_full_no_ground_ta"] = {"pcl": pcl, "counts": counts}
    batch["sample_ids"] = torch.arange(B, dtype=torch.int64, device=dev)

    rs = np.random.default_rng(0)
    sizes = rs.integers(11, 656, M)
    pcls = [np.concatenate([rs.uniform(-1, 1, (c, 3)) * [2.2, 1.0, 0.8], rs.uniform(0, 1, (c, 1))], -1).astype(np.float32) for c in sizes]
    boxes = Shape(pos=torch.zeros(M, 3), dims=torch.tensor([[4.4, 2.0, 1.6]]).repeat(M, 1), rot=torch.zeros(M, 1), probs=torch.ones(M, 1))
    db = BoxSnippetDb({"pcl_in_box_cosy": pcls, "boxes": boxes}, dev)

    batched = BA.BatchBoxAugmenter(cfg, db, need_flow=True, seed=0)
    whole = lambda: batched(batch)  # noqa: E731
    paste = lambda: BA.paste_snippets_batch(db, batch["pcl_ta"]["pcl"], batch["counts"], batch["pcl_ta"]["pillar_coors"], cfg=cfg,  # noqa: E731
                                            draws=batched.draws, sample_ids=batch["sample_ids"], extra_capacity=batched.extra_capacity)
    per_sweep = BoxAugmenter(cfg, db, need_flow=True, reference_draws=False)
    singles = []
    for b in range(B):
        n = int(batch["counts"][b])
        p = batch["pcl_ta"]["pcl"][b, :n].contiguous()
        singles.append({"pcl_ta": {"pcl": p, "pillar_coors": batch["pcl_ta"]["pillar_coors"][b, :n].contiguous()},
                        "pcl_full_w_ground_ta": clouds[b], "pcl_full_no_ground_ta": clouds[b], "gt": {},
                        "slim_flow": {"flow_ta_tb": batch["flow_ta_tb"][b, :n].contiguous()}})
    np.random.seed(0)
    torch.manual_seed(0)
    four = lambda: [per_sweep.create_augmented_sample_from_box_snippet_db(0.1, s) for s in singles]  # noqa: E731

    stream = torch.cuda.Stream()
    graphs = {}
    for name, fn in (("call", whole), ("paste_only", paste)):
        graphs[name], _ = graph_capture.capture(fn, stream, warm_ups=2)
    torch.cuda.synchronize()
    for _ in range(3):
        whole(), paste(), four()
    torch.cuda.synchronize()
    times = {k: [] for k in ("batched_call_eager", "batched_call_replay", "paste_only_eager", "paste_only_replay", "per_sweep_x4")}
    for _ in range(args.rounds):
        times["batched_call_eager"].append(event_ms(whole))
        times["paste_only_eager"].append(event_ms(paste))
        times["per_sweep_x4"].append(event_ms(four))
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            times["batched_call_replay"].append(event_ms(graphs["call"].replay, 10))
            times["paste_only_replay"].append(event_ms(graphs["paste_only"].replay, 10))
        torch.cuda.synchronize()
    result = {"workload": {"B": B, "points_per_sweep": [int(c) for c in counts.tolist()], "grid": G, "range_m": R, "snippets": M,
                           "db_points": int(db.points.shape[0]), "extra_capacity": batched.extra_capacity, "rounds": args.rounds},
              "median_ms": {k: round(statistics.median(v), 4) for k, v in times.items()},
              "min_ms": {k: round(min(v), 4) for k, v in times.items()},
              "launches": {"batched_call": kernel_launches(whole), "paste_only": kernel_launches(paste), "per_sweep_x4": kernel_launches(four)},
              "pasted_points_last_call": [int(v) for v in batched(batch)["extra_counts"].tolist()]}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
