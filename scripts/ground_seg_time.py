"""Ground segmentation timing (include/liso_ground.h), device events after warm-up, medians over `reps` runs.
python scripts/ground_seg_time.py [reps]   -> one JSON line each for, at the KITTI parameters (2083x64, 1.73 m, delta_R 1):
    whole   one 120k-point cloud and a batch of 4: the whole JPCGroundRemove call, and remove_ground_points (JCP + cone + compaction)
    stages  each stage of liso_ground_jcp_f32 on its own (liso_ground_jcp_stages_f32 on the workspace the earlier stages left):
            init, elevation, projection, recm, candidates, resolve, gather -- the resolve wavefront is the one to watch
    host    the numpy host path on the same cloud (wall clock, one CPU core)
One process, one stream; every timed call is preceded by 3 untimed ones."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KITTI = dict(range_img_width=2083, range_img_height=64, sensor_height=1.73, delta_R=1)


def median_ms(fn, reps):
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
    return round(t[len(t) // 2], 4), round(t[0], 4)


def main():
    import torch

    from liso_amd.datasets.synthetic import make_scene, render
    from liso_amd.jcp import jcp

    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    dev = torch.device("cuda:0")
    clouds = [render(make_scene(s, dev)[0], dev, s)[0].contiguous() for s in range(4)]  # [120000, 4]
    for batch in (1, 4):
        full = torch.stack(clouds[:batch]).contiguous()
        xyz = full[..., :3].contiguous()
        med, best = median_ms(lambda: jcp.jcp_device(xyz, **KITTI), reps)
        print(json.dumps({"mode": "whole", "call": "JPCGroundRemove", "B": batch, "N": 120000, "median_ms": med, "min_ms": best}), flush=True)
        med, best = median_ms(lambda: jcp.remove_ground_points(full, **KITTI), reps)
        print(json.dumps({"mode": "whole", "call": "remove_ground_points", "B": batch, "N": 120000, "median_ms": med, "min_ms": best}), flush=True)
        state = jcp.jcp_device(xyz, stages=(0, jcp.N_STAGES), **KITTI)
        row = {"mode": "stages", "B": batch, "N": 120000}
        for s, name in enumerate(jcp.STAGES):
            # stages 0..s-1 are idempotent given the same cloud, so the workspace stays what stage s expects; stage 0 resets it
            def one(s=s):
                jcp.jcp_device(xyz, stages=(0, s), state=state, **KITTI)

            def both(s=s):
                jcp.jcp_device(xyz, stages=(0, s + 1), state=state, **KITTI)

            upto, _ = median_ms(both, reps)
            before, _ = median_ms(one, reps) if s else (0.0, 0.0)
            row[name + "_ms"] = round(upto - before, 4)
        print(json.dumps(row), flush=True)
    p = clouds[0][:, :3].cpu().numpy()
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        labels, info = jcp.jcp_host(p, debug=True, **KITTI)
        times.append(1000 * (time.perf_counter() - t0))
    print(json.dumps({"mode": "host", "N": 120000, "numpy_host_path_ms": round(sorted(times)[1], 1), "candidates": int(info["candidates"].shape[0]),
                      "ground": int(labels.sum())}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
