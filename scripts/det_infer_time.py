"""Detector inference post-processing timing: dense maps -> post-NMS boxes (include/liso_det_nms.h).
python scripts/det_infer_time.py [reps]       -> both measurements below, each in a child process with a time limit; the second only
    after the first succeeded, and the script ends with the first failing child's status.
python scripts/det_infer_time.py phases [reps]   -> ms of (a) order, (b) select, (c) gather, device events around each C call,
    B = 1, 2, 4 x N = 16384 (512^2 input, 128^2 head) and 65536 (1024^2 input, 256^2 head) x (P = 500, no pre cut) and
    (pre 1000, P = 100) x two candidate families: an untrained detector (keyed weights) on synthetic.detector_batch, and
    synthetic.detector_map_trained_like (score peaks and box jitter around 30 objects).
python scripts/det_infer_time.py fullmask [reps] -> the existing path for comparison, per sample: torch.sort + nms_gpu_device
    (N x N suppression mask + greedy sweep) + the host-synced compaction of rotate_nms_pcdet; N = 65536 runs once (512 MB mask).
The parent process never opens the GPU."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

SIDES = (128, 256)
BATCHES = (1, 2, 4)
SETTINGS = ((None, 500), (1000, 100))


def _maps(side, batch, dev):
    import torch

    from keyed_init import keyed_state_dict
    from liso_amd.datasets.synthetic import detector_batch, detector_map_trained_like
    from liso_amd.networks.simple_net.simple_net import BoxLearner
    from liso_amd.utils.config import default_cfg

    grid = side * 4
    cfg = default_cfg(grid=grid, bev_range_m=100.0)
    net = BoxLearner(cfg).to(dev)
    sd = net.state_dict()
    init = keyed_state_dict({k: (tuple(v.shape), v.dtype) for k, v in sd.items()})
    net.load_state_dict({**sd, **{k: v.to(dev) for k, v in init.items()}}, strict=True)
    net.eval()
    pcls, _ = detector_batch(5, batch, dev, n_points=120000, grid=grid, bev_range_m=100.0)
    with torch.no_grad():
        untrained = net(None, pcls, train=False)[0]
    del net
    return {"untrained": untrained, "trained_like": detector_map_trained_like(7, batch, side, dev)}


def phases(reps):
    import torch

    from liso_amd import det_nms as D
    from liso_amd.utils.nms_iou import convert_shapes_to_dense_3d

    dev = torch.device("cuda:0")
    names = ("pos", "dims", "rot", "probs", "velo", "valid", "class_id", "difficulty")
    for side in SIDES:
        for batch in BATCHES:
            for family, boxes in _maps(side, batch, dev).items():
                dense = convert_shapes_to_dense_3d(boxes).float().contiguous()
                logits = boxes.probs[..., 0].contiguous()
                scores = torch.sigmoid(logits)
                valid = boxes.valid.contiguous()
                srcs = [getattr(boxes, k).contiguous() for k in names]
                pads = [0.0] * 5 + [False, 2147483646, 2147483646]
                for pre, post in SETTINGS:
                    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(reps)]
                    for i in range(3 + reps):
                        e = ev[i - 3] if i >= 3 else None
                        if e: e[0].record()
                        keys, idx = D.order(scores, logits, valid, -1e32)
                        if e: e[1].record()
                        keep, counts = D.select(dense, keys, idx, 0.1, pre, post)
                        if e: e[2].record()
                        D.gather(keep, counts, srcs, pads)
                        if e: e[3].record()
                    torch.cuda.synchronize()
                    t = [[e[j].elapsed_time(e[j + 1]) for e in ev] for j in range(3)]
                    med = [sorted(x)[len(x) // 2] for x in t]
                    print(json.dumps({"mode": "phases", "N": side * side, "B": batch, "family": family, "pre": pre, "P": post,
                                      "order_ms": round(med[0], 4), "select_ms": round(med[1], 4), "gather_ms": round(med[2], 4),
                                      "kept": counts.tolist()}), flush=True)


def fullmask(reps):
    import torch

    from liso_amd import iou3d_nms_cuda as M
    from liso_amd.utils.nms_iou import convert_shapes_to_dense_3d

    dev = torch.device("cuda:0")
    for side in SIDES:
        for family, boxes in _maps(side, 1, dev).items():
            dense = convert_shapes_to_dense_3d(boxes[0]).float().contiguous()
            scores = torch.sigmoid(boxes.probs[0, :, 0])
            n_runs = reps if side * side <= 16384 else 1
            times = []
            for i in range(n_runs + (1 if n_runs > 1 else 0)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                order = scores.sort(0, descending=True)[1]
                kd, nd = M.nms_gpu_device(dense[order].contiguous(), 0.1)
                sel = order[kd[: int(nd.item())]][:500]  # rotate_nms_pcdet's host-synced compaction
                torch.cuda.synchronize()
                if n_runs == 1 or i > 0:
                    times.append(1000 * (time.perf_counter() - t0))
                del kd
            print(json.dumps({"mode": "fullmask", "N": side * side, "B": 1, "family": family, "P": 500, "runs": len(times),
                              "ms_per_sample": round(sorted(times)[len(times) // 2], 3), "kept": int(sel.numel())}), flush=True)


def main():
    args = sys.argv[1:]
    if args and args[0] in ("phases", "fullmask"):
        reps = int(args[1]) if len(args) > 1 else 20
        (phases if args[0] == "phases" else fullmask)(reps)
        return 0
    reps = args[0] if args else "20"
    for mode, limit in (("phases", 900), ("fullmask", 600)):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), mode, reps], cwd=ROOT, timeout=limit)
        except subprocess.TimeoutExpired:
            print(f"{mode}: time limit of {limit} s reached; stopping", flush=True)
            return 124
        if r.returncode != 0:
            print(f"{mode}: exit status {r.returncode}; stopping", flush=True)
            return r.returncode if r.returncode > 0 else 128 - r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
