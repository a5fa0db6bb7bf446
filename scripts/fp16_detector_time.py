"""The detector train step (one-graph hipGraph step + eager pillar encoder + AdamW, as bench.py --workload detector runs it) in bf16 and
in fp16 on the same harness: B = 4 / 512^2 (120k points per cloud) and BASELINE configs[4] (B = 2 as `bench.py --workload stress`, 300k
5-channel points, 1024^2).
fp16 adds the loss scale's three launches behind the backward pass (overflow check, gated AdamW, scale update).
python scripts/fp16_detector_time.py [steps]      -> one line per (configuration, dtype): ms per step (event-timed), last loss"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from liso_amd.datasets.synthetic import detector_batch  # noqa: E402
from liso_amd.trainer import DetectorTrainer  # noqa: E402
from liso_amd.utils.config import default_cfg  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
dev = torch.device("cuda:0")
for name, B, grid, n, ch in (("B4_512", 4, 512, 120000, None), ("configs4_1024", 2, 1024, 300000, 5)):
    for dtype in (torch.bfloat16, torch.float16):
        torch.manual_seed(0)
        cfg = default_cfg(grid=grid, bev_range_m=100.0)
        if ch:
            cfg.data.num_point_channels = ch
        tr = DetectorTrainer(cfg, dev, compute_dtype=dtype, total_steps=steps + 10, use_graph=True)
        pcls, targets = detector_batch(1, B, dev, n_points=n, grid=grid, bev_range_m=100.0)
        if ch:
            g = torch.Generator().manual_seed(3)
            pcls = [torch.cat([p, (torch.randint(0, 10, (p.shape[0], 1), generator=g).float() * 0.05).to(dev)], dim=1) for p in pcls]
        for _ in range(5):
            loss = tr.step(pcls, targets)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            loss = tr.step(pcls, targets)
        e1.record()
        torch.cuda.synchronize()
        extra = f"  loss scale {tr.loss_scale_stats()}" if tr.loss_scaler is not None else ""
        print(f"{name} {str(dtype).split('.')[-1]:9s}: {e0.elapsed_time(e1) / steps:7.3f} ms per step, last loss {float(loss):.4f}{extra}",
              flush=True)
        del tr
        torch.cuda.empty_cache()
