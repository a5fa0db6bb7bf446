"""SLIM validation timing.
python scripts/slim_val_time.py [batches]      -> (a) us per metrics update (B = 1, 120k points, three flows, 10 range bins) from a
    `rocprofv3 --kernel-trace --stats` run of this script's `updates` mode in a child process (both launches: partials + finish),
    plus the event-timed figure of the same loop; (b) ms per validation batch at 512^2 / 100 m, 120k points: the device pass
    (SLIM.infer_eval_flows + one metrics update, one read at the end) against the same inference followed by the reference-style
    host path (.cpu().numpy() of the five arrays + numpy metrics as liso/slim/experiment.py:600-822 computes them).
python scripts/slim_val_time.py updates [n]    -> only the update loop (what the trace run profiles)
python scripts/slim_val_time.py batches [n]    -> only (b)
The parent process never opens the GPU: (a) and (b) run as child processes with time limits, (b) only after (a) succeeded, and the
script ends with the first failing child's status (an abort, a fault or a missing trace stops everything that would follow)."""
import csv
import glob
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

dev = torch.device("cuda:0")
BINS = np.linspace(0.0, 100.0, 11)


def update_inputs():
    from liso_amd.datasets.synthetic import slim_val_batch

    s0, _ = slim_val_batch(1, dev, batch=1, n_points=120000, grid=512, bev_range_m=100.0)
    gt = s0["gt"]["flow_ta_tb"]
    g = torch.Generator(device="cpu").manual_seed(0)
    preds = [gt + (torch.randn(gt.shape, generator=g) * s).to(dev) for s in (0.2, 0.08, 0.03)]
    return s0, preds


def updates(n):
    from liso_amd.eval.flow_metrics import FlowMetricsState

    s0, preds = update_inputs()
    st = FlowMetricsState(dev)
    args = (s0["pcl_ta"]["pcl"], s0["gt"]["flow_ta_tb"], preds, s0["pcl_ta"]["pcl_is_valid"], s0["gt"]["moving_mask"],
            s0["gt"]["point_has_valid_flow_label"], BINS)
    for _ in range(10):
        st.update(*args)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        st.update(*args)
    e1.record()
    torch.cuda.synchronize()
    print(f"event-timed: {1000 * e0.elapsed_time(e1) / n:.2f} us per update (host launch included), updates {int(st.read()['updates'])}")


def numpy_host_metrics(points, gt, flows, valid, moving, label):
    """experiment.py:606-822 on host arrays: masks, FlowMetrics.update per sample, the three label categories per flow"""
    mm = moving & valid & label
    sm = ~mm & valid & label
    out = []
    rng = np.linalg.norm(points[..., :3], axis=-1)
    for pred in flows:
        epe = np.linalg.norm(pred - gt, axis=-1)
        for b in range(pred.shape[0]):
            for j in range(len(BINS) - 1):
                inb = (BINS[j] <= rng[b]) & (rng[b] < BINS[j + 1])
                for cm in (valid[b], valid[b] & ~mm[b], valid[b] & mm[b]):
                    sel = inb & cm
                    if np.count_nonzero(sel):
                        out.append(np.mean(epe[b][sel]))
        for mask in (mm | sm, mm, sm):
            with np.errstate(divide="ignore", invalid="ignore"):
                rel = epe / np.linalg.norm(gt, axis=-1)
            for a, r, mode, both in ((0.05, 0.05, 0, 0), (0.1, 0.1, 0, 0), (0.3, 0.1, 1, 0), (0.3, 0.3, 1, 1)):
                pa, pr = (epe < a, rel < r) if mode == 0 else (epe > a, rel > r)
                out.append(np.count_nonzero(((pa & pr) if both else (pa | pr)) & mask) / max(np.count_nonzero(mask), 1))
            out += [np.mean(epe[mask]), pred[mask].mean(axis=0), np.mean(np.linalg.norm(pred[mask], axis=-1)), gt[mask].mean(axis=0),
                    np.mean(np.linalg.norm(gt[mask], axis=-1)), (pred - gt)[mask].mean(axis=0), np.mean(np.linalg.norm(gt, axis=-1)[mask])]
    return out


def per_batch(n_batches):
    from liso_amd.datasets.synthetic import slim_val_batch
    from liso_amd.eval.flow_metrics import FlowMetricsState
    from liso_amd.slim.model.slim import SLIM
    from liso_amd.utils.config import default_cfg

    torch.manual_seed(0)
    net = SLIM(default_cfg(grid=512, bev_range_m=100.0), 100).to(dev).eval()
    batches = [slim_val_batch(100 + i, dev, batch=1, n_points=120000, grid=512, bev_range_m=100.0) for i in range(3)]
    for s0, s1 in batches:  # warm-up
        net.infer_eval_flows(s0, s1)
    torch.cuda.synchronize()

    def device_pass():
        st = FlowMetricsState(dev)
        for i in range(n_batches):
            s0, s1 = batches[i % 3]
            p = net.infer_eval_flows(s0, s1)
            st.update(s0["pcl_ta"]["pcl"], s0["gt"]["flow_ta_tb"], [p.static_flow, p.aggregated_flow, p.static_aggr_flow],
                      s0["pcl_ta"]["pcl_is_valid"], s0["gt"]["moving_mask"], s0["gt"]["point_has_valid_flow_label"], BINS)
        st.read()

    def host_pass():
        for i in range(n_batches):
            s0, s1 = batches[i % 3]
            p = net.infer_eval_flows(s0, s1)
            flows = [p.static_flow.cpu().numpy(), p.aggregated_flow.cpu().numpy(), p.static_aggr_flow.cpu().numpy()]
            numpy_host_metrics(s0["pcl_ta"]["pcl"].cpu().numpy(), s0["gt"]["flow_ta_tb"].cpu().numpy(), flows,
                               s0["pcl_ta"]["pcl_is_valid"].cpu().numpy(), s0["gt"]["moving_mask"].cpu().numpy(),
                               s0["gt"]["point_has_valid_flow_label"].cpu().numpy())

    def infer_only():
        for i in range(n_batches):
            s0, s1 = batches[i % 3]
            net.infer_eval_flows(s0, s1)
        torch.cuda.synchronize()

    for name, fn in (("inference only", infer_only), ("device pass", device_pass), ("host numpy pass", host_pass)):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        print(f"{name:16s}: {1000 * (time.perf_counter() - t0) / n_batches:8.2f} ms per batch ({n_batches} batches)", flush=True)


def traced_updates(n):
    """-> 0, or the status to end the script with (no further GPU work after a failed child)"""
    out = tempfile.mkdtemp(prefix="slim_val_trace_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "run", "--", sys.executable,
           os.path.abspath(__file__), "updates", str(n)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    print(r.stdout.strip().splitlines()[-1] if r.stdout.strip() else "", flush=True)
    if r.returncode != 0:
        print("rocprofv3 run failed:", r.returncode, r.stderr[-2000:])
        return r.returncode
    stats = glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)
    if not stats:
        print("no kernel_stats.csv under", out, ":", sorted(glob.glob(os.path.join(out, "**"), recursive=True))[:20], r.stderr[-1500:])
        return 1
    total = 0.0
    for row in csv.DictReader(open(stats[0])):
        if "flow_metrics" in row["Name"]:
            avg = float(row["AverageNs"]) / 1000
            print(f"  {row['Name'][:90]:90s} calls {row['Calls']:>6s}  {avg:7.2f} us")
            if "reset" not in row["Name"]:
                total += avg
    print(f"kernel trace: {total:.2f} us per update (partials + finish)", flush=True)
    return 0


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "updates":
        updates(int(sys.argv[2]) if len(sys.argv) > 2 else 200)
    elif len(sys.argv) > 1 and sys.argv[1] == "batches":
        per_batch(int(sys.argv[2]) if len(sys.argv) > 2 else 10)
    else:
        n = int(sys.argv[1]) if len(sys.argv) > 1 else 10
        rc = traced_updates(200)
        if rc != 0:
            sys.exit(rc)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "batches", str(n)], cwd=ROOT, timeout=900)
        sys.exit(r.returncode)
