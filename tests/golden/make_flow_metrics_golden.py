"""Generates tests/golden/flow_metrics_reference.npz from the reference's own scene-flow metrics:
  liso/slim/utils/metrics.py   compute_scene_flow_metrics_for_points_in_this_mask + aggregate_metrics
  liso/eval/flow_metrics.py    FlowMetrics(range_bins).update(...) per sample, then its running averages
called per batch and per flow exactly as liso/slim/experiment.py:600-827 (`run_eval_on_this_dataset`) calls them, on synthetic
batches that hold the edge cases: EPE and relative error one f32 ulp either side of 0.05 / 0.1 / 0.3, zero ground-truth flow
with and without error, ranges on and beyond the bin edges, points without flow label, padding rows, a batch without moving
points and a batch with an empty label set.  The two reference files are loaded by path; the modules stubbed for their imports are
matplotlib, matplotlib.pyplot, torch.utils.tensorboard, and `liso` with `liso.visu` / `liso.visu.utils` (flow_metrics.py imports
plot_to_np_image from there; nothing numeric comes from any of them).
With the installed numpy an empty label set makes the reference raise ZeroDivisionError in get_ratio_for_thresh
(np.count_nonzero returns a Python int); that batch's dict is then the all-NaN dict with num_pts_used 0, which the reference's
aggregate_metrics turns into NaN.
Run in the build container only:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_flow_metrics_golden.py
"""
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_targets_golden import _Anything  # noqa: E402
from ref_import import load  # noqa: E402

for _name in ("matplotlib", "matplotlib.pyplot", "torch.utils.tensorboard", "liso", "liso.visu", "liso.visu.utils"):
    sys.modules[_name] = _Anything(_name)

FLOWS = ("raw", "agg", "rig")
CATS = ("overall", "moving", "still")


def edge_rows():
    """(points, gt, pred) rows of the threshold / zero-flow / range edge cases"""
    f32 = np.float32
    pts, gts, preds = [], [], []
    ranges = [0.0, 5.0, 10.0, np.nextafter(f32(10.0), f32(0.0)), 99.99999, 100.0, 100.00001, 150.0, 250.0]
    for thr in (0.05, 0.1, 0.3):
        t = f32(thr)
        for e in (np.nextafter(t, f32(-1)), t, np.nextafter(t, f32(1))):
            for G in (f32(64.0), f32(1.0 / 64.0)):  # relative error far below / above every threshold: the absolute one decides
                gts.append((0, G, 0)), preds.append((e, G, 0))
            gts.append((0, 8, 0)), preds.append((f32(8) * e, 8, 0))  # relative error == e exactly (power-of-two scaling)
    for p in ((0, 0, 0), (0.02, 0, 0), (1.0, 0, 0), (0, 0, 0.3)):  # zero ground truth: rel NaN (no error) or inf
        gts.append((0, 0, 0)), preds.append(p)
    for i in range(len(gts)):
        r = ranges[i % len(ranges)]
        pts.append((r, 0, 0, 0.5))
    a = lambda v: np.array(v, np.float32)  # noqa: E731
    p, g, q = a(pts), a(gts), a(preds)
    epe = np.linalg.norm(q - g, axis=-1)
    assert np.all(epe[:27] == np.abs(q[:27, 0]))  # the constructed errors are exact
    return p, g, q


def make_batch(g, B, N, *, edge=False, no_moving=False, no_label=False, nan_padding=False):
    az = g.uniform(-np.pi, np.pi, (B, N))
    r = g.uniform(0.5, 130.0, (B, N))
    pts = np.stack([r * np.cos(az), r * np.sin(az), g.uniform(-1.5, 2.0, (B, N)), g.uniform(0, 1, (B, N))], -1).astype(np.float32)
    moving = (g.uniform(size=(B, N)) < 0.3) & (not no_moving)
    gt = np.stack([g.uniform(0.3, 1.5, (B, N)), g.normal(0, 0.05, (B, N)), g.normal(0, 0.01, (B, N))], -1)
    gt[moving] += np.stack([g.uniform(-2, 2, moving.sum()), g.uniform(-2, 2, moving.sum()), np.zeros(moving.sum())], -1)
    gt = gt.astype(np.float32)
    gt[g.uniform(size=(B, N)) < 0.02] = 0.0  # some zero ground-truth flows
    preds = []
    for scale in (0.25, 0.08, 0.03):
        q = gt + g.normal(0, scale, gt.shape).astype(np.float32) * g.exponential(1.0, (B, N, 1)).astype(np.float32)
        q[g.uniform(size=(B, N)) < 0.05] = 0.0
        preds.append(q.astype(np.float32))
    valid = np.ones((B, N), bool)
    label = g.uniform(size=(B, N)) >= 0.04
    for b in range(B):
        n_pad = 3 + 11 * b
        valid[b, N - n_pad:] = False
        pts[b, N - n_pad:] = 0.0
        if nan_padding:
            for q in preds:
                q[b, N - n_pad:] = np.nan
    if edge:
        p, gg, q = edge_rows()
        m = len(p)
        pts[0, :m], gt[0, :m] = p, gg
        for k, qq in enumerate(preds):
            qq[0, :m] = q if k == 0 else q[::-1] if k == 1 else np.roll(q, 5, axis=0)
        valid[0, :m], label[0, :m] = True, True
        moving[0, :m] = (np.arange(m) % 2 == 0) & (not no_moving)
    if no_label:
        label[:] = False
    return dict(points=pts, gt=gt, preds=np.stack(preds), valid=valid, moving=moving, label=label)


def run_reference(M, FM, batches, bins):
    """experiment.py:600-827 on host arrays"""
    lists = {f"{f}/{c}": [] for c in CATS for f in FLOWS}
    fms = {f: FM.FlowMetrics(range_bins=bins) for f in FLOWS}
    for bt in batches:
        moving_mask = bt["moving"] & bt["valid"] & bt["label"]
        static_mask = np.logical_not(moving_mask) & bt["valid"] & bt["label"]
        for k, f in enumerate(FLOWS):
            flow = bt["preds"][k]
            for b in range(flow.shape[0]):
                fms[f].update(points=bt["points"][b], flow_pred=flow[b], flow_gt=bt["gt"][b], is_moving=moving_mask[b], mask=bt["valid"][b])
            try:
                d = M.compute_scene_flow_metrics_for_points_in_this_mask(flow, bt["gt"], np.logical_or(moving_mask, static_mask))
            except ZeroDivisionError:
                d = nan_dict()
            lists[f"{f}/overall"].append(d)
            if np.count_nonzero(moving_mask) > 0:
                lists[f"{f}/moving"].append(M.compute_scene_flow_metrics_for_points_in_this_mask(flow, bt["gt"], moving_mask))
            if np.count_nonzero(static_mask) > 0:
                lists[f"{f}/still"].append(M.compute_scene_flow_metrics_for_points_in_this_mask(flow, bt["gt"], static_mask))
    eval_metrics = {k: M.aggregate_metrics(v) for k, v in lists.items() if len(v)}
    return eval_metrics, fms


def nan_dict():
    nan, nan3 = np.float32(np.nan), np.full(3, np.nan, np.float32)
    return {"ACC3D_0_05": nan, "ACC3D_0_1": nan, "Outliers3D": nan, "RobustOutliers3D": nan, "AEE": nan, "AVG_FLOW_VECTOR": nan3,
            "AVG_FLOW_VECTOR_LENGTH": nan, "AVG_GT_FLOW_VECTOR": nan3, "AVG_GT_FLOW_VECTOR_LENGTH": nan, "AVG_ERROR_FLOW_VECTOR": nan3,
            "num_pts_used": 0, "mean_gt_flow": nan}


def main():
    M = load("liso_ref_slim_metrics", "liso/slim/utils/metrics.py")
    FM = load("liso_ref_flow_metrics", "liso/eval/flow_metrics.py")
    g = np.random.default_rng(20261015)
    cases = {
        "mixed": (None, [dict(B=1, N=1000, edge=True), dict(B=3, N=515), dict(B=1, N=777, nan_padding=True)]),
        "custom_bins": ((0.0, 25.0, 50.0, 75.0, 100.0), [dict(B=3, N=300), dict(B=1, N=1100, edge=True)]),
        "no_moving": (None, [dict(B=1, N=600, no_moving=True), dict(B=2, N=301, no_moving=True, edge=True)]),
        "empty_overall": (None, [dict(B=1, N=500), dict(B=2, N=200, no_label=True), dict(B=1, N=400, edge=True)]),
    }
    out = {"cases": np.array(list(cases))}
    for name, (bins, specs) in cases.items():
        batches = [make_batch(g, **s) for s in specs]
        eval_metrics, fms = run_reference(M, FM, batches, bins)
        out[f"{name}__bins"] = np.linspace(0.0, 100.0, 11) if bins is None else np.array(bins, np.float64)
        out[f"{name}__n"] = np.array(len(batches))
        for i, bt in enumerate(batches):
            for k, v in bt.items():
                out[f"{name}__{i}__{k}"] = v
            out[f"{name}__{i}__epe"] = np.stack([np.linalg.norm(q - bt["gt"], axis=-1) for q in bt["preds"]])
        out[f"{name}__keys"] = np.array(list(eval_metrics))
        for key, d in eval_metrics.items():
            for mk, mv in d.items():
                out[f"{name}__m__{key}__{mk}"] = np.asarray(mv, np.float64)
        for f, fm in fms.items():
            for c in CATS:
                out[f"{name}__fm__{f}__aee_per_range_bin__{c}"] = fm.aee_per_range_bin[c]
                out[f"{name}__fm__{f}__num_points_in_range_bin__{c}"] = fm.num_points_in_range_bin[c]
                out[f"{name}__fm__{f}__total_aees__{c}"] = np.array(fm.total_aees[c], np.float64)
                out[f"{name}__fm__{f}__total_num_pts__{c}"] = np.array(fm.total_num_pts[c], np.int64)
    np.savez_compressed(os.path.join(HERE, "flow_metrics_reference.npz"), **out)
    print("keys per case:", {c: list(out[f"{c}__keys"]) for c in cases})


if __name__ == "__main__":
    main()
