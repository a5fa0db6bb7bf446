"""Generates tests/golden/waymo_metrics_reference.npz from the reference's own liso/eval/od_metrics.py:
  WaymoObjectDetectionMetrics(...).update(...)  (:1459-1664)  and  .log(...)  (:1666-1807)
on a few synthetic validation samples: the scenes of make_od_metrics_golden.py's generator with a `difficulty` column (0 and > 0
mixed).  Matching runs through the reference's `match_boxes_by_descending_confidence_iou(matching_mode="hungarian")` ->
`box_iou_matrix` -> iou3d_nms_utils with the native module replaced as in make_nms_iou_golden.py (numbers from oracle/_ref = the
reference's iou3d_cpu.cpp compiled where it lies) -> scipy's linear_sum_assignment.  Stored: the inputs, the collected label /
score / is_fn lists per (class, criterion, category), and every entry of the dictionary `log()` returns.
Run in the build container only:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_waymo_metrics_golden.py
"""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_nms_iou_golden import _cpu_cuda, install_native_stub  # noqa: E402
from make_od_metrics_golden import scene  # noqa: E402
from make_targets_golden import _Anything, import_with_stubs  # noqa: E402

sys.modules["torch.utils.tensorboard"] = _Anything("torch.utils.tensorboard")

# tag: (constructor arguments, samples [(n_gt, n_pred)], seed)
CASES = {
    "bin": (dict(min_eval_range_m=0.0, max_eval_range_m=20.0), [(60, 90), (80, 40), (40, 0), (0, 30), (70, 100), (25, 25)], 11),
    "cls": (dict(eval_movable_classes_as_one=False, class_names=("car", "ped", "cyc"), class_idxs=(0, 1, 2)),
            [(90, 140), (120, 66), (18, 0), (0, 24), (100, 160)], 12),
}


class _Writer:
    """`log()` calls its writer unconditionally (:1833); nothing is written"""

    def add_scalar(self, *a, **k):
        pass

    add_image = flush = add_scalar


def main():
    install_native_stub()

    def _imp():
        import liso.eval.od_metrics as odm
        from liso.kabsch.shape_utils import Shape
        return odm, Shape

    odm, Shape = import_with_stubs(_imp)
    odm.plot_to_np_image = lambda fig: None  # (the figure is not part of the numbers)
    S = lambda d: Shape(**{k: torch.from_numpy(v) for k, v in d.items()})  # noqa: E731
    out = {}
    with _cpu_cuda(), torch.no_grad():
        for tag, (kwargs, samples, seed) in CASES.items():
            g = np.random.default_rng(seed)
            m = odm.WaymoObjectDetectionMetrics(**kwargs)
            out[f"{tag}_n_samples"] = np.array(len(samples))
            for i, (n_gt, n_pred) in enumerate(samples):
                gt, pred = scene(g, n_gt, n_pred, 3)
                gt["difficulty"] = (g.integers(0, 3, (n_gt, 1)) * (g.uniform(size=(n_gt, 1)) < 0.6)).astype(np.int32)
                pred["difficulty"] = np.zeros((n_pred, 1), np.int32)
                for k, v in gt.items():
                    out[f"{tag}_s{i}_gt_{k}"] = v
                for k, v in pred.items():
                    out[f"{tag}_s{i}_pred_{k}"] = v
                m.update(non_batched_gt_boxes=S(gt), non_batched_pred_boxes=S(pred), sample_token=str(i))
            for cn in m.class_names:
                for crit in m.box_matching_criterions:
                    for cat in m.extra_categories:
                        key = f"{tag}_{cn}_{crit}_{cat}"
                        out[key + "_labels"] = np.concatenate(m.per_class_per_crit_per_category_gt_labels[cn][crit][cat]).astype(bool)
                        out[key + "_scores"] = np.concatenate(m.per_class_per_crit_per_category_scores[cn][crit][cat]).astype(np.float64)
                        out[key + "_is_fn"] = np.concatenate(m.per_class_per_crit_per_category_is_fn[cn][crit][cat]).astype(bool)
            metrics = m.log(0, summary_writer=_Writer(), writer_prefix=f"val/{tag}")
            keys = sorted(metrics)
            out[f"{tag}_metric_keys"] = np.array(keys)
            out[f"{tag}_metric_values"] = np.array([float(metrics[k]) for k in keys], np.float64)
            print(tag, len(keys), "metrics;", {k: round(float(metrics[k]), 4) for k in keys if k.endswith("AP@0.4")})
    dst = os.path.join(HERE, "waymo_metrics_reference.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, len(out), "arrays,", os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
