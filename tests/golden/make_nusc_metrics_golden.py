"""Generates tests/golden/nusc_metrics.npz: seeded scenes and what the nuScenes devkit's own `accumulate`, `calc_ap`, `calc_tp` and
`DetectionMetrics` (nuscenes/eval/detection/algo.py, data_classes.py of the reference checkout) compute on them, fed as the reference's
NuscenesObjectDetectionMetrics feeds them (liso/eval/nuscenes_metrics_wrapper.py: the radial filter per class, the predictions'
sizes raised to 1e-4, yaw-only rotations, velocity (0, 0), no attributes), as one class and per class.

The devkit package itself cannot be imported here (its __init__ pulls in what is absent): `nuscenes`, `nuscenes.eval` and
`nuscenes.utils` are registered as bare namespace modules over its directories, `nuscenes.utils.data_classes` is mocked and a
stand-in `pyquaternion.Quaternion` gives the one thing the metrics read, `rotation_matrix`.  No text of the devkit is held here.

Scenes: 12 frames, 0..40 ground-truth boxes and 0..130 predictions out to +-55 m, two classes with radii 50 / 40 m; about 70 % of the
predictions are jittered copies of ground-truth boxes, their logits grow with closeness.  Class 1 is drawn so that no prediction of
it lies within 0.5 m of its box and fewer than a tenth of its boxes are found at 2 m: its 0.5 m cell has no match (`no_predictions`)
and its true-positive errors take calc_tp's 1.0 branch; class 0, and the two as one, take the other.

So that the fp32 walk and the devkit's fp64 loop take the same decisions, a draw is kept only if
  * all scores are distinct after the fp32 sigmoid,
  * every member's radial distance is at least 1e-4 m from its radius,
  * every candidate distance is at least 1e-4 m from every threshold,
  * the two nearest candidates of every step of every walk are at least 1e-4 m apart.

Run in the build container only:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_nusc_metrics_golden.py <reference checkout>
"""
import os
import sys
import types
from unittest.mock import MagicMock

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
F, G_MAX, P_MAX = 12, 40, 130
RADII = (50.0, 40.0)
CLASS_NAMES = ("car", "pedestrian")
THS = (0.5, 1.0, 2.0, 4.0)
TP_METRICS = ("trans_err", "scale_err", "orient_err", "vel_err", "attr_err")
MARGIN = 1e-4


def load_devkit(reference_root):
    sdk = os.path.join(reference_root, "nuscenes-devkit", "python-sdk", "nuscenes")
    for name, sub in (("nuscenes", ""), ("nuscenes.eval", "eval"), ("nuscenes.utils", "utils")):
        m = types.ModuleType(name)
        m.__path__ = [os.path.join(sdk, sub)]
        sys.modules[name] = m
    sys.modules["nuscenes.utils.data_classes"] = MagicMock()

    class Quaternion:  # (w, x, y, z), unit length
        def __init__(self, q):
            self.q = np.asarray(q, np.float64)

        @property
        def rotation_matrix(self):
            w, x, y, z = self.q
            return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                             [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                             [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])

    pq = types.ModuleType("pyquaternion")
    pq.Quaternion = Quaternion
    sys.modules["pyquaternion"] = pq
    from nuscenes.eval.common.data_classes import EvalBoxes
    from nuscenes.eval.common.utils import center_distance
    from nuscenes.eval.detection.algo import accumulate, calc_ap, calc_tp
    from nuscenes.eval.detection.data_classes import DetectionBox, DetectionMetrics

    return EvalBoxes, center_distance, accumulate, calc_ap, calc_tp, DetectionBox, DetectionMetrics


def draw(seed):
    """-> dict of padded fp32 / int arrays; slot order is random and the valid masks have holes"""
    g = np.random.default_rng(seed)
    gt, gv, gc = np.zeros((F, G_MAX, 7), np.float32), np.zeros((F, G_MAX), bool), np.zeros((F, G_MAX), np.int32)
    pr, pv, pc = np.zeros((F, P_MAX, 7), np.float32), np.zeros((F, P_MAX), bool), np.zeros((F, P_MAX), np.int32)
    logit = np.zeros((F, P_MAX), np.float32)

    def boxes(n):
        pos = np.concatenate([g.uniform(-55, 55, (n, 2)), g.uniform(-1.6, -0.4, (n, 1))], -1)
        dims = np.stack([g.uniform(0.5, 6, n), g.uniform(0.5, 2.5, n), g.uniform(1.2, 2.2, n)], -1)
        return np.concatenate([pos, dims, g.uniform(-np.pi, np.pi, (n, 1))], -1)

    for f in range(F):
        n_gt = 0 if f == 3 else int(g.integers(20, G_MAX + 1))
        n_pred = 0 if f == 7 else int(g.integers(60, P_MAX + 1))
        gs, ps = np.sort(g.permutation(G_MAX)[:n_gt]), g.permutation(P_MAX)[:n_pred]
        b, cls = boxes(n_gt), (g.uniform(size=n_gt) < 0.35).astype(np.int32)
        gt[f, gs], gv[f, gs], gc[f, gs] = b, True, cls
        q, qc, lg = boxes(n_pred), g.integers(0, 2, n_pred).astype(np.int32), g.normal(-2.0, 1.0, n_pred)
        k = min(n_gt, int(0.7 * n_pred))
        for i, j in enumerate(g.permutation(n_gt)[:k]):
            if cls[j] == 0:
                off = g.normal(0, 0.45, 2)
            elif g.uniform() < 0.04:  # few of class 1, and none within 0.5 m
                ang, rad = g.uniform(0, 2 * np.pi), g.uniform(0.6, 1.8)
                off = rad * np.array([np.cos(ang), np.sin(ang)])
            else:
                off = g.uniform(6, 9) * np.array([1.0, 0.0])  # a copy far off: clutter of class 1
            q[i, :2] = b[j, :2] + off
            q[i, 2] = b[j, 2] + g.normal(0, 0.1)
            q[i, 3:6] = b[j, 3:6] * g.uniform(0.8, 1.25, 3)
            q[i, 6] = b[j, 6] + g.normal(0, 0.2)
            qc[i] = cls[j] if g.uniform() < 0.9 else 1 - cls[j]
            lg[i] = 3.0 - 4.0 * np.linalg.norm(off) + g.normal(0, 0.7)
        if n_pred > 2:
            q[1, 3] = 0.0  # a prediction of size 0: the wrapper raises it to 1e-4
        pr[f, ps], pv[f, ps], pc[f, ps], logit[f, ps] = q, True, qc, lg
    return dict(gt=gt, gt_valid=gv, gt_class=gc, pred=pr, pred_valid=pv, pred_class=pc, logit=logit)


def members(rows, valid, cls, as_one):
    r = np.linalg.norm(rows[..., :2].astype(np.float64), axis=-1)
    rad = np.full(r.shape, RADII[0]) if as_one else np.asarray(RADII)[cls]
    return valid & (r <= rad), float(np.abs(r - rad)[valid].min()) if valid.any() else np.inf


def margins_ok(s, score):
    """the docstring's conditions, for both modes; fp64 walks of this file's own"""
    flat = score[s["pred_valid"]]
    if len(np.unique(flat)) != len(flat):
        return False
    for as_one in (True, False):
        g_in, mg = members(s["gt"], s["gt_valid"], s["gt_class"], as_one)
        p_in, mp = members(s["pred"], s["pred_valid"], s["pred_class"], as_one)
        if min(mg, mp) < MARGIN:
            return False
        for f in range(F):
            gi, pi = np.flatnonzero(g_in[f]), np.flatnonzero(p_in[f])
            if not len(gi) or not len(pi):
                continue
            d = np.linalg.norm(s["gt"][f][gi][:, None, :2].astype(np.float64) - s["pred"][f][pi][None, :, :2].astype(np.float64), axis=-1)
            same = np.ones_like(d, bool) if as_one else s["gt_class"][f, gi][:, None] == s["pred_class"][f, pi][None, :]
            if any(np.abs(d[same] - t).min(initial=np.inf) < MARGIN for t in THS):
                return False
            visit = np.argsort(-score[f, pi].astype(np.float64), kind="stable")
            for t in THS:
                free = np.ones(len(gi), bool)
                for j in visit:
                    c = np.flatnonzero(free & same[:, j])
                    if not len(c):
                        continue
                    dd = np.sort(d[c, j])
                    if len(dd) > 1 and dd[1] - dd[0] < MARGIN:
                        return False
                    if dd[0] < t:
                        free[c[np.argmin(d[c, j])]] = False
    return True


def devkit_results(dk, s, score, as_one):
    EvalBoxes, center_distance, accumulate, calc_ap, calc_tp, DetectionBox, DetectionMetrics = dk
    names = ("movable",) if as_one else CLASS_NAMES
    g_in, _ = members(s["gt"], s["gt_valid"], s["gt_class"], as_one)
    p_in, _ = members(s["pred"], s["pred_valid"], s["pred_class"], as_one)
    gt_boxes, pred_boxes = EvalBoxes(), EvalBoxes()

    def box(row, name, token, **kw):
        yaw = float(row[6])
        return DetectionBox(sample_token=token, translation=tuple(float(v) for v in row[:3]), size=tuple(float(v) for v in row[3:6]),
                            rotation=(np.cos(yaw / 2), 0.0, 0.0, np.sin(yaw / 2)), velocity=(0, 0), ego_translation=(0, 0, 0),
                            detection_name=name, num_pts=-1, **kw)

    for f in range(F):
        token = f"frame{f}"
        gt_boxes.add_boxes(token, [box(s["gt"][f, i], names[0 if as_one else s["gt_class"][f, i]], token) for i in np.flatnonzero(g_in[f])])
        rows = s["pred"][f].copy()
        rows[:, 3:6] = np.maximum(rows[:, 3:6], np.float32(1e-4))
        pred_boxes.add_boxes(token, [box(rows[i], names[0 if as_one else s["pred_class"][f, i]], token, detection_score=float(score[f, i]))
                                     for i in np.flatnonzero(p_in[f])])
    cfg = types.SimpleNamespace(class_names=list(names), mean_ap_weight=5, dist_ths=list(THS), dist_th_tp=2.0, min_recall=0.1, min_precision=0.1)
    metrics = DetectionMetrics(cfg)
    md = {(n, t): accumulate(gt_boxes, pred_boxes, n, center_distance, t, {}) for n in names for t in THS}
    for n in names:
        for t in THS:
            metrics.add_label_ap(n, t, calc_ap(md[(n, t)], cfg.min_recall, cfg.min_precision))
        for k in TP_METRICS:
            metrics.add_label_tp(n, k, calc_tp(md[(n, cfg.dist_th_tp)], cfg.min_recall, k))
    curves = np.stack([[np.asarray(getattr(md[(n, 2.0)], k), np.float64) for k in ("recall", "precision", "confidence") + TP_METRICS] for n in names])
    matches = np.array([[int(np.count_nonzero(md[(n, t)].confidence)) for t in THS] for n in names])
    return dict(ap=np.array([[metrics.get_label_ap(n, t) for t in THS] for n in names]),
                tp=np.array([[metrics.get_label_tp(n, k) for k in TP_METRICS] for n in names]), mean_ap=np.float64(metrics.mean_ap),
                tp_errors=np.array([metrics.tp_errors[k] for k in TP_METRICS]), nd_score=np.float64(metrics.nd_score), curves=curves,
                max_recall_ind=np.array([md[(n, 2.0)].max_recall_ind for n in names]), nonzero_conf=matches)


def main():
    dk = load_devkit(sys.argv[1] if len(sys.argv) > 1 else os.environ["LISO_REFERENCE"])
    for seed in range(100, 400):
        s = draw(seed)
        score = torch.sigmoid(torch.from_numpy(s["logit"])).numpy()  # fp32, as the collection with sigmoid_scores=True sees them
        if margins_ok(s, score):
            break
    else:
        raise SystemExit("no seed meets the margins")
    out = dict(seed=np.int64(seed), radii=np.asarray(RADII, np.float32), class_names=np.array(CLASS_NAMES), thresholds=np.asarray(THS), **s)
    for tag, as_one in (("one", True), ("cls", False)):
        r = devkit_results(dk, s, score, as_one)
        out.update({f"{tag}_{k}": v for k, v in r.items()})
    one, cls = out["one_max_recall_ind"], out["cls_max_recall_ind"]
    assert one[0] >= 11 and cls[0] >= 11 and cls[1] < 11, (one, cls)  # both branches of calc_tp
    assert out["cls_nonzero_conf"][1, 0] == 0 and out["cls_ap"][1, 0] == 0.0 and out["cls_nonzero_conf"][1, 2] > 0, out["cls_nonzero_conf"]
    assert out["one_mean_ap"] > 0.2 and out["cls_ap"][0].min() > 0.2, (out["one_mean_ap"], out["cls_ap"])
    assert np.all(out["cls_tp"][1, :3] == 1.0) and np.all(out["one_tp"][0, :3] < 1.0)
    np.savez_compressed(os.path.join(HERE, "nusc_metrics.npz"), **out)
    print("seed", seed, "mAP one", float(out["one_mean_ap"]), "NDS", float(out["one_nd_score"]), "per class AP", out["cls_ap"].tolist(),
          "tp", out["cls_tp"].tolist(), os.path.getsize(os.path.join(HERE, "nusc_metrics.npz")), "bytes")


if __name__ == "__main__":
    main()
