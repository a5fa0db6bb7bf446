"""Shared by the nuScenes-metrics tests (test_nusc_metrics_host.py, test_gpu_nusc_metrics.py): the devkit fixture as a padded batch and
its assertions, and seeded batches for the kernel's edges.  Not a test module."""
import numpy as np
import torch

from liso_amd.kabsch.shape_utils import Shape

TP_METRICS = ("trans_err", "scale_err", "orient_err", "vel_err", "attr_err")
CURVES = ("recall", "precision", "confidence") + TP_METRICS
# Every error term is a few fp32 roundings of a value <= 4: <= 16 * 2^-24 * 4 ~ 4e-6; cummean and interp are convex combinations.
TP_TOL = 1e-5


def fixture_shapes(g):
    """the fixture's 12 frames as one padded batch (host Shapes [12,40] / [12,130]); the predictions carry the raw logits"""
    t = torch.from_numpy

    def shape(rows, valid, cls, probs):
        rows = t(rows)
        return Shape(pos=rows[..., :3].contiguous(), dims=rows[..., 3:6].contiguous(), rot=rows[..., 6:7].contiguous(), probs=probs[..., None],
                     velo=torch.zeros(rows.shape[:2] + (1,)), class_id=t(cls.astype(np.int64))[..., None], valid=t(valid))
    return (shape(g["gt"], g["gt_valid"], g["gt_class"], torch.ones(g["gt_valid"].shape)),
            shape(g["pred"], g["pred_valid"], g["pred_class"], t(g["logit"])))


def fixture_metric(g, as_one):
    from liso_amd.eval.nuscenes_metrics import NuscenesObjectDetectionMetrics

    if as_one:
        return NuscenesObjectDetectionMetrics(eval_movable_classes_as_one=True, sigmoid_scores=True)
    names = tuple(str(n) for n in g["class_names"])
    return NuscenesObjectDetectionMetrics(eval_movable_classes_as_one=False, class_names=names, sigmoid_scores=True,
                                          class_ranges={n: float(r) for n, r in zip(names, g["radii"])})


def assert_fixture(metric, g, as_one):
    """every AP, mean_ap and the precision / recall / confidence arrays exactly; every TP error and NDS within TP_TOL"""
    tag = "one" if as_one else "cls"
    r = metric.evaluate()
    names = metric.target_class_names
    assert names == (["movable"] if as_one else [str(n) for n in g["class_names"]])
    for c, name in enumerate(names):
        for t, thr in enumerate(metric.matching_thresholds):
            assert r["label_aps"][name][thr] == g[f"{tag}_ap"][c, t], (name, thr, r["label_aps"][name][thr], g[f"{tag}_ap"][c, t])
        md = r["metric_data"][(name, 2.0)]
        for k, key in enumerate(CURVES):
            want = g[f"{tag}_curves"][c, k]
            if k < 3:
                assert np.array_equal(md[key], want), (name, key)
            else:
                assert np.abs(md[key] - want).max() <= TP_TOL, (name, key, np.abs(md[key] - want).max())
        for k, key in enumerate(TP_METRICS):
            assert abs(r["label_tp_errors"][name][key] - g[f"{tag}_tp"][c, k]) <= TP_TOL, (name, key)
    assert r["mean_ap"] == float(g[f"{tag}_mean_ap"])
    assert np.abs(np.array([r["tp_errors"][k] for k in TP_METRICS]) - g[f"{tag}_tp_errors"]).max() <= TP_TOL
    assert abs(r["nd_score"] - float(g[f"{tag}_nd_score"])) <= TP_TOL
    return r


# ---- seeded batches for the kernel ------------------------------------------------------------------------------------------------
def kernel_batch(seed, F, G, P, n_classes=3, keep=0.8):
    """packed arrays of F frames: boxes out to +-45 m (radii 40 / 30 / 20 m cut some), ~60 % of the predictions near a ground-truth
    box, holes in both masks, a class id out of range and NaN rows in both sets when there is room
    -> dict(gt rows, gv, gc, pred rows, pv, pc, score, radius)"""
    g = np.random.default_rng(seed)

    def rows(n):
        pos = np.concatenate([g.uniform(-45, 45, (F, n, 2)), g.uniform(-1.6, -0.4, (F, n, 1))], -1)
        dims = np.stack([g.uniform(0.5, 6, (F, n)), g.uniform(0.5, 2.5, (F, n)), g.uniform(1.2, 2.2, (F, n))], -1)
        return np.concatenate([pos, dims, g.uniform(-4, 4, (F, n, 1))], -1).astype(np.float32)
    gt, pred = rows(G), rows(P)
    gc, pc = g.integers(0, n_classes, (F, G)).astype(np.int32), g.integers(0, n_classes, (F, P)).astype(np.int32)
    k = min(G, int(0.6 * P))
    for f in range(F):
        sel = g.permutation(G)[:k]
        pred[f, :k, :2] = gt[f, sel, :2] + g.normal(0, 0.8, (k, 2)).astype(np.float32)
        pred[f, :k, 3:6] = gt[f, sel, 3:6] * g.uniform(0.8, 1.25, (k, 3)).astype(np.float32)
        pc[f, :k] = np.where(g.uniform(size=k) < 0.85, gc[f, sel], pc[f, :k])
        perm = g.permutation(P)
        pred[f], pc[f] = pred[f, perm], pc[f, perm]
    gv, pv = g.uniform(size=(F, G)) < keep, g.uniform(size=(F, P)) < keep
    if G > 4:
        gt[0, 1, 0], gv[0, 1] = np.nan, True  # NaN centre: never a member
        gc[0, 2], gv[0, 2] = n_classes, True  # class out of range
        gt[0, 3, 3], gv[0, 3] = np.nan, True  # NaN size: a member; its scale term is NaN when matched
    if P > 4:
        pred[0, 1, 1], pv[0, 1] = np.nan, True
        pc[0, 2], pv[0, 2] = -1, True
        pred[0, 3, 4], pv[0, 3] = 0.0, True  # size 0: raised to 1e-4
    score = g.uniform(0.02, 0.98, (F, P)).astype(np.float32)
    score[:, ::7] = np.float32(0.5)  # equal scores: ascending slot
    return dict(gt=gt, gv=gv.astype(np.uint8), gc=gc, pred=pred, pv=pv.astype(np.uint8), pc=pc, score=score,
                radius=np.array([40.0, 30.0, 20.0][:n_classes], np.float32))


def kernel_host(b, as_one, thresholds=(0.5, 1.0, 2.0, 4.0)):
    from liso_amd.eval.det_validation import stable_order_host
    from liso_amd.eval.nuscenes_metrics import nusc_match_host

    order = stable_order_host(b["score"], b["pv"])
    return order, nusc_match_host(b["gt"], b["gv"], b["gc"], b["pred"], b["pv"], b["pc"], order, b["radius"], as_one, thresholds)
