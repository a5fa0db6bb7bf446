"""Shared by the detector-validation tests (test_det_val_host.py, test_gpu_det_val.py): the reference fixture as padded batches, its
assertions (those of test_gpu_od_metrics.py), the edge scenes and the seeded validation set.  Not a test module."""
import numpy as np
import torch

from liso_amd.kabsch.shape_utils import Shape

KEYS = ("pos", "dims", "rot", "probs", "velo", "class_id", "valid")
# tag: criterion, class names, class idxs, BEV area, radial range  (tests/golden/make_od_metrics_golden.py)
CASES = {"bev": ("iou_bev", ("overall",), (0,), None, (None, None)),
         "i3d": ("iou_3d", ("overall", "car", "ped"), (0, 1, 2), (-40.0, -40.0, 40.0, 40.0), (2.0, 50.0))}


def shape_of(d):
    return Shape(**{k: torch.from_numpy(np.ascontiguousarray(d[k])) for k in KEYS})


def fixture_batch(g, tag):
    """all frames of a fixture case as ONE padded batch (host Shapes), its (5, 0) and (0, 7) frames included"""
    n = int(g[f"{tag}_n_samples"])
    side = lambda s: Shape.from_list_of_shapes([shape_of({k: g[f"{tag}_s{i}_{s}_{k}"] for k in KEYS}) for i in range(n)])  # noqa: E731
    return side("gt"), side("pred")


def fixture_validator(tag):
    from liso_amd.eval.det_validation import Collection, DetectionValidator

    crit, names, idxs, bev, (rmin, rmax) = CASES[tag]
    return DetectionValidator([Collection("", "gt", dict(moving_velocity_thresh=0.5, class_names=names, class_idxs=idxs, box_matching_criterion=crit,
                                                         filter_detections_by_bev_area_min_max_m=bev, min_eval_range_m=rmin, max_eval_range_m=rmax))])


def assert_fixture(validator, g, tag):
    """the assertions of tests/test_gpu_od_metrics.py::test_metrics_match_reference_fixture on a validator's single collection"""
    crit, names, _, _, _ = CASES[tag]
    res = validator.compute("val")
    m = validator.metrics[0]
    for cn in names:
        for thr in m.matching_thresholds:
            for cat in m.CATEGORIES:
                key = f"{tag}_{cn}_{thr}_{cat}"
                lab, sc, fn = m.collected(cn, thr, cat)
                assert np.array_equal(lab, g[key + "_labels"]) and np.array_equal(fn, g[key + "_is_fn"]), key
                assert np.array_equal(sc.astype(np.float32), g[key + "_scores"].astype(np.float32)), key
                got, want = res[f"val/{crit}/{cn}/{cat}/AP@{thr:.1f}{crit}"], float(g[key + "_ap"])
                assert (np.isnan(got) and np.isnan(want)) or abs(got - want) <= 1e-9, (key, got, want)
                assert res[f"val/{crit}/{cn}//{cat}/{thr:.1f}{crit}/num_objs"] == int(g[key + "_num_objs"])
            ate, ase, aoe, tps = g[f"{tag}_{cn}_{thr}_tp_errors"]
            e = m.tp_errors[cn][thr]
            assert e["tps"] == int(tps)
            assert abs(e["ATE"] - ate) <= 1e-4 * max(ate, 1) and abs(e["ASE"] - ase) <= 1e-4 * max(ase, 1) and abs(e["AOE"] - aoe) <= 1e-4 * max(aoe, 1)
    assert res[f"val/{crit}/overall/AP@0.5{crit}"] == res[f"val/{crit}/overall/overall/AP@0.5{crit}"] > 0.1


# ---- synthetic scenes -----------------------------------------------------------------------------------------------------------
def scene(g, n_gt, n_pred, n_classes, spread=45.0):
    """ground truth + predictions in the style of the fixture's generator: ~60 % of the predictions are jittered copies of
    ground-truth boxes, the rest clutter"""
    def boxes(n):
        pos = np.concatenate([g.uniform(-spread, spread, (n, 2)), g.uniform(-1.6, -0.4, (n, 1))], -1)
        dims = np.stack([g.uniform(2, 6, n), g.uniform(1, 2.5, n), g.uniform(1.2, 2.2, n)], -1)
        return pos, dims, g.uniform(-np.pi, np.pi, (n, 1))
    gp, gd, gr = boxes(n_gt)
    pp, pd, pr = boxes(n_pred)
    k = min(n_gt, int(0.6 * n_pred))
    sel = g.permutation(n_gt)[:k]
    pp[:k] = gp[sel] + g.normal(0, 0.25, (k, 3))
    pd[:k] = gd[sel] * g.uniform(0.85, 1.15, (k, 3))
    pr[:k] = gr[sel] + g.normal(0, 0.15, (k, 1))
    f = lambda a: a.astype(np.float32)  # noqa: E731
    gt = dict(pos=f(gp), dims=f(gd), rot=f(gr), probs=np.ones((n_gt, 1), np.float32),
              velo=f(g.uniform(0, 2.0, (n_gt, 1)) * (g.uniform(size=(n_gt, 1)) < 0.5)),
              class_id=g.integers(0, n_classes, (n_gt, 1)).astype(np.int64), valid=np.ones(n_gt, bool))
    pred = dict(pos=f(pp), dims=f(pd), rot=f(pr), probs=f(g.uniform(0.05, 1.0, (n_pred, 1))), velo=np.zeros((n_pred, 1), np.float32),
                class_id=g.integers(0, n_classes, (n_pred, 1)).astype(np.int64), valid=np.ones(n_pred, bool))
    return gt, pred


def pad_batch(dicts):
    return Shape.from_list_of_shapes([shape_of(d) for d in dicts])


def punch_holes(shape, g, keep=0.7):
    """holes in the valid mask: a random subset of the valid slots is switched off (the rows keep their values)"""
    shape.valid = shape.valid & torch.from_numpy(g.uniform(size=tuple(shape.valid.shape)) < keep)
    return shape
