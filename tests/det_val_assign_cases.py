"""Shared by the optimal-assignment tests of the detector validation (test_det_val_assign_host.py, test_det_val_assign_abi.py,
test_gpu_det_val_assign.py): the Waymo fixture as Shapes, scenes with a `difficulty` column, the per-frame reference loop and the
comparison of two sets of Waymo-style collections.  Not a test module."""
import numpy as np
import torch

from liso_amd.kabsch.shape_utils import Shape

KEYS = ("pos", "dims", "rot", "probs", "velo", "class_id", "difficulty", "valid")
# tag: constructor arguments (tests/golden/make_waymo_metrics_golden.py)
CASES = {"bin": dict(min_eval_range_m=0.0, max_eval_range_m=20.0),
         "cls": dict(eval_movable_classes_as_one=False, class_names=("car", "ped", "cyc"), class_idxs=(0, 1, 2))}


def shape_of(d):
    return Shape(**{k: torch.from_numpy(np.ascontiguousarray(d[k])) for k in KEYS})


def with_difficulty(g, gt, pred):
    """adds the `difficulty` column to a scene of tests/det_val_cases.py: 0 and > 0 mixed on the ground truth"""
    n_gt, n_pred = len(gt["valid"]), len(pred["valid"])
    gt["difficulty"] = (g.integers(0, 3, (n_gt, 1)) * (g.uniform(size=(n_gt, 1)) < 0.6)).astype(np.int32)
    pred["difficulty"] = np.zeros((n_pred, 1), np.int32)
    return gt, pred


def pad_batch(dicts):
    return Shape.from_list_of_shapes([shape_of(d) for d in dicts])


def fixture_frames(g, tag):
    n = int(g[f"{tag}_n_samples"])
    side = lambda s: [shape_of({k: g[f"{tag}_s{i}_{s}_{k}"] for k in KEYS}) for i in range(n)]  # noqa: E731
    return side("gt"), side("pred")


def host_box_iou_matrix(gt, pred, mode):
    """`box_iou_matrix` from the library's host twin of the pair kernel (no GPU): unbatched Shapes -> torch fp32 [n_gt, n_pred]"""
    from liso_amd.eval.det_validation import host_pair_matrices, pack_boxes

    g, p = pack_boxes(Shape.from_list_of_shapes([gt])), pack_boxes(Shape.from_list_of_shapes([pred]))
    mats = host_pair_matrices(g["rows"].numpy(), g["valid"].numpy(), p["rows"].numpy(), p["valid"].numpy())
    return torch.from_numpy(np.ascontiguousarray(mats[mode][0].T))


def assert_same_waymo_collections(a, b, what=""):
    """two WaymoObjectDetectionMetrics: equal collected lists, every AP within 1e-9, precision / recall exactly equal"""
    assert a.class_names == b.class_names
    n = 0
    for cn in a.class_names:
        for crit in a.CRITERIA:
            for cat in a.CATEGORIES:
                for x, y in zip(a.collected(cn, crit, cat), b.collected(cn, crit, cat)):
                    assert x.dtype == y.dtype and np.array_equal(x, y), (what, cn, crit, cat)
                n += 1
    ra, rb = a.compute("p/"), b.compute("p/")
    assert set(ra) == set(rb) and len(ra) >= 3 * n // 2
    for k, w in rb.items():
        if "AP@" in k:
            assert (np.isnan(ra[k]) and np.isnan(w)) or abs(ra[k] - w) <= 1e-9, (what, k, ra[k], w)
        else:
            assert ra[k] == w or (np.isnan(ra[k]) and np.isnan(w)), (what, k, ra[k], w)
    return n


def _quad(b):
    c, s = np.cos(b[6]), np.sin(b[6])
    return np.array([[b[0] + sx * b[3] / 2 * c - sy * b[4] / 2 * s, b[1] + sx * b[3] / 2 * s + sy * b[4] / 2 * c]
                     for sx, sy in ((-1, -1), (1, -1), (1, 1), (-1, 1))])


def _overlap64(a, b):
    """area of the intersection of two rotated rectangles in fp64 (Sutherland-Hodgman)"""
    poly, clip = _quad(a), _quad(b)
    for i in range(4):
        p0, p1 = clip[i], clip[(i + 1) % 4]
        side = lambda q: (p1[0] - p0[0]) * (q[1] - p0[1]) - (p1[1] - p0[1]) * (q[0] - p0[0])  # noqa: E731
        out = []
        for k in range(len(poly)):
            q0, q1 = poly[k], poly[(k + 1) % len(poly)]
            s0, s1 = side(q0), side(q1)
            if s0 >= 0:
                out.append(q0)
            if (s0 > 0 > s1) or (s0 < 0 < s1):
                out.append(q0 + (q1 - q0) * (s0 / (s0 - s1)))
        poly = out
        if len(poly) < 3:
            return 0.0
    x, y = np.array(poly).T
    return 0.5 * abs(np.dot(x, np.roll(y, -1)) - np.dot(y, np.roll(x, -1)))


def assert_no_iou_on_the_assignment_edge(gts, preds):
    """in fp64: no BEV or 3-D IoU of any pair within 1e-4 of the Waymo-style collections' 0.4, no radius within 1e-3 m of a range-bin
    edge and no coordinate within 1e-3 m of the (+-50, +-20) area's bounds"""
    rows = lambda d: np.concatenate([d["pos"], d["dims"], d["rot"]], -1).astype(np.float64)  # noqa: E731
    for f in range(len(preds)):
        p, g = rows(preds[f]), rows(gts[f])
        for boxes in (g, p):
            r = np.hypot(boxes[:, 0], boxes[:, 1])
            assert (np.abs(r[:, None] - np.array([20.0, 40.0, 60.0, 1000.0])) > 1e-3).all() and (r > 1e-3).all(), f
            assert (np.abs(np.abs(boxes[:, 0]) - 50.0) > 1e-3).all() and (np.abs(np.abs(boxes[:, 1]) - 20.0) > 1e-3).all(), f
        for a in g:
            d = np.hypot(p[:, 0] - a[0], p[:, 1] - a[1])
            for b in p[d < 12.0]:
                ov = _overlap64(a, b)
                if ov == 0.0:
                    continue
                bev = ov / (a[3] * a[4] + b[3] * b[4] - ov)
                h = min(a[2] + a[5] / 2, b[2] + b[5] / 2) - max(a[2] - a[5] / 2, b[2] - b[5] / 2)
                inter = ov * h if h > 0 else 0.0
                i3d = inter / (a[3] * a[4] * a[5] + b[3] * b[4] * b[5] - inter)
                assert abs(bev - 0.4) > 1e-4 and abs(i3d - 0.4) > 1e-4, (f, bev, i3d)
