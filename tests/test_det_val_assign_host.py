"""CPU: the optimal assignment of the detector validation, stated in numpy (liso_amd/eval/det_validation.py::assign_host), against
the reference's fixture and scipy; the host `WaymoObjectDetectionMetrics` against its reference fixture; and the validator's host
path with Waymo-style collections against the per-frame `update` loop.  Pair matrices: the library's host twin of the pair kernel.

Totals are compared within 1e-9: an assignment's total is a sum of at most 130 values of magnitude <= 1, the solver performs fewer
than 2^20 fp64 roundings of at most 2^-53 each on such values, far below fp32's spacing at 0.4 (3e-8)."""
import numpy as np
import pytest
import torch

from tests.det_val_assign_cases import (CASES, assert_same_waymo_collections, fixture_frames, host_box_iou_matrix, pad_batch,
                                        with_difficulty)
from tests.det_val_cases import scene

HUNGARIAN_CASES = ("h0", "h1", "h2", "h3", "h4", "h5", "h6")
SIDES = (1, 2, 63, 64, 65, 130)


def _all(iou):
    return np.ones(iou.shape[0], bool), np.ones(iou.shape[1], bool)


def _value(iou):
    return np.where(np.isfinite(iou), iou, -1.0).astype(np.float64)


def _assignment_total(iou):
    """the optimal total of the smaller side's assignment, from scipy (rectangular: every member of the smaller side is assigned)"""
    from scipy.optimize import linear_sum_assignment

    r, c = linear_sum_assignment(_value(iou), maximize=True)
    return _value(iou)[r, c].sum()


@pytest.mark.parametrize("thr", [0.3, 0.5])
@pytest.mark.parametrize("tag", HUNGARIAN_CASES)
def test_restatement_reproduces_the_reference_fixture(golden_dir, tag, thr):
    from liso_amd.eval.det_validation import assign_host

    g = np.load(f"{golden_dir}/matching_hungarian_reference.npz")
    iou = g[f"{tag}_iou"]  # [n_gt, n_pred], NaN / inf entries included
    got = assign_host(iou.T, *_all(iou), thr)
    want = sorted(zip(g[f"{tag}_{thr}_idx_gt"].tolist(), g[f"{tag}_{thr}_idx_pred"].tolist()))
    assert got == want
    gm, pm = np.zeros(iou.shape[0], bool), np.zeros(iou.shape[1], bool)
    gm[[a for a, _ in got]], pm[[b for _, b in got]] = True, True
    assert np.array_equal(gm, g[f"{tag}_{thr}_gt_mask"]) and np.array_equal(pm, g[f"{tag}_{thr}_pred_mask"])


def _assigned_all(iou):
    """every assigned pair of the restatement (threshold below every value)"""
    from liso_amd.eval.det_validation import assign_host

    return assign_host(iou.T, *_all(iou), -2.0)


@pytest.mark.parametrize("small", SIDES)
def test_restatement_agrees_with_scipy_on_seeded_matrices(small):
    from liso_amd.eval.det_validation import assign_host
    from liso_amd.kabsch.box_groundtruth_matching_iou import hungarian_match_iou_matrix

    rng = np.random.default_rng(100 + small)
    n_cases = 0
    for large in SIDES:
        if large < small:
            continue
        for n_gt, n_pred in {(small, large), (large, small)}:
            sparsity = rng.uniform(0.5, 0.95)
            iou = rng.uniform(0.0, 1.0, (n_gt, n_pred)).astype(np.float32)
            iou[rng.uniform(size=iou.shape) < sparsity] = 0.0
            got = assign_host(iou.T, *_all(iou), 0.4)
            ig, ip, _, _, _ = hungarian_match_iou_matrix(iou, 0.4)
            assert got == sorted(zip(ig.tolist(), ip.tolist())), (n_gt, n_pred)
            every = _assigned_all(iou)
            assert len(every) == min(n_gt, n_pred)
            total = sum(float(iou[a, b]) for a, b in every)
            assert abs(total - _assignment_total(iou)) <= 1e-9, (n_gt, n_pred)
            n_cases += 1
    assert n_cases >= 1


def test_ties_valid_optimal_and_by_the_documented_rule():
    """duplicate boxes / equal IoUs: scipy may take another of the equally good assignments; what is checked is validity, the optimal
    total, and the rule: rows in ascending order, each taking the lowest column position among equal reduced distances"""
    from liso_amd.eval.det_validation import assign_host

    # three identical ground-truth boxes, five predictions of which 1, 3, 4 are copies of them: every 3 x 3 sub-assignment is optimal
    iou = np.zeros((3, 5), np.float32)
    iou[:, [1, 3, 4]] = 0.75
    got = assign_host(iou.T, *_all(iou), 0.4)
    assert got == [(0, 1), (1, 3), (2, 4)]  # row 0 first, lowest position; the later rows never push it away at equal cost
    # more ground truth than predictions: the predictions are the rows, the ground truth the columns
    got_t = assign_host(iou, np.ones(5, bool), np.ones(3, bool), 0.4)
    assert got_t == [(1, 0), (3, 1), (4, 2)]
    # equal sizes: the ground truth takes the rows; all values equal
    eq = np.full((4, 4), 0.5, np.float32)
    assert assign_host(eq.T, *_all(eq), 0.4) == [(0, 0), (1, 1), (2, 2), (3, 3)]
    # a tie that must be broken against the first choice: row 0 takes column 0 first, row 1 only fits column 0 -> row 0 moves on
    tie = np.float32([[0.6, 0.6, 0.0], [0.6, 0.0, 0.0]])
    assert assign_host(tie.T, *_all(tie), 0.4) == [(0, 1), (1, 0)]
    rng = np.random.default_rng(3)
    for n_gt, n_pred in ((7, 12), (12, 7), (9, 9)):
        m = np.round(rng.uniform(0, 1, (n_gt, n_pred)), 1).astype(np.float32)  # eleven distinct values: ties everywhere
        m[rng.uniform(size=m.shape) < 0.5] = 0.0
        pairs = assign_host(m.T, *_all(m), -2.0)
        gs, ps = [a for a, _ in pairs], [b for _, b in pairs]
        assert len(pairs) == min(n_gt, n_pred) and len(set(gs)) == len(gs) and len(set(ps)) == len(ps)
        assert all(0 <= a < n_gt and 0 <= b < n_pred for a, b in pairs) and gs == sorted(gs)
        assert abs(sum(float(m[a, b]) for a, b in pairs) - _assignment_total(m)) <= 1e-9
    # masks: only members take part, and an empty side matches nothing
    g_in, p_in = np.array([0, 1, 1], bool), np.array([1, 0, 0, 1, 1], bool)
    assert assign_host(iou.T, g_in, p_in, 0.4) == [(1, 3), (2, 4)]
    assert assign_host(iou.T, np.zeros(3, bool), p_in, 0.4) == [] and assign_host(iou.T, g_in, np.zeros(5, bool), 0.4) == []


@pytest.fixture()
def host_iou(monkeypatch):
    """the per-frame path's IoU matrices from the library's host twin instead of the device kernels"""
    import liso_amd.kabsch.box_groundtruth_matching_iou as M

    monkeypatch.setattr(M, "box_iou_matrix", host_box_iou_matrix)


@pytest.mark.parametrize("tag", sorted(CASES))
def test_host_waymo_metrics_reproduce_the_reference_fixture(golden_dir, host_iou, tag):
    from liso_amd.eval.od_metrics import WaymoObjectDetectionMetrics

    g = np.load(f"{golden_dir}/waymo_metrics_reference.npz")
    gts, preds = fixture_frames(g, tag)
    sizes = [(len(a.valid), len(b.valid)) for a, b in zip(gts, preds)]
    assert len(sizes) >= 5 and any(p == 0 < n for n, p in sizes) and any(n == 0 < p for n, p in sizes) and any(n > p > 0 for n, p in sizes)
    assert any(int((a.difficulty > 0).sum()) > 0 for a in gts) and any(int((a.difficulty == 0).sum()) > 0 for a in gts)
    m = WaymoObjectDetectionMetrics(**CASES[tag])
    for gt, pred in zip(gts, preds):
        m.update(non_batched_gt_boxes=gt, non_batched_pred_boxes=pred, sample_token="")
    for cn in m.class_names:
        for crit in m.CRITERIA:
            for cat in m.CATEGORIES:
                key = f"{tag}_{cn}_{crit}_{cat}"
                lab, sc, fn = m.collected(cn, crit, cat)
                assert np.array_equal(lab, g[key + "_labels"]) and np.array_equal(fn, g[key + "_is_fn"]), key
                assert np.array_equal(sc, g[key + "_scores"]), key
    res = m.compute(f"val/{tag}")
    want = dict(zip(g[f"{tag}_metric_keys"].tolist(), g[f"{tag}_metric_values"].tolist()))
    assert set(res) == set(want) and len(want) == 10 * len(m.class_names) * 2
    for k, w in want.items():
        if "AP@" in k:
            assert abs(res[k] - w) <= 1e-9, (k, res[k], w)
        else:
            assert res[k] == w, (k, res[k], w)
    assert max(w for k, w in want.items() if "AP@" in k) > 0.04


def test_host_validator_with_waymo_collections_equals_the_per_frame_loop(host_iou):
    from liso_amd.eval.det_validation import Collection, DetectionValidator
    from liso_amd.eval.od_metrics import WaymoObjectDetectionMetrics
    from tests.det_val_assign_cases import shape_of

    g = np.random.default_rng(31)
    frames = [with_difficulty(g, *scene(g, n_gt, n_pred, 3, spread=30.0)) for n_gt, n_pred in ((40, 60), (50, 30), (7, 0), (0, 9), (33, 33))]
    kws = [dict(min_eval_range_m=0.0, max_eval_range_m=20.0), dict(min_eval_range_m=20.0, max_eval_range_m=40.0),
           dict(eval_movable_classes_as_one=False, class_names=("car", "ped", "cyc"), class_idxs=(0, 1, 2))]
    v = DetectionValidator([Collection(f"c{i}/", "benchmark" if i == 1 else "gt", kw, "waymo") for i, kw in enumerate(kws)])
    assert [len(t.jobs) for t in v.tables.values()] == [0, 0] and len(v.assign_tables["gt"].jobs) == 2 + 6 and len(v.assign_tables["benchmark"].jobs) == 2
    gt, pred = pad_batch([f[0] for f in frames]), pad_batch([f[1] for f in frames])
    v.update_batch_host(gt, gt, pred)
    got = v.compute("val/")
    ref = [WaymoObjectDetectionMetrics(**kw) for kw in kws]
    for f_gt, f_pred in frames:
        for m in ref:
            m.update(non_batched_gt_boxes=shape_of(f_gt), non_batched_pred_boxes=shape_of(f_pred))
    want = {}
    for i, (m, mine) in enumerate(zip(ref, v.metrics)):
        assert assert_same_waymo_collections(mine, m, f"collection {i}") == len(m.class_names) * 4
        want.update(m.compute(f"val/c{i}/"))
    assert got == want and "val/c0/iou_bev/overall/L1/AP@0.4" in got and got["val/c0/iou_bev/overall/L2/AP@0.4"] > 0.1
    assert torch.is_tensor(gt.difficulty) and int((gt.difficulty[gt.valid] > 0).sum()) > 10
