"""CPU: the nuScenes detection metrics on the host (liso_amd/eval/nuscenes_metrics.py) -- the numpy restatement of the walk plus
`evaluate()` against what the devkit computes on the fixture (tests/golden/make_nusc_metrics_golden.py), the per-frame `update()`
path against the batched one, hand-made edges of the walk, and run_val's collection sets with the flag off and on."""
import numpy as np
import pytest
import torch

from tests.nusc_metrics_cases import assert_fixture, fixture_metric, fixture_shapes

F32 = np.float32


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(f"{golden_dir}/nusc_metrics.npz")


def _validator(metric_kwargs):
    from liso_amd.eval.det_validation import Collection, DetectionValidator

    return DetectionValidator([Collection("nusc/", "gt", metric_kwargs, "nusc")])


def _kwargs(g, as_one):
    m = fixture_metric(g, as_one)
    return dict(eval_movable_classes_as_one=as_one, class_names=m.class_names, class_ranges=m.class_ranges, sigmoid_scores=True)


@pytest.mark.parametrize("as_one", [True, False])
def test_restatement_and_evaluate_reproduce_the_devkit(golden, as_one):
    gt, pred = fixture_shapes(golden)
    v = _validator(_kwargs(golden, as_one))
    v.update_batch_host(gt, None, pred)
    res = v.compute("val/")
    r = assert_fixture(v.metrics[0], golden, as_one)
    if as_one:
        assert r["mean_ap"] > 0.2 and res["val/nusc/mAP"] == r["mean_ap"] and res["val/nusc/NDS"] == r["nd_score"]
        assert res["val/nusc/mAVE"] == 0.0 and res["val/nusc/mAAE"] == 1.0 and res["val/nusc/movable/ATE"] == r["tp_errors"]["trans_err"]
        assert set(res) == {f"val/nusc/{k}" for k in ("mAP", "mATE", "mASE", "mAOE", "mAVE", "mAAE", "NDS")} | {
            f"val/nusc/movable/{k}" for k in ("AP", "ATE", "ASE", "AOE", "AVE", "AAE")}
    else:  # the second class: no match at 0.5 m, and calc_tp's 1.0 branch at 2 m
        name = v.metrics[0].target_class_names[1]
        assert r["label_aps"][name][0.5] == 0.0 and not r["metric_data"][(name, 0.5)]["confidence"].any()
        assert r["metric_data"][(name, 2.0)]["confidence"].any() and r["label_tp_errors"][name]["trans_err"] == 1.0
        assert res[f"val/nusc/{name}/AVE"] == 1.0 and len(res) == 7 + 2 * 6


@pytest.mark.parametrize("as_one", [True, False])
def test_per_frame_update_equals_the_batched_path(golden, as_one):
    gt, pred = fixture_shapes(golden)
    v = _validator(_kwargs(golden, as_one))
    v.update_batch_host(gt[:5], None, pred[:5])  # two batches: the flattened state is concatenated across them
    v.update_batch_host(gt[5:], None, pred[5:])
    batched = v.compute("val/")
    m = fixture_metric(golden, as_one)
    for f in range(gt.valid.shape[0]):
        m.update(non_batched_gt_boxes=gt[f].drop_padding_boxes(), non_batched_pred_boxes=pred[f].drop_padding_boxes(), sample_token=str(f))
    per_frame = m.compute("val/nusc")
    assert set(per_frame) == set(batched) and all(per_frame[k] == batched[k] for k in batched), {k: (per_frame[k], batched[k]) for k in batched}
    assert_fixture(m, golden, as_one)


# ---- hand-made edges of the walk --------------------------------------------------------------------------------------------------
def _walk(gt_xy, pred_xy, gt_cls=None, pred_cls=None, radius=(50.0,), as_one=True, gt_rows=None, pred_rows=None, order=None, thresholds=(2.0,)):
    from liso_amd.eval.nuscenes_metrics import nusc_match_host

    def rows(xy, given):
        r = np.zeros((1, len(xy), 7), F32)
        r[0, :, 3:6] = 1.0
        r[0, :, :2] = np.asarray(xy, F32).reshape(len(xy), 2)
        if given is not None:
            r[0] = given
        return r
    g, p = rows(gt_xy, gt_rows), rows(pred_xy, pred_rows)
    G, P = g.shape[1], p.shape[1]
    gc = np.zeros((1, G), np.int32) if gt_cls is None else np.asarray(gt_cls, np.int32)[None]
    pc = np.zeros((1, P), np.int32) if pred_cls is None else np.asarray(pred_cls, np.int32)[None]
    order = np.arange(P, dtype=np.int32)[None] if order is None else np.asarray(order, np.int32)[None]
    o = nusc_match_host(g, np.ones((1, G), np.uint8), gc, p, np.ones((1, P), np.uint8), pc, order, np.asarray(radius, F32), as_one, thresholds)
    return o, [tuple(q) for q in o["pairs"][0, 0, : o["count"][0, 0]].tolist()]


def test_a_box_at_exactly_the_radius_is_kept():
    above = np.nextafter(F32(50.0), F32(np.inf))
    o, pairs = _walk([(50.0, 0.0), (above, 0.0), (30.0, 40.0)], [(0.0, 50.0), (0.0, above)])
    assert o["gt_in"].tolist() == [[1, 0, 1]] and o["pred_in"].tolist() == [[1, 0]] and pairs == []
    o, _ = _walk([(40.0, 0.0), (np.nextafter(F32(40.0), F32(np.inf)), 0.0)], [(45.0, 0.0)], gt_cls=[1, 1], pred_cls=[0], radius=(50.0, 40.0), as_one=False)
    assert o["gt_in"].tolist() == [[1, 0]] and o["pred_in"].tolist() == [[1]]  # the radius of the box's own class
    o, _ = _walk([(45.0, 0.0)], [(45.0, 0.0)], gt_cls=[1], pred_cls=[2], radius=(50.0, 40.0), as_one=False)
    assert o["gt_in"].tolist() == [[0]] and o["pred_in"].tolist() == [[0]]  # 45 m > 40 m; a class id past the table


def test_a_distance_of_exactly_the_threshold_is_no_match():
    o, pairs = _walk([(1.0, 0.0)], [(1.0, 2.0)])
    assert pairs == [] and o["count"].tolist() == [[0]]
    o, pairs = _walk([(1.0, 0.0)], [(1.0, np.nextafter(F32(2.0), F32(0.0)))])
    assert pairs == [(0, 0)] and o["err"][0, 0, 0, 0] == np.nextafter(F32(2.0), F32(0.0))


def test_equal_distances_take_the_lowest_slot():
    _, pairs = _walk([(9.0, 9.0), (0.0, 1.0), (0.0, -1.0), (1.0, 0.0)], [(0.0, 0.0)])
    assert pairs == [(1, 0)]


def test_the_second_nearest_is_matched_when_the_nearest_is_taken():
    _, pairs = _walk([(0.0, 0.0), (1.5, 0.0)], [(0.1, 0.0), (0.2, 0.0), (0.3, 0.0)], order=[1, 0, 2])
    assert pairs == [(0, 1), (1, 0)]  # the third finds nothing left


def test_a_class_mismatch_is_no_match():
    _, pairs = _walk([(0.0, 0.0), (1.0, 0.0)], [(0.0, 0.1)], gt_cls=[1, 0], pred_cls=[0], radius=(50.0, 50.0), as_one=False)
    assert pairs == [(1, 0)]
    _, pairs = _walk([(0.0, 0.0)], [(0.0, 0.1)], gt_cls=[1], pred_cls=[0], radius=(50.0, 50.0), as_one=False)
    assert pairs == []
    _, pairs = _walk([(0.0, 0.0)], [(0.0, 0.1)], gt_cls=[1], pred_cls=[0], radius=(50.0, 50.0), as_one=True)
    assert pairs == [(0, 0)]


def test_a_prediction_of_size_zero_is_clamped():
    g = np.array([[0, 0, 0, 2, 1, 1, 0.5]], F32)
    p = np.array([[0.3, 0.4, 0, 0, 1, 1, 0.25]], F32)
    o, pairs = _walk([(0, 0)], [(0, 0)], gt_rows=g, pred_rows=p)
    assert pairs == [(0, 0)]
    inter = F32(1e-4) * F32(1) * F32(1)
    scale = F32(1) - inter / (F32(2) + inter - inter)
    trans = np.sqrt(F32(0.3) * F32(0.3) + F32(0.4) * F32(0.4))
    assert o["err"][0, 0, 0].tolist() == [float(trans), float(scale), 0.25] and np.isfinite(scale) and scale < 1


def test_no_ground_truth_no_predictions_and_nan_centres():
    from liso_amd.eval.nuscenes_metrics import NuscenesObjectDetectionMetrics

    o, pairs = _walk(np.zeros((0, 2)), [(0.0, 0.0)])
    assert pairs == [] and o["pairs"].shape == (1, 1, 0, 2) and o["pred_in"].tolist() == [[1]]
    m = NuscenesObjectDetectionMetrics()  # npos == 0: no_predictions()
    m.accumulate_matches(np.full((1, 1), 0.5, F32), np.zeros((1, 1), np.int32), np.zeros((1, 0), np.int32),
                         np.zeros((1, 4), np.int32), np.zeros((1, 4, 0, 2), np.int16), np.zeros((1, 4, 0, 3), F32), o["gt_in"], o["pred_in"])
    r = m.evaluate()
    assert r["mean_ap"] == 0.0 and all(v == 1.0 for v in r["tp_errors"].values()) and r["nd_score"] == 0.0
    o, pairs = _walk([(0.0, 0.0)], np.zeros((0, 2)))
    assert pairs == [] and o["gt_in"].tolist() == [[1]]
    m = NuscenesObjectDetectionMetrics()  # ground truth and no predictions at all, and nothing accumulated
    assert m.evaluate()["nd_score"] == 0.0
    m.accumulate_matches(np.zeros((1, 0), F32), np.zeros((1, 0), np.int32), np.zeros((1, 1), np.int32), np.zeros((1, 4), np.int32),
                         np.zeros((1, 4, 0, 2), np.int16), np.zeros((1, 4, 0, 3), F32), o["gt_in"], o["pred_in"])
    assert m.evaluate()["mean_ap"] == 0.0 and m._npos.tolist() == [1]
    o, pairs = _walk([(np.nan, 0.0), (0.0, 0.0)], [(0.0, np.nan), (0.0, 0.5)])
    assert o["gt_in"].tolist() == [[0, 1]] and o["pred_in"].tolist() == [[0, 1]] and pairs == [(1, 1)]


def test_scores_outside_the_unit_interval_are_refused(golden):
    from liso_amd.eval.nuscenes_metrics import NuscenesObjectDetectionMetrics

    gt, pred = fixture_shapes(golden)  # raw logits, many of them negative
    m = NuscenesObjectDetectionMetrics()
    with pytest.raises(ValueError):
        m.update(non_batched_gt_boxes=gt[0].drop_padding_boxes(), non_batched_pred_boxes=pred[0].drop_padding_boxes())
    with pytest.raises(ValueError):
        NuscenesObjectDetectionMetrics(eval_movable_classes_as_one=False, class_names=("car", "barrier"))
    m = NuscenesObjectDetectionMetrics(eval_movable_classes_as_one=False)  # the reference's defaults, radii by class id
    assert m.class_names[2] == "trailer" and m.radius.tolist() == [50, 50, 50, 50, 50, 40, 40, 40] and m.target_class_names[2] == "bus"


# ---- run_val's collection sets ------------------------------------------------------------------------------------------------------
def test_the_flag_off_leaves_collections_and_keys_as_they_were():
    from liso_amd.eval.det_validation import DetectionValidator
    from tests.det_val_cases import pad_batch, scene

    v = DetectionValidator.for_run_val("kitti", ("car", "ped"), (0, 1))
    w = DetectionValidator.for_run_val("kitti", ("car", "ped"), (0, 1), nuscenes_metrics=True)
    assert len(v.collections) == 25 and all(c.kind == "od" for c in v.collections) and [c.tag for c in w.collections[:25]] == [c.tag for c in v.collections]
    assert len(w.collections) == 26 and w.collections[25] == ("final_result/NUSC_OFFICIAL/detection_metrics/", "gt",
                                                              dict(eval_movable_classes_as_one=True, sigmoid_scores=False), "nusc")
    for name in ("gt", "benchmark"):  # the job tables are untouched
        assert w.tables[name].jobs == v.tables[name].jobs and w.tables[name].filters == v.tables[name].filters and not w.assign_tables[name].jobs
    g = np.random.default_rng(3)
    frames = [scene(g, 9, 14, 2) for _ in range(3)]
    gt, pred = pad_batch([f[0] for f in frames]), pad_batch([f[1] for f in frames])
    draws = torch.from_numpy(g.integers(0, 2, (3, 14)).astype(np.int32))
    v.update_batch_host(gt, gt, pred, class_draws=draws)
    w.update_batch_host(gt, gt, pred, class_draws=draws)
    off, on = v.compute("val/"), w.compute("val/")
    same = lambda a, b: a == b or (np.isnan(a) and np.isnan(b))  # noqa: E731
    assert len(off) > 1000 and set(off) < set(on) and all(same(on[k], x) for k, x in off.items())
    new = set(on) - set(off)
    assert new == {"val/final_result/NUSC_OFFICIAL/detection_metrics/" + k for k in (
        "mAP", "mATE", "mASE", "mAOE", "mAVE", "mAAE", "NDS", "movable/AP", "movable/ATE", "movable/ASE", "movable/AOE", "movable/AVE", "movable/AAE")}
    assert on["val/final_result/NUSC_OFFICIAL/detection_metrics/mAP"] > 0.1


def test_nuscenes_is_buildable_with_the_flag_only():
    from liso_amd.eval.det_validation import DetectionValidator

    with pytest.raises(NotImplementedError):
        DetectionValidator.for_run_val("nuscenes")
    with pytest.raises(NotImplementedError):
        DetectionValidator.for_run_val("nuscenes", waymo_metrics=True)
    n = DetectionValidator.for_run_val("nuscenes", nuscenes_metrics=True, sigmoid_scores=True)
    assert len(n.collections) == 26 and [c.kind for c in n.collections] == ["od"] * 24 + ["nusc"] * 2 and n.n_classes == 8
    assert all(m.min_precision == 0.1 for c, m in zip(n.collections[:24], n.metrics) if "waymo_cropped" not in c.tag)
    assert n.collections[24].tag == "final_result/NUSC_OFFICIAL/per_class/detection_metrics/" and not n.metrics[24].eval_movable_classes_as_one
    assert n.metrics[24].sigmoid_scores and n.metrics[25].sigmoid_scores and n.metrics[25].eval_movable_classes_as_one
    assert len(n.tables["gt"].jobs) == 64 and len(n.tables["benchmark"].jobs) == 32
    s = DetectionValidator.for_run_val("nuscenes", ("pedestrian", "car", "bicycle"), (2, 0, 1), nuscenes_metrics=True)
    assert s.metrics[24].class_names == ("car", "bicycle", "pedestrian") and s.metrics[24].radius.tolist() == [50, 40, 40]
    with pytest.raises(ValueError):
        DetectionValidator.for_run_val("nuscenes", ("car", "pedestrian"), (0, 2), nuscenes_metrics=True)
