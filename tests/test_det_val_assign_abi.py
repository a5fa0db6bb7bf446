"""CPU: the C ABI of the optimal assignment (include/liso_det_val.h: liso_det_val_assign_f32, liso_match_assign_f32) -- exported
symbols, error codes without a GPU, what Python refuses, and the validator's tables with and without the Waymo-style collections."""
import ctypes

import numpy as np
import pytest

from tests.det_val_cases import pad_batch, scene

SYMBOLS = ("liso_det_val_assign_f32", "liso_match_assign_f32")


def test_library_exports_the_symbols():
    from liso_amd import _lib

    lib = _lib.lib()
    for s in SYMBOLS:
        assert s in _lib.SIGNATURES and hasattr(lib, s), s


def test_error_codes_without_gpu():
    from liso_amd import _lib

    lib = _lib.lib()
    one = ctypes.c_void_p(8)  # a non-null pointer that is never dereferenced: every call below returns before it launches
    a = lambda *args: lib.liso_det_val_assign_f32(*args)  # noqa: E731
    #        F  G  P  gt   gv   gc   pred pv   pc   bev  i3d  mask filters S jobs J count pairs gt_in pred_in stream
    assert a(0, 4, 4, None, None, None, None, None, None, None, None, 3, None, 1, None, 2, None, None, None, None, None) == 0  # F == 0
    assert a(2, 4, 4, one, one, one, one, one, one, one, one, 3, one, 1, one, 0, one, one, one, one, None) == 0  # no jobs
    assert a(2, 4, 4, one, one, one, one, one, one, one, one, 4, one, 1, one, 2, one, one, one, one, None) == -1  # `dist` bit
    assert a(2, 4, 4, one, one, one, one, one, one, one, one, -1, one, 1, one, 2, one, one, one, one, None) == -1
    assert a(2, 4, 4, one, one, one, one, one, one, None, one, 1, one, 1, one, 2, one, one, one, one, None) == -1  # job matrix missing
    assert a(2, 4, 4, one, one, one, one, one, one, one, None, 2, one, 1, one, 2, one, one, one, one, None) == -1
    assert a(2, 4, 4, one, one, one, one, one, one, None, None, 0, one, 1, one, 2, one, one, one, one, None) == -1  # no matrix at all
    assert a(2, 4, 4, one, one, one, one, one, one, one, one, 3, None, 1, one, 2, one, one, one, one, None) == -1  # no filter table
    assert a(2, 4, 4, one, one, one, one, one, one, one, one, 3, one, 1, one, 2, None, one, one, one, None) == -1  # no count
    assert a(2, 4, 4, one, one, one, one, one, one, one, one, 3, one, 1, one, 2, one, None, one, one, None) == -1  # no pairs
    assert a(2, 1025, 4, one, one, one, one, one, one, one, one, 3, one, 1, one, 2, one, one, one, one, None) == -1
    assert a(-1, 4, 4, one, one, one, one, one, one, one, one, 3, one, 1, one, 2, one, one, one, one, None) == -1
    m = lambda *args: lib.liso_match_assign_f32(*args)  # noqa: E731
    assert m(None, 0, 4, 4, 0.4, None, None, None) == 0  # an empty batch launches nothing
    assert m(None, 2, 4, 4, 0.4, one, one, None) == -1
    assert m(one, 2, 4, 4, 0.4, None, one, None) == -1
    assert m(one, 2, 4, 4, 0.4, one, None, None) == -1
    assert m(one, 2, 4, 2000, 0.4, one, one, None) == -1 and m(one, -1, 4, 4, 0.4, one, one, None) == -1


def test_python_refuses_what_is_not_built():
    import torch

    from liso_amd import _lib
    from liso_amd.eval.det_validation import Collection, DetectionValidator, FilterSet, JobTable, match_detections, match_detections_host, pack_boxes
    from liso_amd.kabsch.box_groundtruth_matching_iou import assign_iou_matrix

    t = JobTable([FilterSet()], assignment=True)
    with pytest.raises(NotImplementedError):
        t.add_job(0, "dist", 2.0)
    assert t.add_job(0, "iou_bev", 0.4) == 0 and t.criteria_mask == 1
    gt, pred = scene(np.random.default_rng(0), 5, 6, 2)
    gt, pred = pad_batch([gt]), pad_batch([pred])
    greedy = JobTable([FilterSet()], [(0, "iou_bev", 0.4)])
    pk = lambda s: {k: v.numpy() for k, v in pack_boxes(s).items()}  # noqa: E731
    with pytest.raises(NotImplementedError):  # a greedy table is not an assignment table
        match_detections_host(pk(gt), pk(pred), greedy, assign=greedy)
    with pytest.raises(_lib.LisoHipError):  # host tensors
        match_detections(gt, pred, greedy, assign=t)
    with pytest.raises(_lib.LisoHipError):
        assign_iou_matrix(torch.zeros(3, 4), 0.4)
    with pytest.raises(NotImplementedError):  # the nuScenes devkit wrapper stays out, Waymo needs the flag
        DetectionValidator.for_run_val("nuscenes", waymo_metrics=True)
    with pytest.raises(NotImplementedError):
        DetectionValidator.for_run_val("waymo")
    with pytest.raises(ValueError):
        DetectionValidator([Collection("", "gt", {}, "other")])
    with pytest.raises(NotImplementedError):  # `dist` with optimal assignment
        DetectionValidator([Collection("", "gt", dict(moving_velocity_thresh=0.1, box_matching_criterion="dist", use_slow_nuscenes_matching=False))])


def test_run_val_tables_with_and_without_the_flag():
    from liso_amd.eval.det_validation import DetectionValidator

    v = DetectionValidator.for_run_val("kitti", ("car", "ped"), (0, 1))
    assert len(v.collections) == 25 and len(v.tables["gt"].jobs) == 32 + 32 + 8 and len(v.tables["benchmark"].jobs) == 32
    assert not v.assign_tables["gt"].jobs and not v.assign_tables["benchmark"].jobs
    w = DetectionValidator.for_run_val("kitti", ("car", "ped"), (0, 1), waymo_metrics=True)
    assert len(w.collections) == 29 and [c.kind for c in w.collections[25:]] == ["waymo"] * 4
    assert [c.tag for c in w.collections[:25]] == [c.tag for c in v.collections]
    assert len(w.tables["gt"].jobs) == 72 and len(w.tables["benchmark"].jobs) == 32  # the greedy tables are untouched
    assert not w.assign_tables["gt"].jobs and len(w.assign_tables["benchmark"].jobs) == 4 * 2
    assert w.collections[26].tag == "final_result/WAYMO/detection_metrics/0_20m" and w.collections[26].gt_set == "benchmark"
    y = DetectionValidator.for_run_val("waymo", ("car", "ped", "cyc"), (0, 1, 2), waymo_metrics=True)
    assert len(y.collections) == 24 + 1 + 4 and y.collections[24].kind == "waymo" and y.collections[24].gt_set == "gt"
    assert y.collections[24].tag == "final_result/WAYMO/per_class/detection_metrics/"
    assert all(m.min_precision == 0.1 for c, m in zip(y.collections[:24], y.metrics) if "waymo_cropped" not in c.tag)
    assert len(y.tables["gt"].jobs) == 64 and len(y.assign_tables["gt"].jobs) == 3 * 2 and len(y.assign_tables["benchmark"].jobs) == 8
    assert y.assign_tables["gt"].needs_classes and not y.assign_tables["benchmark"].needs_classes
