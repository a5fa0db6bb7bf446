"""CPU: the C ABI of the nuScenes metrics' device part (include/liso_nusc_metrics.h: liso_det_val_nusc_f32) -- the exported symbol,
its error codes without a GPU, and what the Python device path refuses."""
import ctypes

import numpy as np
import pytest


def test_library_exports_the_symbol():
    from liso_amd import _lib

    assert "liso_det_val_nusc_f32" in _lib.SIGNATURES and hasattr(_lib.lib(), "liso_det_val_nusc_f32")
    assert len(_lib.SIGNATURES["liso_det_val_nusc_f32"][1]) == 21


def test_error_codes_without_gpu():
    from liso_amd import _lib

    lib = _lib.lib()
    one = ctypes.c_void_p(8)  # a non-null pointer that is never dereferenced: every call below returns before it launches
    thr = (ctypes.c_float * 8)(0.5, 1.0, 2.0, 4.0, 5.0, 6.0, 7.0, 8.0)
    n = lambda *args: lib.liso_det_val_nusc_f32(*args)  # noqa: E731
    #        F  G  P  gt   gv   gc   pred pv   pc   order radius C as_one thr T count pairs err gt_in pred_in stream
    assert n(0, 4, 4, None, None, None, None, None, None, None, None, 1, 1, None, 4, None, None, None, None, None, None) == 0  # F == 0
    assert n(-1, 4, 4, one, one, one, one, one, one, one, one, 1, 1, thr, 4, one, one, one, one, one, None) == -1
    assert n(2, 1025, 4, one, one, one, one, one, one, one, one, 1, 1, thr, 4, one, one, one, one, one, None) == -1
    assert n(2, 4, 1025, one, one, one, one, one, one, one, one, 1, 1, thr, 4, one, one, one, one, one, None) == -1
    assert n(2, 4, -1, one, one, one, one, one, one, one, one, 1, 1, thr, 4, one, one, one, one, one, None) == -1
    assert n(2, 4, 4, one, one, one, one, one, one, one, one, 1, 1, thr, 9, one, one, one, one, one, None) == -1  # T > 8
    assert n(2, 4, 4, one, one, one, one, one, one, one, one, 1, 1, thr, 0, one, one, one, one, one, None) == -1  # T < 1
    assert n(0, 4, 4, None, None, None, None, None, None, None, None, 1, 1, None, 9, None, None, None, None, None, None) == -1  # also with F == 0
    assert n(2, 4, 4, one, one, one, one, one, one, one, one, 0, 1, thr, 4, one, one, one, one, one, None) == -1  # no class
    ok = [2, 4, 4, one, one, one, one, one, one, one, one, 2, 0, thr, 4, one, one, one, one, one, None]
    for i in (3, 4, 5, 6, 7, 8, 9, 10, 13, 15, 16, 17, 18, 19):  # every required pointer
        bad = list(ok)
        bad[i] = None
        assert n(*bad) == -1, i
    # G == 0 / P == 0: the pointers of the empty side, and pairs / err, are not required; seen through the other side's missing output
    empty_gt = [2, 0, 4, None, None, None, one, one, one, one, one, 2, 0, thr, 4, one, None, None, None, None, None]
    assert n(*empty_gt) == -1  # pred_in missing
    empty_pred = [2, 4, 0, one, one, one, None, None, None, None, one, 2, 0, thr, 4, one, None, None, None, None, None]
    assert n(*empty_pred) == -1  # gt_in missing


def test_the_device_path_refuses_cpu_tensors():
    import torch

    from liso_amd import _lib
    from liso_amd.eval.det_validation import Collection, DetectionValidator, pack_boxes
    from liso_amd.eval.nuscenes_metrics import nusc_match_packed
    from tests.det_val_cases import pad_batch, scene

    gt, pred = scene(np.random.default_rng(0), 5, 6, 2)
    gt, pred = pad_batch([gt]), pad_batch([pred])
    g, p = pack_boxes(gt), pack_boxes(pred)
    order = torch.zeros((1, 6), dtype=torch.int32)
    with pytest.raises(_lib.LisoHipError):
        nusc_match_packed(g, p, order, torch.tensor([50.0]), True)
    v = DetectionValidator([Collection("n/", "gt", {}, "nusc")])
    with pytest.raises(_lib.LisoHipError):
        v.update_batch(gt, None, pred)
    with pytest.raises(ValueError):
        DetectionValidator([Collection("n/", "gt", {}, "nuscenes")])
