"""CPU: the C ABI of include/liso_det_val.h -- exported symbols, error codes without a GPU, CPU tensors refused, and the host
twin of the pair kernel against the library's other host entry point."""
import ctypes

import numpy as np
import pytest
import torch

from tests.det_val_cases import pad_batch, scene

SYMBOLS = ("liso_det_val_pairs_f32", "liso_det_val_pairs_cpu_f32", "liso_det_val_transfer_classes", "liso_det_val_match_f32")


def test_library_exports_the_symbols():
    from liso_amd import _lib

    lib = _lib.lib()
    for s in SYMBOLS:
        assert s in _lib.SIGNATURES and hasattr(lib, s), s


def test_error_codes_without_gpu():
    from liso_amd import _lib

    lib = _lib.lib()
    one = ctypes.c_void_p(8)  # a non-null pointer that is never dereferenced: every call below returns before it launches
    assert lib.liso_det_val_pairs_f32(-1, 1, 1, one, one, one, one, one, one, one, None) == -1
    assert lib.liso_det_val_pairs_f32(1, 1025, 1, one, one, one, one, one, one, one, None) == -1
    assert lib.liso_det_val_pairs_f32(1, 4, 4, None, one, one, one, one, one, one, None) == -1
    assert lib.liso_det_val_pairs_f32(0, 4, 4, None, None, None, None, None, None, None, None) == 0  # no frames: nothing launched
    assert lib.liso_det_val_pairs_f32(3, 0, 4, None, None, None, None, None, None, None, None) == 0  # no pairs
    assert lib.liso_det_val_pairs_cpu_f32(1, 4, -2, one, one, one, one, one, one, one) == -1
    assert lib.liso_det_val_transfer_classes(2, 4, 0, None, None, None, None, None, 3.0, None, None, None) == 0
    assert lib.liso_det_val_transfer_classes(2, 4, 4, one, one, one, one, one, 3.0, None, one, None) == -1
    m = lambda *a: lib.liso_det_val_match_f32(*a)  # noqa: E731
    assert m(2, 4, 4, one, one, one, one, one, one, one, one, one, one, 7, one, 1, one, 0, one, one, one, one, one, None) == 0  # no jobs
    assert m(2, 4, 4, one, one, one, one, one, one, one, one, one, one, 7, None, 1, one, 3, one, one, one, one, one, None) == -1
    assert m(2, 4, 4, one, one, one, one, one, one, one, None, one, one, 1, one, 1, one, 3, one, one, one, one, one, None) == -1  # job matrix missing
    assert m(2, 4, 4, one, one, one, one, one, one, one, one, one, one, 8, one, 1, one, 3, one, one, one, one, one, None) == -1
    assert m(2, 4, 2000, one, one, one, one, one, one, one, one, one, one, 7, one, 1, one, 3, one, one, one, one, one, None) == -1


def test_device_path_refuses_cpu_tensors():
    from liso_amd import _lib
    from liso_amd.eval.det_validation import DetectionValidator, FilterSet, JobTable, match_detections

    gt, pred = scene(np.random.default_rng(0), 5, 6, 2)
    gt, pred = pad_batch([gt]), pad_batch([pred])
    t = JobTable([FilterSet()], [(0, "iou_bev", 0.5)])
    with pytest.raises(_lib.LisoHipError):
        match_detections(gt, pred, t)
    with pytest.raises(_lib.LisoHipError):
        DetectionValidator.for_run_val("av2").update_batch(gt, gt, pred)


def test_host_twin_bev_iou_equals_the_cpu_entry_point_bitwise():
    from liso_amd import iou3d_nms_cuda as M
    from liso_amd.eval.det_validation import host_pair_matrices, pack_boxes

    g = np.random.default_rng(5)
    frames = [scene(g, n_gt, n_pred, 3, spread=12.0) for n_gt, n_pred in ((17, 70), (66, 9))]
    gt, pred = pack_boxes(pad_batch([f[0] for f in frames])), pack_boxes(pad_batch([f[1] for f in frames]))
    mats = host_pair_matrices(gt["rows"].numpy(), gt["valid"].numpy(), pred["rows"].numpy(), pred["valid"].numpy())
    hits = 0
    for f, (n_gt, n_pred) in enumerate(((17, 70), (66, 9))):
        want = torch.zeros(n_gt, n_pred)
        assert M.boxes_iou_bev_cpu(gt["rows"][f, :n_gt].contiguous(), pred["rows"][f, :n_pred].contiguous(), want) == 1
        got = mats["iou_bev"][f, :n_pred, :n_gt]
        assert np.array_equal(got.view(np.uint32), want.numpy().T.copy().view(np.uint32))
        hits += int((got > 0).sum())
        assert not mats["iou_bev"][f, n_pred:].any() and not mats["iou_bev"][f, :, n_gt:].any()  # pairs with a padding slot: 0
        d = np.linalg.norm(gt["rows"][f, None, :n_gt, :2].numpy().astype(np.float64) - pred["rows"][f, :n_pred, None, :2].numpy(), axis=-1)
        assert np.allclose(mats["dist"][f, :n_pred, :n_gt], d, rtol=1e-6, atol=0)
    assert hits > 50
