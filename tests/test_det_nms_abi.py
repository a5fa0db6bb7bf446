"""CPU: the detector NMS ABI (include/liso_det_nms.h) is exported, its workspace query behaves, and every entry point refuses bad
arguments before it launches anything; the Python wrappers refuse wrong dtypes and CPU tensors."""
import ctypes
import os

import pytest
import torch

EINVAL = -1


def _lib():
    from liso_amd import _lib as L

    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return L


def test_symbols_present():
    L = _lib()
    lib = L.lib()
    for s in ("liso_det_nms_workspace_bytes", "liso_det_nms_order", "liso_det_nms_select", "liso_det_nms_gather"):
        assert hasattr(lib, s) and s in L.SIGNATURES
    assert ctypes.sizeof(L.DetGatherField) == 32  # 2 pointers, 2 ints, 1 uint64


def test_workspace_query_is_monotone():
    lib = _lib().lib()
    assert lib.liso_det_nms_workspace_bytes(1, 0) == 0
    assert lib.liso_det_nms_workspace_bytes(0, 100) == 0
    assert lib.liso_det_nms_workspace_bytes(1, (1 << 24) + 1) == 0  # above LISO_DET_NMS_MAX_N
    prev = 0
    for n in (1, 63, 64, 4095, 4096, 4097, 16384, 65536, 1 << 20, 1 << 24):
        w = lib.liso_det_nms_workspace_bytes(1, n)
        assert w >= 8 * n and w >= prev, (n, w, prev)
        prev = w
    for n in (1, 1000, 65536):
        ws = [lib.liso_det_nms_workspace_bytes(b, n) for b in (1, 2, 4, 8)]
        assert ws == sorted(ws) and ws[1] >= 2 * 8 * n


def test_order_refuses_bad_arguments_before_launching():
    lib = _lib().lib()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 255) // 256 * 256)  # never touched: every call below returns first
    big = 1 << 30

    def order(b=2, n=100, s=p, gate=None, valid=None, keys=p, idx=p, ws=p, wsb=big):
        return lib.liso_det_nms_order(b, n, s, gate, valid, -1e32, keys, idx, ws, wsb, None)

    assert order(b=0) == EINVAL
    assert order(b=-3) == EINVAL
    assert order(n=-1) == EINVAL
    assert order(n=(1 << 24) + 1) == EINVAL
    assert order(s=None) == EINVAL
    assert order(keys=None) == EINVAL
    assert order(idx=None) == EINVAL
    assert order(ws=None) == EINVAL
    assert order(wsb=lib.liso_det_nms_workspace_bytes(2, 100) - 1) == -2  # LISO_EWORKSPACE
    assert order(n=0) == EINVAL  # N == 0 with non-null arrays
    assert order(n=0, s=None, keys=None, idx=None, ws=None, wsb=0) == 0  # empty: nothing to launch


def test_select_refuses_bad_arguments_before_launching():
    lib = _lib().lib()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 255) // 256 * 256)

    def select(b=2, n=100, boxes=p, keys=p, idx=p, pre=0, post=500, keep=p, counts=p):
        return lib.liso_det_nms_select(b, n, boxes, keys, idx, 0.1, pre, post, keep, counts, None)

    assert select(b=0) == EINVAL
    assert select(n=-1) == EINVAL
    assert select(post=1025) == EINVAL  # above LISO_DET_NMS_MAX_POST
    assert select(post=0) == EINVAL
    assert select(boxes=None) == EINVAL
    assert select(keys=None) == EINVAL
    assert select(idx=None) == EINVAL
    assert select(keep=None) == EINVAL
    assert select(counts=None) == EINVAL
    assert select(n=0) == EINVAL  # N == 0 with non-null inputs


def test_gather_refuses_bad_arguments_before_launching():
    L = _lib()
    lib = L.lib()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 255) // 256 * 256)
    f = (L.DetGatherField * 9)(*[L.DetGatherField(p, p, 3, 4, 0) for _ in range(9)])

    def gather(b=2, n=100, post=500, keep=p, counts=p, fields=f, nf=2):
        return lib.liso_det_nms_gather(b, n, post, keep, counts, None if fields is None else ctypes.cast(fields, ctypes.c_void_p), nf,
                                       None)

    assert gather(b=0) == EINVAL
    assert gather(n=-5) == EINVAL
    assert gather(post=1025) == EINVAL
    assert gather(keep=None) == EINVAL
    assert gather(counts=None) == EINVAL
    assert gather(fields=None) == EINVAL
    assert gather(nf=0) == EINVAL
    assert gather(nf=9) == EINVAL  # above LISO_DET_GATHER_MAX_FIELDS
    assert gather(n=0) == EINVAL   # N == 0 with a non-null source
    bad = (L.DetGatherField * 1)(L.DetGatherField(p, p, 3, 3, 0))
    assert gather(fields=bad, nf=1) == EINVAL  # element size 3
    bad = (L.DetGatherField * 1)(L.DetGatherField(p, None, 3, 4, 0))
    assert gather(fields=bad, nf=1) == EINVAL  # no destination


def test_python_wrappers_refuse_wrong_dtype_and_cpu_tensors():
    L = _lib()
    from liso_amd import det_nms as D

    with pytest.raises(L.LisoHipError, match="float32"):
        D.order(torch.zeros(2, 8, dtype=torch.float64))
    with pytest.raises(L.LisoHipError, match="CPU tensor"):
        D.order(torch.zeros(2, 8))
    with pytest.raises(L.LisoHipError, match="float32"):
        D.select(torch.zeros(1, 8, 7, dtype=torch.float16), torch.zeros(1, 8, dtype=torch.int32), torch.zeros(1, 8, dtype=torch.int32), 0.1)
    with pytest.raises(L.LisoHipError, match="CPU tensor"):
        D.select(torch.zeros(1, 8, 7), torch.zeros(1, 8, dtype=torch.int32), torch.zeros(1, 8, dtype=torch.int32), 0.1)
    with pytest.raises(L.LisoHipError, match="int64"):
        D.gather(torch.zeros(1, 4, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), [torch.zeros(1, 8, 3)], [0.0])
    with pytest.raises(L.LisoHipError, match="CPU tensor"):
        D.gather(torch.zeros(1, 4, dtype=torch.int64), torch.zeros(1, dtype=torch.int32), [torch.zeros(1, 8, 3)], [0.0])


def test_batched_entry_points_exist():
    from liso_amd.networks.simple_net.simple_net import BoxLearner
    from liso_amd.utils.config import default_cfg
    from liso_amd.utils.nms_iou import iou_based_nms_batched

    assert callable(iou_based_nms_batched) and callable(BoxLearner.predict_boxes)
    assert default_cfg().nms_iou_threshold == 0.1
