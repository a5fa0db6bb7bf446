"""CPU: the error paths of liso_amd/utils/device_args.py, with the messages the data-path wrappers raised before they shared it."""
import numpy as np
import pytest
import torch

from liso_amd._lib import LisoHipError
from liso_amd.utils import device_args as A


def test_cloud3_refuses_wrong_shapes_dtypes_and_cpu_tensors():
    for bad in (np.zeros((4, 3), np.float32), torch.zeros(4), torch.zeros(2, 4, 3, 1), torch.zeros(4, 2)):
        with pytest.raises(LisoHipError, match=r"pcl must be a \[N, C\] or \[B, N, C\] tensor with C >= 3"):
            A.cloud3(bad)
    with pytest.raises(LisoHipError, match=r"cloud_b must be a \[N, C\]"):
        A.cloud3(torch.zeros(4), "cloud_b")
    for allow in (False, True):  # the CPU check comes before the dtype and the batch checks
        with pytest.raises(LisoHipError, match="device op called with a CPU tensor"):
            A.cloud3(torch.zeros((0, 4, 3), dtype=torch.float64), allow_empty_batch=allow)


def test_counts_arg_refuses_what_is_not_int32_per_cloud():
    p3 = torch.zeros(2, 5, 3)
    assert A.counts_arg(None, p3) is None
    good = torch.tensor([5, 3], dtype=torch.int32)
    assert A.counts_arg(good, p3) is good
    for bad in ([5, 3], np.array([5, 3], np.int32), good.long(), good[:1], good[None]):
        with pytest.raises(LisoHipError, match=r"counts must be an int32 \[B\] tensor on the cloud's device"):
            A.counts_arg(bad, p3)


def test_as_u8_views_bools_keeps_bytes_and_refuses_the_rest():
    m = torch.tensor([[True, False], [False, True]])
    v = A.as_u8(m)
    assert v.dtype == torch.uint8 and v.data_ptr() == m.data_ptr() and v.tolist() == [[1, 0], [0, 1]]
    t = A.as_u8(m.t())
    assert t.is_contiguous() and t.tolist() == [[1, 0], [0, 1]]
    assert A.as_u8(v) is v
    with pytest.raises(LisoHipError, match="must be a bool or uint8 tensor, got torch.float32"):
        A.as_u8(torch.ones(2))
    assert A.as_u8(torch.tensor([0.0, 2.0]), convert=True).tolist() == [0, 2]


def test_opt_ptr_and_is_np():
    assert A.opt_ptr(None) is None and A.opt_ptr(torch.zeros(0, 3)) is None
    t = torch.zeros(3)
    assert A.opt_ptr(t).value == t.data_ptr()
    assert A.is_np(np.zeros(1)) and not A.is_np(t) and not A.is_np([1.0])
