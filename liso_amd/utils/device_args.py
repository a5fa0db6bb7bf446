"""Argument checks shared by the Python wrappers of the data-path kernels (ground removal, sample and label preparation, detector
NMS, snippet harvest): what a cloud, its `counts`, a mask and an optional pointer look like at the C ABI.  A new wrapper imports
these instead of writing them out again."""
import numpy as np
import torch

from liso_amd import _lib as L


def is_np(x):
    return isinstance(x, np.ndarray)


def opt_ptr(t):
    """void* of a tensor; None for an absent or empty one (an empty tensor has no address to hand over)"""
    return None if t is None or t.numel() == 0 else L.ptr(t)


def as_u8(t, convert=False):
    """the bytes a kernel reads a mask as: a contiguous uint8 view of a bool tensor, a uint8 tensor as it is (made contiguous).  Any
    other dtype raises, or with `convert` is cast the way `.to(torch.uint8)` casts it."""
    if t.dtype == torch.bool:
        return t.contiguous().view(torch.uint8)
    if t.dtype != torch.uint8 and not convert:
        raise L.LisoHipError(f"a mask must be a bool or uint8 tensor, got {t.dtype}")
    return t.to(torch.uint8).contiguous()


def cloud3(pcl, name="pcl", allow_empty_batch=False):
    """float32 device cloud [N, C] or [B, N, C], C >= 3 -> its contiguous [B, N, C] view.  A batch of no clouds raises unless
    `allow_empty_batch`."""
    if not torch.is_tensor(pcl) or pcl.dim() not in (2, 3) or pcl.shape[-1] < 3:
        raise L.LisoHipError(f"{name} must be a [N, C] or [B, N, C] tensor with C >= 3")
    L.require_cuda(pcl)
    if pcl.dtype != torch.float32:
        raise L.LisoHipError(f"{name} must be float32 on the device, got {pcl.dtype}")
    p3 = pcl if pcl.dim() == 3 else pcl[None]
    if p3.shape[0] < 1 and not allow_empty_batch:
        raise L.LisoHipError(f"{name}: need at least one cloud")
    return p3.contiguous()


def counts_arg(counts, p3):
    """the optional rows-per-cloud of the cloud `p3` [B, N, C]: int32 [B] on its device, contiguous; None stays None"""
    if counts is None:
        return None
    if not torch.is_tensor(counts) or counts.dtype != torch.int32 or tuple(counts.shape) != (p3.shape[0],) or counts.device != p3.device:
        raise L.LisoHipError("counts must be an int32 [B] tensor on the cloud's device")
    return counts.contiguous()
