"""Shared checks of the fp16 parametrizations of the detector-path GPU tests."""
import torch


def require_fp16():
    """host check, before anything is allocated: the library was built with fp16 storage (LISO_CONV_F16 / element code 2)"""
    from liso_amd import _lib as L

    assert hasattr(L, "CONV_F16") and hasattr(L, "elem_code"), "fp16 storage is not built"
    assert L.elem_code(torch.float16) == L.ELEM_F16 == 2
    return L


def ulp16(v):
    """spacing of fp16 at |v| (2^-24 in the subnormal range)"""
    a = v.abs().double().clamp(min=2.0 ** -14)
    return torch.exp2(torch.floor(torch.log2(a)) - 10)


def assert_fp16_rounded(y, ref, slack_rel):
    """every element of the fp16 result `y` within half an fp16 ulp of the exact `ref`, plus `slack_rel` * max|ref| for the fp32
    arithmetic in front of the store: a store that truncates or rounds to a coarser format is off by more than half an ulp"""
    y, ref = y.detach().double().cpu(), ref.detach().double().cpu()
    err = (y - ref).abs() - 0.5 * ulp16(ref)
    lim = slack_rel * float(ref.abs().max())
    assert float(err.max()) <= lim, f"max error {float(((y - ref).abs() / ulp16(ref)).max()):.3f} fp16 ulps"
