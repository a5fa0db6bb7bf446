"""Python boundary of include/liso_det_nms.h: detector maps -> post-NMS boxes on the device, for a batch, with no host sync.

`order` (a), `select` (b) and `gather` (c) are the three C calls; `liso_amd.utils.nms_iou.iou_based_nms_batched` composes them
for a padded `Shape`.  Every wrapper checks devices, dtypes and shapes before anything is launched and raises
`LisoHipError` on a mismatch; nothing here reads device memory back, so all three steps can be captured in one hipGraph.
"""
import ctypes

import torch

from liso_amd import _lib as L
from liso_amd.utils.device_args import as_u8, opt_ptr as _p

MAX_POST = 1024  # LISO_DET_NMS_MAX_POST
MAX_N = 1 << 24  # LISO_DET_NMS_MAX_N
MAX_FIELDS = 8  # LISO_DET_GATHER_MAX_FIELDS


def _need(t, name, dtype, shape):
    if not torch.is_tensor(t):
        raise L.LisoHipError(f"{name} must be a tensor")
    if t.dtype != dtype:
        raise L.LisoHipError(f"{name} must be {dtype}, got {t.dtype}")
    L.require_cuda(t)
    if tuple(t.shape) != tuple(shape):
        raise L.LisoHipError(f"{name} must have shape {tuple(shape)}, got {tuple(t.shape)}")
    if not t.is_contiguous():
        raise L.LisoHipError(f"{name} must be contiguous")


def _bn(scores):
    if not torch.is_tensor(scores) or scores.dim() != 2:
        raise L.LisoHipError("scores must be a [B, N] tensor")
    B, N = scores.shape
    if B < 1 or N > MAX_N:
        raise L.LisoHipError(f"need B >= 1 and N <= {MAX_N}, got B={B}, N={N}")
    return B, N


def order(scores, gate=None, valid=None, logit_threshold=None):
    """(a) per-sample stable descending order of the participating slots.
    scores fp32 [B,N]; gate fp32 [B,N] (compared against `logit_threshold` instead of the scores); valid bool/uint8 [B,N].
    A slot takes part iff valid and not (gate < logit_threshold); `logit_threshold=None` drops nothing.
    Returns (sorted_keys int32 [B,N] holding the uint32 keys, sorted_idx int32 [B,N]): ties keep ascending slot index, NaN first,
    the slots that take no part last (key 0xFFFFFFFF, i.e. -1 as int32)."""
    B, N = _bn(scores)
    _need(scores, "scores", torch.float32, (B, N))
    if gate is not None:
        _need(gate, "gate", torch.float32, (B, N))
    if valid is not None:
        if valid.dtype == torch.bool:
            valid = as_u8(valid)
        _need(valid, "valid", torch.uint8, (B, N))
    dev = scores.device
    keys = torch.empty((B, N), dtype=torch.int32, device=dev)
    idx = torch.empty((B, N), dtype=torch.int32, device=dev)
    thr = float("-inf") if logit_threshold is None else float(logit_threshold)
    lib = L.lib()
    ws_bytes = lib.liso_det_nms_workspace_bytes(B, N)
    ws = torch.empty(max(ws_bytes, 256), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        L.check(lib.liso_det_nms_order(B, N, _p(scores), _p(gate), _p(valid), thr, _p(keys), _p(idx), _p(ws) if N else None,
                                       ws_bytes, L.stream_ptr()), "det_nms order")
    return keys, idx


def select(boxes, sorted_keys, sorted_idx, thresh, pre_nms_max=None, post_nms_max=500):
    """(b) the first `post_nms_max` survivors of the reference's greedy rotated NMS over the first `pre_nms_max` participating
    entries of the order (None: all).  boxes fp32 [B,N,7] = (x,y,z,dx,dy,dz,heading).
    Returns (keep int64 [B,P] of slot indices, -1 padded; counts int32 [B])."""
    if not torch.is_tensor(boxes) or boxes.dim() != 3:
        raise L.LisoHipError("boxes must be a [B, N, 7] tensor")
    B, N = boxes.shape[0], boxes.shape[1]
    _need(boxes, "boxes", torch.float32, (B, N, 7))
    _need(sorted_keys, "sorted_keys", torch.int32, (B, N))
    _need(sorted_idx, "sorted_idx", torch.int32, (B, N))
    P = int(post_nms_max)
    if not 1 <= P <= MAX_POST:
        raise L.LisoHipError(f"post_nms_max must be in [1, {MAX_POST}], got {P}")
    pre = 0 if pre_nms_max is None else int(pre_nms_max)
    dev = boxes.device
    keep = torch.empty((B, P), dtype=torch.int64, device=dev)
    counts = torch.empty((B,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        L.check(L.lib().liso_det_nms_select(B, N, _p(boxes), _p(sorted_keys), _p(sorted_idx), float(thresh), pre, P, _p(keep),
                                            _p(counts), L.stream_ptr()), "det_nms select")
    return keep, counts


def gather(keep, counts, srcs, pads):
    """(c) dst[b,p] = src[b, keep[b,p]] for the kept rows, `pad` elsewhere, for every src [B,N,...] of `srcs` (at most 8),
    in one launch.  `pads`: one Python number per src (bool sources: False).  Returns the [B,P,...] tensors."""
    if not torch.is_tensor(keep) or keep.dim() != 2:
        raise L.LisoHipError("keep must be a [B, P] tensor")
    B, P = keep.shape
    _need(keep, "keep", torch.int64, (B, P))
    _need(counts, "counts", torch.int32, (B,))
    if not 1 <= len(srcs) <= MAX_FIELDS or len(pads) != len(srcs):
        raise L.LisoHipError(f"gather takes 1..{MAX_FIELDS} fields, each with a padding value")
    if not 1 <= P <= MAX_POST:
        raise L.LisoHipError(f"P must be in [1, {MAX_POST}], got {P}")
    N = None
    fields = (L.DetGatherField * len(srcs))()
    outs = []
    for i, (s, pad) in enumerate(zip(srcs, pads)):
        if not torch.is_tensor(s) or s.dim() < 2 or s.shape[0] != B:
            raise L.LisoHipError(f"field {i} must be a [B, N, ...] tensor")
        L.require_cuda(s)
        if not s.is_contiguous():
            raise L.LisoHipError(f"field {i} must be contiguous")
        if s.device != keep.device:
            raise L.LisoHipError(f"field {i} is on {s.device}, keep on {keep.device}")
        if N is None:
            N = s.shape[1]
        elif s.shape[1] != N:
            raise L.LisoHipError(f"field {i} has {s.shape[1]} slots, field 0 has {N}")
        row = 1
        for d in s.shape[2:]:
            row *= int(d)
        if row < 1 or s.element_size() not in (1, 2, 4, 8):
            raise L.LisoHipError(f"field {i}: unsupported row shape {tuple(s.shape)} / dtype {s.dtype}")
        dst = torch.empty((B, P) + tuple(s.shape[2:]), dtype=s.dtype, device=s.device)
        bits = torch.tensor([pad], dtype=s.dtype).view(torch.uint8).tolist()  # host-side bytes of the padding value
        fields[i] = L.DetGatherField(_p(s), L.ptr(dst), row, s.element_size(), int.from_bytes(bytes(bits), "little"))
        outs.append(dst)
    if N > MAX_N:
        raise L.LisoHipError(f"N must be <= {MAX_N}")
    with torch.cuda.device(keep.device):
        L.check(L.lib().liso_det_nms_gather(B, N, P, _p(keep), _p(counts), ctypes.cast(fields, ctypes.c_void_p), len(srcs),
                                            L.stream_ptr()), "det_nms gather")
    return outs
