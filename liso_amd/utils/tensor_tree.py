"""Samples are trees of tensors (dicts, lists and tuples around them): the walks over such trees the trainers need, the padding
of a loss cloud, and the byte-packing of many small tensors into one buffer."""
import torch
import torch.nn.functional as F

from liso_amd import _lib as L


def tree_map(obj, fn):
    """the same tree with every tensor replaced by `fn(tensor)`; anything that is no tensor, dict, list or tuple stays"""
    if torch.is_tensor(obj):
        return fn(obj)
    if isinstance(obj, dict):
        return {k: tree_map(v, fn) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return type(obj)(tree_map(v, fn) for v in obj)
    return obj


def tree_pairs(dst, src):
    """[(tensor of dst, its counterpart in src)] in the order `tree_map` visits them; `src` may hold more than `dst`"""
    if torch.is_tensor(dst):
        return [(dst, src)]
    if isinstance(dst, dict):
        return [p for k in dst for p in tree_pairs(dst[k], src[k])]
    if isinstance(dst, (list, tuple)):
        return [p for d, s in zip(dst, src) for p in tree_pairs(d, s)]
    return []


def tree_copy_(dst, src):
    """dst <- src over a tree of tensors: the device-to-device ones as ONE launch (_lib.multi_copy)"""
    pairs = tree_pairs(dst, src)
    if pairs:
        L.multi_copy(pairs)


def tree_signature(obj, skip_dim=None):
    """((shape, dtype) of every tensor): the key of a graph's static inputs.  `skip_dim`: an axis left out of the shapes."""
    return tuple((tuple(d for i, d in enumerate(t.shape) if i != skip_dim), t.dtype) for t, _ in tree_pairs(obj, obj))


def tree_stack(samples):
    """batch of sample dicts (each with batch size 1) -> one sample dict: tensors are concatenated along the batch axis, lists
    (per-sample clouds of different lengths) are chained, anything else is taken from the first sample"""
    first = samples[0]
    if torch.is_tensor(first):
        return torch.cat(list(samples), dim=0) if first.dim() > 0 else first
    if isinstance(first, dict):
        return {k: tree_stack([s_[k] for s_ in samples]) for k in first}
    if isinstance(first, (list, tuple)):
        return type(first)(x for s_ in samples for x in s_)
    return first


def pad_pcl_ta(pa, n):
    """the loss cloud dict `pcl_ta` with its point axis grown to `n` rows the way the dataset's own collate pads it
    (torch_dataset_commons.py:380-431): NaN rows, pcl_is_valid False, pillar_coors -1.  A new dict, or `pa` itself when it has
    `n` rows already."""
    pad = n - pa["pcl"].shape[1]
    if pad == 0:
        return pa
    return {**pa, "pcl": F.pad(pa["pcl"], (0, 0, 0, pad), value=float("nan")),
            "pcl_is_valid": F.pad(pa["pcl_is_valid"], (0, pad), value=False),
            "pillar_coors": F.pad(pa["pillar_coors"], (0, 0, 0, pad), value=-1)}


# ---- many tensors in ONE byte buffer, filled by a single concatenation launch: the inputs of a graph per replay, the outputs of a
# captured body.  A layout is [(name, byte offset, bytes, dtype, shape)]; the two order their segments differently (`packed_statics`).
def _byte_layout(named):
    sizes = [t.numel() * t.element_size() for _, t in named]
    return [(name, sum(sizes[:i]), sizes[i], t.dtype, tuple(t.shape)) for i, (name, t) in enumerate(named)], sum(sizes)


def _bytes(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


def pack_into(flat, layout, tensors):
    """{name: tensor} -> `flat` (the buffer `layout` describes) by ONE torch.cat launch"""
    parts = [_bytes(tensors[name]) for name, *_ in layout]
    assert sum(p_.numel() for p_ in parts) == flat.numel()  # (cat(out=) would silently resize the static buffer)
    torch.cat(parts, out=flat)


def pack(named):
    """[(name, tensor)] -> (flat uint8 tensor = ONE torch.cat launch, layout) with every segment aligned for its dtype: 8-byte types
    first, then 4-byte, then the rest"""
    named = sorted(named, key=lambda nt: -nt[1].element_size())
    return torch.cat([_bytes(t) for _, t in named]), _byte_layout(named)[0]


def unpack(flat, layout):
    return {name: flat[off:off + nbytes].view(dtype).view(shape) for name, off, nbytes, dtype, shape in layout}


def packed_statics(tensors):
    """static copies of a graph's input tensors as typed views of ONE byte buffer: -> (views {name: tensor}, flat uint8 buffer,
    layout) for `pack_into`.  Kernels read these views in place of separately allocated tensors, so segments whose byte size is
    not a multiple of 16 go last (every view then starts 16-B aligned -- `pack`'s order only aligns for the dtype), and when there
    is more than one of them, or a tensor is empty or not contiguous, the copies are separate tensors and the caller refreshes
    them one by one: -> (copies, None, None)."""
    size = lambda t: t.numel() * t.element_size()  # noqa: E731
    named = sorted(tensors.items(), key=lambda nt: size(nt[1]) % 16 != 0)
    if not all(t.is_contiguous() and t.numel() > 0 for _, t in named) or sum(1 for _, t in named if size(t) % 16) > 1:
        return {k: t.clone() for k, t in tensors.items()}, None, None
    layout, total = _byte_layout(named)
    flat = torch.empty(total, dtype=torch.uint8, device=named[0][1].device)
    views = unpack(flat, layout)
    for k, t in named:
        views[k].copy_(t)
    return views, flat, layout
