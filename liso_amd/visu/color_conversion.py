"""HSV -> RGB by the usual sector formula, for [B, 3, H, W] images with all three channels in [0, 1]:

    chroma = value * saturation,  k = 6 * hue,  second = chroma * (1 - |k mod 2 - 1|),  sector = trunc(k) mod 6

Each sector places (chroma, second, 0) on the three colour channels in its own order (`_ORDER`), and value - chroma is added to
all of them.  A hue of exactly 1 gives sector 6 mod 6 = 0, the same red as hue 0.  Arithmetic stays in the input's float dtype,
one operation at a time, which is what the flow-wheel kernel (include/liso_visu.h entry 1) evaluates per pixel."""
import numpy as np
import torch

# _ORDER[sector][channel]: which of (chroma, second, zero) = (0, 1, 2) the channel takes
_ORDER = ((0, 1, 2), (1, 0, 2), (2, 0, 1), (2, 1, 0), (1, 2, 0), (0, 2, 1))


def hsv2rgb_host(hsv):
    """numpy [B, 3, H, W] -> [B, 3, H, W] in the input's float dtype"""
    hsv = np.asarray(hsv)
    one, two, six = (hsv.dtype.type(v) for v in (1.0, 2.0, 6.0))
    hue, sat, val = hsv[:, 0], hsv[:, 1], hsv[:, 2]
    with np.errstate(invalid="ignore"):
        chroma = val * sat
        k = hue * six
        second = chroma * (one - np.abs(np.fmod(k, two) - one))
        rest = val - chroma
        sector = np.nan_to_num(k, nan=0.0).astype(np.uint8) % 6
    parts = np.stack([chroma, second, np.zeros_like(chroma)], axis=0)  # [3, B, H, W]
    pick = np.asarray(_ORDER, np.int64)[sector]  # [B, H, W, 3]
    rgb = np.take_along_axis(parts, np.moveaxis(pick, -1, 0), axis=0)  # [3, B, H, W]
    return np.moveaxis(rgb, 0, 1) + rest[:, None]


def hsv2rgb(hsv):
    """numpy array or tensor (host or device) [B, 3, H, W] -> rgb of the same kind.  The tensor form is plain torch arithmetic with
    no host read; the flow wheel does not come through here but through its own kernel (flow_image.pytorch_create_flow_image)."""
    if isinstance(hsv, np.ndarray):
        return hsv2rgb_host(hsv)
    hue, sat, val = hsv[:, 0], hsv[:, 1], hsv[:, 2]
    chroma = val * sat
    k = hue * 6.0
    second = chroma * (1.0 - torch.abs(torch.remainder(k, 2.0) - 1.0))
    sector = k.to(torch.uint8).to(torch.int64) % 6
    parts = torch.stack([chroma, second, torch.zeros_like(chroma)], dim=1)  # [B, 3, H, W]
    pick = torch.tensor(_ORDER, dtype=torch.int64, device=hsv.device)[sector].permute(0, 3, 1, 2)  # [B, 3, H, W]
    return torch.gather(parts, 1, pick) + (val - chroma)[:, None]
