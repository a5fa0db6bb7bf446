"""The flow wheel (reference liso/visu/flow_image.py): hue from the flow's direction, value from its magnitude over the image's
largest.  Device tensors go through include/liso_visu.h entry 1 (two launches, no host read); numpy arrays run the host path, which
states the same fp32 expressions.  Two consequences of the reference's expressions hold on both paths: an all-zero flow image has
max_mag == 0, mag / max_mag is NaN, NaN < 1 is false and the value becomes 1 (full red, not NaN); a tiny negative angle gives a hue
of exactly 1 and sector 6 % 6 = 0."""
import numpy as np
import torch

from liso_amd import _lib as L
from liso_amd.utils.device_args import is_np, opt_ptr as _p
from liso_amd.visu.color_conversion import hsv2rgb_host


def create_flow_image_host(flow):
    """numpy [B, 2, H, W] -> fp32 rgb [B, 3, H, W]"""
    flow = np.asarray(flow, np.float32)
    assert flow.ndim == 4 and flow.shape[1] == 2, flow.shape
    f32 = np.float32
    two_pi = f32(2.0 * np.pi)
    with np.errstate(invalid="ignore", divide="ignore"):
        mag = np.sqrt(flow[:, 0] * flow[:, 0] + flow[:, 1] * flow[:, 1])
        max_mag = mag.max(axis=(1, 2))
        ang = np.arctan2(flow[:, 1], flow[:, 0])
        hue = np.where(ang >= 0, ang, ang + two_pi) / two_pi
        q = mag / max_mag[:, None, None]
        val = np.where(q < 1.0, q, f32(1.0))
    return hsv2rgb_host(np.stack([hue, np.ones_like(hue), val], axis=1).astype(np.float32))


def pytorch_create_flow_image(flow):
    """flow [B, 2, H, W] -> rgb [B, 3, H, W] fp32 (reference :29-45)"""
    if flow.ndim != 4 or flow.shape[1] != 2:
        raise ValueError(f"flow must be [B, 2, H, W], got {tuple(flow.shape)}")
    if is_np(flow):
        return create_flow_image_host(flow)
    L.require_cuda(flow)
    if flow.dtype != torch.float32:
        raise L.LisoHipError(f"flow must be float32 on the device, got {flow.dtype}")
    flow = flow.contiguous()
    B, _, H, W = flow.shape
    rgb = torch.empty((B, 3, H, W), dtype=torch.float32, device=flow.device)
    max_mag = torch.empty((max(B, 1),), dtype=torch.float32, device=flow.device)
    with torch.cuda.device(flow.device):
        L.check(L.lib().liso_visu_flow_wheel_f32(B, H, W, _p(flow), _p(max_mag), _p(rgb), L.stream_ptr()), "flow wheel")
    return rgb


def log_flow_image(writer, cfg, global_step, flow_2d, prefix="DATA/FLOW_T0_T1/", suffix=""):
    """reference :7-26.  `writer` is any object with `add_images(tag, array, global_step=, dataformats=)`; it receives the first
    `cfg.logging.max_log_img_batches` flow wheels as one NCHW batch.  The reference tiles them into one picture with torchvision's
    `make_grid` first; image grids are out of scope here."""
    if flow_2d.ndim != 4 or flow_2d.shape[1] != 2 or min(flow_2d.shape[2:]) <= 3:  # (a channels-last image would pass for [B, 2, H, W])
        raise ValueError(f"flow_2d must be [B, 2, H, W] with H, W > 3, got {tuple(flow_2d.shape)}")
    flow_img = pytorch_create_flow_image(flow_2d)
    writer.add_images(prefix + suffix, flow_img[: cfg.logging.max_log_img_batches], global_step=global_step, dataformats="NCHW")
