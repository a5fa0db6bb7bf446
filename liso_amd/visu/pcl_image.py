"""Clouds and box centres as bird's-eye images (reference liso/visu/pcl_image.py:7-157).

numpy arrays run the host path of this file; device tensors go through include/liso_visu.h (entries 2 and 3) without a host read,
provided grid sizes come as host integers and extents as device tensors.  Both paths follow the same rules:

* pillar coordinates: trunc(((p + 0.5 * range) / range) * resolution) clamped to [0, resolution - 1], in fp64 for the occupancy
  image (what numpy's promotion gives the reference for the fp64 ranges a config holds); a NaN lands on 0.
* the variable-extent projection scales BOTH axes by the smaller of the two factors grid / (max - min), in fp32, and truncates.
* a point is inside the extent when min + 1 cm < p < max - 1 cm on both axes.
* intensities are re-normalised only when some value of the cloud lies outside [0, 1]: minus the minimum, then over the maximum of
  the shifted values (= max - min).
* several points on one pixel: the reference scatters, which has no defined winner on a GPU.  Here the point with the HIGHEST INDEX
  wins, which is what the reference's scatter does in practice on the CPU.
* the batched form of `create_topdown_f32_pcl_image_variable_extent` takes NaN-padded clouds [B, N, 4]: a row whose x or y is NaN
  is padding, takes no part in the image and none in the minimum and maximum.
"""
import numpy as np
import torch

from liso_amd import _lib as L
from liso_amd.utils.device_args import as_u8, is_np, opt_ptr as _p

EPSILON_M = 0.01  # the inside test's margin


def _hw(img_grid_size):
    """(H, W) as host integers (a device tensor here costs a host read)"""
    v = img_grid_size.tolist() if hasattr(img_grid_size, "tolist") else list(img_grid_size)
    assert len(v) == 2, img_grid_size
    return int(v[0]), int(v[1])


# ---- pillar coordinates ----------------------------------------------------------------------------------------------------------
def pillarize_pointcloud(pcl_np, bev_range_m, pillar_bev_resolution):
    """numpy cloud [N, >=2] -> int32 [N, 2] pillar coordinates (reference :7-19)"""
    assert pcl_np.ndim == 2, pcl_np.shape
    rng = np.asarray(bev_range_m, np.float64)
    res = np.asarray(pillar_bev_resolution)
    with np.errstate(invalid="ignore"):
        coords = (((pcl_np[:, :2].astype(np.float64) + 0.5 * rng) / rng) * res.astype(np.float64)).astype(np.int32)
    return np.maximum(np.minimum(coords, res.astype(np.int32) - 1), 0)


def torch_batched_pillarize_pointcloud(pcl_torch, bev_range_m, pillar_bev_resolution):
    """cloud [B, N, >=2], range [2] and resolution [2] tensors on one device -> (batch index int64 [B, N, 1], pillar coordinates
    int64 [B, N, 2]) (reference :22-43): plain tensor arithmetic in the cloud's dtype, no host read"""
    res = pillar_bev_resolution
    coords = (((pcl_torch[:, :, :2] + 0.5 * bev_range_m) / bev_range_m) * res.to(torch.float32)).to(torch.int32)
    coords = torch.maximum(torch.minimum(coords, res - 1), torch.zeros_like(res))
    B, N = pcl_torch.shape[:2]
    batch = torch.arange(B, device=pcl_torch.device)[:, None, None].expand(B, N, 1)
    return batch.to(torch.long).contiguous(), coords.to(torch.long)


def create_occupancy_pcl_image(pcl, bev_range_m, img_shape, valid=None):
    """points [N, >=2] -> fp32 [H, W, 1], 1 in every pixel that holds a point (reference :46-56).  Extensions: a batch [B, N, >=2]
    gives [B, H, W, 1]; `valid` [.., N] leaves rows out (box centres of a padded Shape)."""
    H, W = _hw(img_shape)
    if is_np(pcl):
        if pcl.ndim == 3:
            return np.stack([create_occupancy_pcl_image(pcl[b], bev_range_m, img_shape, None if valid is None else valid[b])
                             for b in range(pcl.shape[0])])
        rows = pcl if valid is None else pcl[np.asarray(valid, bool)]
        img = np.zeros((H, W, 1), np.float32)
        rc = pillarize_pointcloud(rows, bev_range_m, np.array([H, W]))
        img[rc[:, 0], rc[:, 1]] = 1.0
        return img
    L.require_cuda(pcl)
    unb = pcl.dim() == 2
    p3 = (pcl[None] if unb else pcl).to(torch.float64).contiguous()
    if p3.dim() != 3 or p3.shape[-1] < 2:
        raise L.LisoHipError(f"points must be [N, >=2] or [B, N, >=2], got {tuple(pcl.shape)}")
    B, N, C = p3.shape
    if valid is not None:
        valid = as_u8(valid.reshape(B, N), convert=True)
    rng = [float(v) for v in (bev_range_m.tolist() if hasattr(bev_range_m, "tolist") else bev_range_m)]
    img = torch.empty((B, H, W, 1), dtype=torch.float32, device=p3.device)
    with torch.cuda.device(p3.device):
        L.check(L.lib().liso_visu_occupancy_f64(B, N, C, H, W, rng[0], rng[1], _p(p3), _p(valid), _p(img), L.stream_ptr()), "occupancy image")
    return img[0] if unb else img


# ---- variable extent ---------------------------------------------------------------------------------------------------------------
def _factor_host(coords_min, coords_max, H, W):
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.array([H, W], np.float32) / (coords_max - coords_min)
    return f.min()  # (numpy's min carries a NaN, as torch's)


def project_2d_pcl_to_rowcol_nonsquare_bev_range(pcl_2d, coords_min, coords_max, img_grid_size):
    """[N, 2] metres -> [N, 2] fractional (row, col): (p - min) * f with ONE f = min(grid / (max - min)) for both axes (reference
    :140-157).  numpy in, numpy out (fp32); tensors in, tensor out by plain tensor arithmetic."""
    if is_np(pcl_2d):
        H, W = _hw(img_grid_size)
        lo, hi = np.asarray(coords_min, np.float32), np.asarray(coords_max, np.float32)
        with np.errstate(invalid="ignore"):
            return (pcl_2d.astype(np.float32) - lo) * _factor_host(lo, hi, H, W)
    grid = torch.as_tensor(img_grid_size, device=pcl_2d.device) if not torch.is_tensor(img_grid_size) else img_grid_size.to(pcl_2d.device)
    return (pcl_2d - coords_min) * (grid / (coords_max - coords_min)).min()


def get_linear_bev_idx(pcl, coords_min, coords_max, img_grid_size):
    """cloud [N, >=2] -> (inside the extent by the 1 cm margin: bool [N], row * W + col after truncation: int64 [N]) (reference
    :114-137); the index of a point outside the extent means nothing"""
    H, W = _hw(img_grid_size)
    rowcol = project_2d_pcl_to_rowcol_nonsquare_bev_range(pcl[:, :2], coords_min, coords_max, (H, W))
    if is_np(pcl):
        lo, hi = np.asarray(coords_min, np.float32), np.asarray(coords_max, np.float32)
        p = pcl[:, :2].astype(np.float32)
        with np.errstate(invalid="ignore"):
            inside = np.all(lo + np.float32(EPSILON_M) < p, axis=-1) & np.all(p < hi - np.float32(EPSILON_M), axis=-1)
            rc = np.where(np.isfinite(rowcol), rowcol, 0).astype(np.int64)
        return inside, rc[:, 0] * W + rc[:, 1]
    p = pcl[:, :2]
    inside = torch.all(coords_min + EPSILON_M < p, dim=-1) & torch.all(p < coords_max - EPSILON_M, dim=-1)
    rc = rowcol.long()
    return inside, rc[:, 0] * W + rc[:, 1]


def _topdown_one_host(pcl, intensity, lo, hi, H, W):
    pcl, intensity = np.asarray(pcl, np.float32), np.asarray(intensity, np.float32)
    real = ~(np.isnan(pcl[:, 0]) | np.isnan(pcl[:, 1]))
    if real.any() and not np.all(np.isnan(intensity[real])):
        i_lo, i_hi = np.nanmin(intensity[real]), np.nanmax(intensity[real])
        if i_lo < 0.0 or i_hi > 1.0:
            with np.errstate(invalid="ignore", divide="ignore"):
                intensity = (intensity - i_lo) / (i_hi - i_lo)
    inside, lin = get_linear_bev_idx(pcl, lo, hi, (H, W))
    with np.errstate(invalid="ignore"):
        rc = project_2d_pcl_to_rowcol_nonsquare_bev_range(pcl[:, :2], lo, hi, (H, W))
        rc = np.where(np.isfinite(rc), rc, -1).astype(np.int64)
    keep = inside & real & (rc[:, 0] >= 0) & (rc[:, 0] < H) & (rc[:, 1] >= 0) & (rc[:, 1] < W)  # (a pixel outside the image is dropped)
    img, occ = np.zeros(H * W, np.float32), np.zeros(H * W, bool)
    img[lin[keep]] = intensity[keep]  # (numpy assigns a repeated index its last value: the highest point index wins)
    occ[lin[keep]] = True
    return img.reshape(H, W), occ.reshape(H, W)


def create_topdown_f32_pcl_image_variable_extent(pcl, intensity, coords_min, coords_max, img_grid_size):
    """cloud [N, 4] with intensity [N] -> (intensity image fp32 [H, W], pixel is occupied bool [H, W]) over the extent coords_min ..
    coords_max (reference :59-111); NaN-padded clouds [B, N, 4] with intensity [B, N] -> [B, H, W] each.  Rules in the module
    docstring.  Device: three launches; `coords_min` / `coords_max` as device tensors keep it free of host copies."""
    H, W = _hw(img_grid_size)
    assert pcl.shape[-1] == 4 and tuple(intensity.shape) == tuple(pcl.shape[:-1]), (pcl.shape, intensity.shape)
    if is_np(pcl):
        lo, hi = np.asarray(coords_min, np.float32), np.asarray(coords_max, np.float32)
        if pcl.ndim == 2:
            return _topdown_one_host(pcl, intensity, lo, hi, H, W)
        res = [_topdown_one_host(pcl[b], intensity[b], lo, hi, H, W) for b in range(pcl.shape[0])]
        return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])
    L.require_cuda(pcl, intensity)
    if pcl.dtype != torch.float32 or intensity.dtype != torch.float32:
        raise L.LisoHipError("cloud and intensity must be float32 on the device")
    unb = pcl.dim() == 2
    p3 = (pcl[None] if unb else pcl).contiguous()
    inten = (intensity[None] if unb else intensity).contiguous()
    B, N, C = p3.shape
    dev = p3.device
    extent = torch.cat([torch.as_tensor(coords_min, dtype=torch.float32, device=dev).reshape(2),
                        torch.as_tensor(coords_max, dtype=torch.float32, device=dev).reshape(2)])
    img = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    occ = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
    nbytes = L.lib().liso_visu_topdown_workspace_bytes(max(B, 1), H, W)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        L.check(L.lib().liso_visu_topdown_f32(B, N, C, H, W, _p(p3), _p(inten), _p(extent), _p(img), _p(occ), _p(ws), nbytes, L.stream_ptr()),
                "top-down image")
    occ = occ.view(torch.bool)
    return (img[0], occ[0]) if unb else (img, occ)
