"""JCP range-image ground removal (reference liso/jcp/jcp.py:253-384) on the device and on the host.

`JPCGroundRemove` keeps the reference's keyword-only signature.  Its result is defined as the reference's function applied to the
float64 widening of the cloud, quirks included (include/liso_ground.h lists them).  Device tensors go through
liso_ground_jcp_f32 (liso_amd/csrc/ground_jcp.hip) without a host synchronisation; numpy arrays and CPU tensors run the numpy
host path below, which is vectorised wherever the reference's loop order does not matter (projection, the column scans across
columns, dilation, the 24 weights) and keeps the loop where it does (positions within a column, the raster-order JCP pass).
The host path is also what the full-size device tests compare against, and it can return its intermediates and decision
margins (`jcp_host(..., debug=True)`).

`remove_ground_points` is the device form of `remove_ground_points_from_sample` (torch_dataset_commons.py:1165-1185): JCP label
OR cone label, then an order-preserving compaction into a NaN-padded batch with per-cloud counts.
"""
import ctypes
import math

import numpy as np
import torch

from liso_amd import _lib as L
from liso_amd.utils.device_args import as_u8, cloud3, counts_arg, opt_ptr as _p

MIN_RANGE, MAX_RANGE, TH_G, SIGMA_DEG = 3.0, 70.0, 0.3, 7.0
MAX_HEIGHT, MAX_PIXELS = 1024, 1 << 24  # LISO_GROUND_MAX_HEIGHT, LISO_GROUND_MAX_PIXELS
N_STAGES = 7  # LISO_GROUND_N_STAGES
STAGES = ("init", "elevation", "projection", "recm", "candidates", "resolve", "gather")
EMPTY, GROUND, OBSTACLE, CANDIDATE = 0, 1, 2, 3
# the reference's neighborx_ / neighbory_: the 5x5 window in raster order without its centre
NEIGHBOR_DROW = np.array([w // 5 - 2 for w in range(25) if w != 12])
NEIGHBOR_DCOL = np.array([w % 5 - 2 for w in range(25) if w != 12])


def _region_length(delta_R):
    length = int((MAX_RANGE - MIN_RANGE) / delta_R)
    if length > 255:
        raise ValueError(f"delta_R={delta_R}: int(67 / delta_R) = {length} > 255 regions, the reference's uint8 region image would wrap")
    if length < 1:
        raise ValueError(f"delta_R={delta_R}: no region fits into the 3..70 m range")
    return length


def _check_image(width, height):
    width, height = int(width), int(height)
    if width < 1 or height < 1 or height > MAX_HEIGHT or width * height > MAX_PIXELS:
        raise ValueError(f"range image {width}x{height}: need 1 <= height <= {MAX_HEIGHT} and width * height <= {MAX_PIXELS}")
    if (height - 1) * height + width - 1 >= width * height:
        raise ValueError(f"range image {width}x{height}: the candidate filter's transposed read cloud_index_[row * H + col] leaves the table")
    return width, height


def _frac_dist(v, use):
    """per element the distance of `v` from an integer; inf where `use` is False or `v` is not finite"""
    with np.errstate(invalid="ignore"):
        d = np.abs(v - np.rint(v))
    return np.where(use & np.isfinite(v), d, np.inf)


def jcp_host(pcl, range_img_width, range_img_height, sensor_height, delta_R, debug=False):
    """numpy [N,3] (any float dtype, widened to float64) -> bool [N]; with `debug` also a dict of intermediates in the numbering
    of the valid (NaN-free) rows: cloud_index [W*H] (col * H + row), region_minz [W*length] after RECM, candidates [K,2] (row, col)
    in visiting order, labels image, margins |score_r - score_g| per candidate, RECM branch counts and the near-tie figures
    (index_frac [n]: per row the distance of its row / column / region value from an integer); and stage by stage: row / col [n]
    (col negative for y == -0.0, x < 0), kept (the rows that take part in the projection), min_ele / max_ele, region_minz_raw
    (before RECM), labels_recm (before the dilation), labels_candidates (after the candidate filter), weights [K,24]."""
    W, H = _check_image(range_img_width, range_img_height)
    delta_R, sensor_height = float(delta_R), float(sensor_height)
    length = _region_length(delta_R)
    full = np.asarray(pcl)
    assert full.ndim == 2 and full.shape[-1] == 3, full.shape
    full = full.astype(np.float64)
    valid = ~np.isnan(full).any(axis=-1)
    out = np.zeros(full.shape[0], bool)
    p = full[valid]
    n = p.shape[0]
    if n == 0:
        return (out, None) if debug else out
    x, y, z = p[:, 0], p[:, 1], p[:, 2]

    # ---- range-image indices (jcp.py:273-305)
    with np.errstate(invalid="ignore", divide="ignore"):
        angle = np.arctan2(y, x)
        angle = np.where(y < 0, angle + 2 * np.pi, angle)
        r_xy = np.sqrt(x * x + y * y)
        a = z / np.maximum(r_xy, 1e-6)
        a = np.where(a > 1.0, 1.0, np.where(a < -1.0, -1.0, a))
        ele = np.arcsin(a)
        finite = np.isfinite(ele)
        if finite.any():
            max_ele, min_ele = np.max(ele[finite]), np.min(ele[finite])
        else:
            max_ele = min_ele = np.nan
        row_f = H * (ele - min_ele) / (max_ele - min_ele)
        col_f = (W - 1) * (angle * 180.0 / np.pi) / 360.0
        row = np.clip(row_f.astype(np.int32), 0, H - 1).astype(np.int64)
        col = col_f.astype(np.int32).astype(np.int64)

    # ---- RangeProjection (:26-56): the never-true bounds tests and z clause are left out.  col < 0 holds for y == -0.0 with
    # x < 0 (angle -pi, not lifted by 2 pi): no projection, and the label is read below at column W + col.
    skip = (r_xy < MIN_RANGE) | (r_xy > MAX_RANGE) | (col < 0) | ((x < 3) & (x > -2) & (y < 1.5) & (y > -1.5))
    kept = np.nonzero(~skip)[0]
    region_f = (r_xy[kept] - MIN_RANGE) / delta_R
    region = region_f.astype(np.int64)
    cloud_index = np.full(W * H, -1, np.int64)
    np.maximum.at(cloud_index, col[kept] * H + row[kept], kept)  # last writer in index order
    minz = np.full(W * length, 100.0)
    ri = col[kept] * length + region  # flat: region == length (r == 70) lands in the next column, as in the reference
    in_table = ri < W * length  # in the last column that is one past the table: no update (include/liso_ground.h)
    np.minimum.at(minz, ri[in_table], z[kept][in_table])
    minz_raw = minz.copy()

    # ---- RECM (:75-105), all columns at once, positions in order
    m = minz.reshape(W, length)
    ground_level = sensor_height + TH_G
    branch = {"hole_before_first": 0, "hole_after_first": 0, "smoothed": 0, "second_scan_lowered": 0}
    flag = np.zeros(W, bool)
    m[:, 0] = np.where(ground_level < m[:, 0], ground_level, m[:, 0])
    for j in range(1, length - 1):
        v = m[:, j].copy()
        hole = v == 100
        first = hole & ~flag
        filled = hole & flag
        v[filled] = m[filled, j - 1]
        flag |= ~first
        smooth = ~first & (np.abs(v - m[:, j - 1]) > 0.5) & (np.abs(v - m[:, j + 1]) > 0.5)
        v[smooth] = (m[smooth, j - 1] + m[smooth, j + 1]) / 2
        v[first] = ground_level
        m[:, j] = v
        branch["hole_before_first"] += int(first.sum())
        branch["hole_after_first"] += int(filled.sum())
        branch["smoothed"] += int(smooth.sum())
    step = delta_R * math.tan(SIGMA_DEG * np.pi / 180)
    pre_th = np.where(sensor_height < m[:, 0], sensor_height, m[:, 0])
    for j in range(1, length):
        cand = pre_th + step
        lower = cand < m[:, j]
        branch["second_scan_lowered"] += int(lower.sum())
        pre_th = np.where(lower, cand, m[:, j])
        m[:, j] = pre_th
    minz = m.reshape(-1)

    # ---- per-pixel ground / obstacle (:107-116); label images are [H, W]
    widx = cloud_index.reshape(W, H).T  # [H, W] view of the winner table
    has = widx >= 0
    lab = np.zeros((H, W), np.uint8)
    rr, cc = np.nonzero(has)
    win = widx[rr, cc]
    win_region = ((r_xy[win] - MIN_RANGE) / delta_R).astype(np.int64)
    th = minz[np.minimum(cc * length + win_region, W * length - 1)]
    lab[rr, cc] = np.where(z[win] >= th + TH_G, OBSTACLE, GROUND)
    lab_recm = lab.copy()

    # ---- 5x5 cross dilation of the obstacle channel, candidates, the transposed filter (:339-367)
    obst = lab == OBSTACLE
    reach = obst.copy()
    for o in (1, 2):
        reach[:, o:] |= obst[:, :-o]
        reach[:, :-o] |= obst[:, o:]
        reach[o:, :] |= obst[:-o, :]
        reach[:-o, :] |= obst[o:, :]
    rel_r, rel_c = np.nonzero((lab == GROUND) & reach)  # row-major
    has_valid = cloud_index[rel_r * H + rel_c] != -1
    lab[rel_r[~has_valid], rel_c[~has_valid]] = OBSTACLE
    cand_r, cand_c = rel_r[has_valid], rel_c[has_valid]
    lab[cand_r, cand_c] = CANDIDATE
    K = cand_r.shape[0]
    lab_cand = lab.copy()

    # ---- the 24 weights of every candidate (:184-230): they do not depend on the labels
    ny = cand_r[:, None] + NEIGHBOR_DROW[None]
    nx = cand_c[:, None] + NEIGHBOR_DCOL[None]
    inside = (nx >= 0) & (nx < W) & (ny >= 0) & (ny < H)
    nyc, nxc = np.clip(ny, 0, H - 1), np.clip(nx, 0, W - 1)
    npt = np.where(inside, widx[nyc, nxc], -1)
    d3 = p[widx[cand_r, cand_c]][:, None, :] - p[np.maximum(npt, 0)]
    dist = np.sqrt(d3[..., 0] * d3[..., 0] + d3[..., 1] * d3[..., 1] + d3[..., 2] * d3[..., 2])
    D = np.where((npt >= 0) & ~(dist > 3), np.exp(-5 * dist), 0.0)
    sumD = np.zeros(K)
    for i in range(24):
        sumD = sumD + D[:, i]
    Wt = D / np.maximum(sumD, 1e-6)[:, None]

    # ---- JCP (:184-249): candidates in row-major order, the image updated in place
    padded = np.zeros((H + 4, W + 4), np.uint8)
    padded[2:-2, 2:-2] = lab
    flat = padded.reshape(-1).tolist()
    PW = W + 4
    offs = [int(dr * PW + dc) for dr, dc in zip(NEIGHBOR_DROW, NEIGHBOR_DCOL)]
    margins = np.zeros(K)
    wl = Wt.tolist()
    for k, (r0, c0) in enumerate(zip(cand_r.tolist(), cand_c.tolist())):
        centre = (r0 + 2) * PW + c0 + 2
        score_r = score_g = 0.0
        w = wl[k]
        for i in range(24):
            lbl = flat[centre + offs[i]]
            if lbl == OBSTACLE:
                score_r += w[i]
            elif lbl == GROUND:
                score_g += w[i]
        flat[centre] = OBSTACLE if score_r > score_g else GROUND
        margins[k] = abs(score_r - score_g)
        if debug and score_r == score_g and score_r != 0.0:
            margins[k] = -1.0  # an exact tie that is not 0 vs 0
    lab = np.asarray(flat, np.uint8).reshape(H + 4, W + 4)[2:-2, 2:-2]

    out[valid] = lab[row, col] == GROUND  # a negative column wraps, as in the reference
    if not debug:
        return out
    nonzero = margins[margins > 0]
    # pre-truncation row / column / region values; rows within 1e-9 of 0 or H clip to the same index from either side
    index_frac = np.minimum(_frac_dist(row_f, ~((np.abs(row_f) < 1e-9) | (np.abs(row_f - H) < 1e-9))), _frac_dist(col_f, col_f > 1e-9))
    index_frac[kept] = np.minimum(index_frac[kept], _frac_dist(region_f, region_f > 1e-9))
    info = {
        "cloud_index": cloud_index, "region_minz": minz, "candidates": np.stack([cand_r, cand_c], -1), "labels": lab,
        "margins": margins, "branch": branch,
        "row": row, "col": col, "kept": kept, "min_ele": float(min_ele), "max_ele": float(max_ele), "region_minz_raw": minz_raw,
        "labels_recm": lab_recm, "labels_candidates": lab_cand, "weights": Wt,
        "min_nonzero_margin": float(nonzero.min()) if nonzero.size else float("inf"),
        "exact_ties": int((margins == 0).sum()), "bad_ties": int((margins < 0).sum()),
        "index_frac": index_frac, "min_index_frac": float(index_frac.min()),
    }
    return out, info


# ---- device ---------------------------------------------------------------------------------------------------------------------
def _cfg(p3, width, height, sensor_height, delta_R):
    return L.GroundCfg(p3.shape[0], p3.shape[1], p3.shape[2], int(width), int(height), float(sensor_height), float(delta_R))


def jcp_device(pcl, range_img_width, range_img_height, sensor_height, delta_R, counts=None, stages=None, state=None):
    """float32 device tensor [N,C] or [B,N,C] (x, y, z first; NaN rows are padding) -> bool tensor [N] / [B,N], no host sync.
    `counts` int32 [B]: rows per cloud.  `stages=(begin, end)` runs that range of STAGES only and returns (labels uint8 [B,N],
    workspace); pass the pair back as `state` to go on with the same workspace (scripts/ground_seg_time.py times stage by stage)."""
    p3 = cloud3(pcl)
    counts = counts_arg(counts, p3)
    B, N = p3.shape[0], p3.shape[1]
    cfg = _cfg(p3, range_img_width, range_img_height, sensor_height, delta_R)
    lib = L.lib()
    if state is None:
        ws_bytes = lib.liso_ground_jcp_workspace_bytes(ctypes.byref(cfg))
        out = torch.empty((B, N), dtype=torch.uint8, device=p3.device)
        ws = torch.empty(max(ws_bytes, 256), dtype=torch.uint8, device=p3.device)
    else:
        out, ws = state
    begin, end = (0, N_STAGES) if stages is None else stages
    with torch.cuda.device(p3.device):
        L.check(lib.liso_ground_jcp_stages_f32(ctypes.byref(cfg), _p(p3), _p(counts), _p(out), L.ptr(ws), ws.numel(), int(begin), int(end),
                                               L.stream_ptr()), "ground jcp")
    if stages is not None:
        return out, ws
    res = out.view(torch.bool)
    return res if pcl.dim() == 3 else res[0]


LAYOUT = ("ele_key", "ele", "pix", "widx", "minz_key", "minz", "lab0", "lab1", "row_cnt", "cols", "wts")  # LISO_GROUND_N_LAYOUT entries


def jcp_tables(state, pcl, range_img_width, range_img_height, sensor_height, delta_R):
    """(labels, workspace) as `jcp_device(..., stages=...)` returns them, for the same cloud and parameters -> dict of tensor views
    into the workspace, named and shaped as include/liso_ground.h lists them (liso_ground_jcp_workspace_layout), plus "labels"
    uint8 [B,N].  The label images come as [B,H,W] without the padding behind them."""
    p3 = cloud3(pcl)
    B, N = p3.shape[0], p3.shape[1]
    W, H = int(range_img_width), int(range_img_height)
    length = _region_length(float(delta_R))
    cfg = _cfg(p3, W, H, sensor_height, delta_R)
    offsets = (ctypes.c_size_t * len(LAYOUT))()
    L.check(L.lib().liso_ground_jcp_workspace_layout(ctypes.byref(cfg), offsets), "ground jcp workspace layout")
    labels, ws = state
    lab_stride = (W * H + 15) // 16 * 16
    shapes = {"ele_key": (torch.int64, (B, 2)), "ele": (torch.float64, (B, N)), "pix": (torch.int32, (B, N)), "widx": (torch.int32, (B, W * H)),
              "minz_key": (torch.int32, (B, W * length)), "minz": (torch.float64, (B, W * length)), "lab0": (torch.uint8, (B, lab_stride)),
              "lab1": (torch.uint8, (B, lab_stride)), "row_cnt": (torch.int32, (B, H)), "cols": (torch.int32, (B, H, W)),
              "wts": (torch.float64, (B, H, W, 24))}
    out = {"labels": labels}
    for name, off in zip(LAYOUT, offsets):
        dtype, shape = shapes[name]
        nbytes = math.prod(shape) * torch.empty((), dtype=dtype).element_size()
        out[name] = ws[off:off + nbytes].view(dtype).view(shape)
    for name in ("lab0", "lab1"):
        out[name] = out[name][:, : W * H].view(B, H, W)
    return out


def unkey_f64(keys):
    """ordered uint64 keys (read as int64 numpy) -> the float64 values"""
    k = np.asarray(keys).astype(np.int64).view(np.uint64)
    neg = (k >> np.uint64(63)) == 0  # the key of a negative value has its top bit clear
    return np.where(neg, ~k, k & np.uint64(0x7FFFFFFFFFFFFFFF)).astype(np.uint64).view(np.float64)


def unkey_f32(keys):
    """ordered uint32 keys (read as int32 numpy) -> the float32 values"""
    k = np.asarray(keys).astype(np.int32).view(np.uint32)
    neg = (k >> np.uint32(31)) == 0
    return np.where(neg, ~k, k & np.uint32(0x7FFFFFFF)).astype(np.uint32).view(np.float32)


def cone_device(pcl, cone_z_threshold__m, cone_angle__deg, counts=None, or_with=None):
    """the cone test in fp64 on the device, OR-ed with `or_with` (bool, same leading shape); invalid rows are False"""
    p3 = cloud3(pcl)
    counts = counts_arg(counts, p3)
    B, N = p3.shape[0], p3.shape[1]
    slope = float(np.tan(cone_angle__deg / 180.0 * np.pi)) if cone_angle__deg > 0.0 else 0.0
    if or_with is not None:
        if or_with.dtype != torch.bool or or_with.numel() != B * N or or_with.device != p3.device:
            raise L.LisoHipError("or_with must be a bool tensor of the cloud's leading shape on its device")
        or_with = as_u8(or_with)
    out = torch.empty((B, N), dtype=torch.uint8, device=p3.device)
    with torch.cuda.device(p3.device):
        L.check(L.lib().liso_ground_cone_f32(B, N, p3.shape[2], _p(p3), _p(counts), float(cone_z_threshold__m), slope, _p(or_with), _p(out),
                                             L.stream_ptr()), "ground cone")
    res = out.view(torch.bool)
    return res if pcl.dim() == 3 else res[0]


def remove_ground_points(pcl, *, range_img_width, range_img_height, sensor_height, delta_R, cone=(-1.70, 0.8), counts=None):
    """float32 device tensor [N,C] or [B,N,C] -> (pcl_no_ground [.., N, C] with the kept rows first, in order, NaN behind them;
    counts int32 [B]; is_ground bool [.., N] = JCP label | cone label).  `cone` = (cone_z_threshold__m, cone_angle__deg) or None
    for the JCP label alone.  Nothing is read back: the call can be captured in a hipGraph."""
    p3 = cloud3(pcl)
    counts = counts_arg(counts, p3)
    B, N, C = p3.shape
    is_ground = jcp_device(p3, range_img_width, range_img_height, sensor_height, delta_R, counts=counts)
    if cone is not None:
        is_ground = cone_device(p3, cone[0], cone[1], counts=counts, or_with=is_ground)
    out = torch.empty((B, N, C), dtype=torch.float32, device=p3.device)
    kept = torch.empty((B,), dtype=torch.int32, device=p3.device)
    lib = L.lib()
    ws_bytes = lib.liso_ground_compact_workspace_bytes(B, N)
    ws = torch.empty(max(ws_bytes, 256), dtype=torch.uint8, device=p3.device)
    with torch.cuda.device(p3.device):
        L.check(lib.liso_ground_compact_f32(B, N, C, _p(p3), _p(counts), _p(as_u8(is_ground)), _p(out), L.ptr(kept),
                                            L.ptr(ws) if N else None, ws_bytes, L.stream_ptr()), "ground compact")
    if pcl.dim() == 2:
        return out[0], kept, is_ground[0]
    return out, kept, is_ground


def JPCGroundRemove(*, pcl, range_img_width, range_img_height, sensor_height, delta_R):
    """reference jcp.py:253-384.  numpy [N,3] -> numpy bool [N] (host path); CPU tensor -> CPU bool tensor (host path);
    device tensor [N,3] or [B,N,3] float32 -> device bool tensor of the same leading shape, without synchronising."""
    assert pcl.shape[-1] == 3, pcl.shape
    if torch.is_tensor(pcl):
        if pcl.is_cuda:
            _check_image(range_img_width, range_img_height)
            _region_length(float(delta_R))
            return jcp_device(pcl, range_img_width, range_img_height, sensor_height, delta_R)
        clouds = pcl if pcl.dim() == 3 else pcl[None]
        res = torch.from_numpy(np.stack([jcp_host(c.numpy(), range_img_width, range_img_height, sensor_height, delta_R) for c in clouds])
                               if clouds.shape[0] else np.zeros(clouds.shape[:2], bool))
        return res if pcl.dim() == 3 else res[0]
    return jcp_host(pcl, range_img_width, range_img_height, sensor_height, delta_R)
