"""Box-snippet augmentation of a whole batch on the device, the random draws included (include/liso_augment.h, the batched entries;
liso_amd/csrc/box_augment_batch.hip, philox_draws.h).

`BoxAugmenter` (box_augmentation.py) pastes into one sweep at a time and makes its draws on the host in the reference's order: it
keeps the fixture parity and costs host work and device reads per sweep.  This module is the training-rate path: one call pastes into
B sweeps, makes no host read and is capturable; every draw is a pure function of (seed, call number, sample id, object slot,
purpose, element) through Philox4x32-10, so a sample's augmentation does not depend on the batch it rides in and every replay of a
captured call draws afresh (the call number lives in device memory and the call's last launch advances it).

The draws follow the reference (liso/datasets/torch_dataset_commons.py:1531-1690) in DISTRIBUTION, not in generator stream.
Deviations, all deliberate:
  * locations: up to 32 independent attempts per object, each a uniform index among the free cells, accepted when it differs from
    every earlier object's index; an object that finds none is left out (the reference permutes all free cells and raises when
    there are too few);
  * point drop-out keeps a uniform random subset of `num_keep` rows IN DATABASE ORDER (the reference permutes the rows);
  * heading: fp64 theta = 2 pi (u - 1/2) with an own fp64 sine / cosine (the reference evaluates them in fp32);
  * the resolution ray-drop, which the reference computes and discards, is not built;
  * a pasted object whose kept rows do not fit into the output's capacity is dropped whole and counted in `overflow`.
Kept reference behaviour: no z shift of the pasted points (`t_z=None`), fp64 pose arithmetic rounded once to fp32.

`paste_snippets_batch_host` restates the whole call in numpy, operation by operation; the device results equal it bit for bit.
"""
import ctypes
import ctypes.util
from fractions import Fraction

import numpy as np
import torch

from liso_amd import _lib as L
from liso_amd.datasets.box_augmentation import BoxSnippetDb
from liso_amd.kabsch.shape_utils import Shape
from liso_amd.utils.device_args import opt_ptr

MAX_OBJS, MAX_ATTEMPTS, DRAW_COLS = 64, 32, 16  # LISO_AUGMENT_MAX_OBJS / _MAX_ATTEMPTS / _DRAW_COLS
SELECT_ALL, SELECT_DROPOUT, SELECT_RAYDROP = 0, 1, 2
SLOT_UNUSED, SLOT_PASTED, SLOT_NO_LOCATION, SLOT_OVERFLOW = 0, 1, 2, 3
# purposes of a draw (philox_draws.h: Purpose)
P_COUNT, P_LOCATION, P_JITTER, P_SNIPPET, P_HEIGHT, P_HEADING, P_FLIP, P_SCALE, P_KEEP, P_NTH, P_START, P_KEY, P_FLOW = range(13)
_PASTE_THREADS = 256  # kThreads of the paste body: fixes the summation order of the box speed

_M32 = np.uint64(0xFFFFFFFF)


# ---- the generator, restated (philox_draws.h) ----------------------------------------------------------------------------------------
def philox4x32(counter, key):
    """Philox4x32-10.  counter [..., 4], key [..., 2] (broadcastable) of 32-bit words -> uint32 [..., 4]"""
    c = [np.asarray(counter)[..., i].astype(np.uint64) & _M32 for i in range(4)]
    k = [np.asarray(key)[..., i].astype(np.uint64) & _M32 for i in range(2)]
    m0, m1, w0, w1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]
        c = [(p1 >> s32) ^ c[1] ^ k[0], p1 & _M32, (p0 >> s32) ^ c[3] ^ k[1], p0 & _M32]
        k = [(k[0] + w0) & _M32, (k[1] + w1) & _M32]
    return np.stack(np.broadcast_arrays(*c), -1).astype(np.uint32)


def _blocks(seed, calls, sample_id, purpose, obj, element):
    seed, calls = int(seed) & (2 ** 64 - 1), int(calls) & (2 ** 64 - 1)
    element = np.asarray(element, np.uint64)
    word1 = (int(purpose) << 27) | (int(obj) << 20) | (int(sample_id) & 0xFFFFF)
    ctr = np.stack([element & _M32, np.full_like(element, word1), np.full_like(element, calls & 0xFFFFFFFF),
                    np.full_like(element, calls >> 32)], -1)
    return philox4x32(ctr, np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint64))


def draw_uniform(seed, calls, sample_id, purpose, obj=0, element=0):
    """the uniform double in [0, 1) of one draw (or of an array of elements)"""
    o = _blocks(seed, calls, sample_id, purpose, obj, element).astype(np.uint64)
    return (((o[..., 0] << np.uint64(32)) | o[..., 1]) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def draw_key32(seed, calls, sample_id, purpose, obj, element):
    return _blocks(seed, calls, sample_id, purpose, obj, element)[..., 0]


def _below(u, n):
    return min(int(u * float(n)), int(n) - 1)


_SIN_COEF = [-1.0 / 355687428096000.0, 1.0 / 1307674368000.0, -1.0 / 6227020800.0, 1.0 / 39916800.0, -1.0 / 362880.0, 1.0 / 5040.0,
             -1.0 / 120.0, 1.0 / 6.0]
_COS_COEF = [1.0 / 20922789888000.0, -1.0 / 87178291200.0, 1.0 / 479001600.0, -1.0 / 3628800.0, 1.0 / 40320.0, -1.0 / 720.0, 1.0 / 24.0, -0.5]


def sincos_turn(u):
    """(sin, cos) of 2 pi (u - 1/2) for u in [0, 1): the routine of philox_draws.h, one numpy operation per fp64 operation"""
    u = np.asarray(u, np.float64)
    u8 = 8.0 * u
    q = u8.astype(np.int64)
    r = u8 - q.astype(np.float64)
    t = 0.78539816339744830962 * r
    t2 = t * t
    p = np.full_like(t, _SIN_COEF[0])
    for coef in _SIN_COEF[1:]:
        p = coef + t2 * p
    S = t * (1.0 - t2 * p)
    c = np.full_like(t, _COS_COEF[0])
    for coef in _COS_COEF[1:]:
        c = coef + t2 * c
    C = 1.0 + t2 * c
    h = 0.70710678118654752440
    odd = (q & 1) == 1
    S, C = np.where(odd, h * (C + S), S), np.where(odd, h * (C - S), C)
    quad = (q >> 1) & 3
    sp = np.select([quad == 0, quad == 1, quad == 2], [S, C, -S], -C)
    cp = np.select([quad == 0, quad == 1, quad == 2], [C, -S, -C], S)
    return -sp, -cp


def _fma_exact(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))  # (Fraction -> float rounds correctly)


def _libm_fma():
    name = ctypes.util.find_library("m")
    if not name:
        return None
    try:
        f = ctypes.CDLL(name).fma
    except (OSError, AttributeError):
        return None
    f.restype, f.argtypes = ctypes.c_double, [ctypes.c_double] * 3
    return f


_FMA = _libm_fma() or _fma_exact


def fma(a, b, c):
    """round(a * b + c), one rounding, elementwise over fp64 arrays (what the paste body's fma() computes)"""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64))
    out = np.empty(a.shape, np.float64)
    flat = out.reshape(-1)
    for i, (x, y, z) in enumerate(zip(a.reshape(-1).tolist(), b.reshape(-1).tolist(), c.reshape(-1).tolist())):
        flat[i] = _FMA(x, y, z)
    return out


# ---- configuration -----------------------------------------------------------------------------------------------------------------
def augment_params(cfg):
    """what the call needs of `cfg.data` (reference :1531-1557): grid, radius, the fp32 range and pillar size, the box block"""
    bc = cfg.data.augmentation.boxes
    rng = np.array(cfg.data.bev_range_m, np.float32)
    grid = np.array(cfg.data.img_grid_size).astype(np.int32)
    size = 1 / (grid / rng).astype(np.float32)
    min_dist = bc.get("min_obj_center_dist_from_occupied_pillars_m", 2.0) if hasattr(bc, "get") else 2.0
    K = int(bc.max_num_objs)
    if not 1 <= K <= MAX_OBJS:
        raise ValueError(f"max_num_objs must be in 1..{MAX_OBJS}, got {K}")
    if bc.use_raydrop_augm:
        selection = SELECT_RAYDROP
    else:
        selection = SELECT_DROPOUT if bc.max_points_dropout != 0.0 else SELECT_ALL
    return {"h": int(grid[0]), "w": int(grid[1]), "radius": max(3, int(min_dist / size.mean())), "K": K, "selection": selection,
            "range": (float(rng[0]), float(rng[1])), "cell": (float(size[0]), float(size[1])),
            "max_scale_delta": float(bc.max_scale_delta), "max_points_dropout": float(bc.max_points_dropout),
            "vmin": float(bc.min_artificial_obj_velo), "vmax": float(bc.max_artificial_obj_velo)}


def default_extra_capacity(db, K):
    """min(K * the largest snippet, P), from the host copy of the offsets: no device read"""
    return max(1, int(min(K * int(db.counts.max()), int(db.offsets[-1]))))


# ---- the numpy restatement -----------------------------------------------------------------------------------------------------------
def free_mask_host(coors, grid_hw, radius):
    """True where no occupied cell lies within the disk (liso_bev_free_mask); rows with a coordinate outside the grid are ignored"""
    H, W = int(grid_hw[0]), int(grid_hw[1])
    coors = np.asarray(coors).reshape(-1, 2)
    ok = (coors[:, 0] >= 0) & (coors[:, 0] < H) & (coors[:, 1] >= 0) & (coors[:, 1] < W)
    occ = np.zeros((H, W), bool)
    occ[coors[ok, 0], coors[ok, 1]] = True
    run = np.concatenate([np.zeros((H, 1), np.int64), np.cumsum(occ, 1)], 1)  # run[:, j] = occupied cells in columns < j
    cols = np.arange(W)
    hit = np.zeros((H, W), bool)
    for dy in range(-radius, radius + 1):
        hw = int(np.floor(np.sqrt(radius * radius - dy * dy)))
        while (hw + 1) ** 2 + dy * dy <= radius * radius:
            hw += 1
        while hw * hw + dy * dy > radius * radius:
            hw -= 1
        lo, hi = np.maximum(cols - hw, 0), np.minimum(cols + hw, W - 1) + 1
        any_in_run = (run[:, hi] - run[:, lo]) > 0  # [H, W]: row y' has an occupied cell in [x - hw, x + hw]
        src = np.arange(H) + dy  # the row y' = y + dy that cell row y looks at
        inside = (src >= 0) & (src < H)
        hit[inside] |= any_in_run[src[inside]]
    return ~hit


def cell_center(i, n, rng):
    """centre of cell i of n along an axis of extent rng (get_voxel_center_coords_m), rounded to fp32 like the stored table"""
    return np.float32(((float(i) + 0.5) / float(n)) * rng + (-0.5 * rng))


def _host_tables(db):
    rows = None
    if db.lidar_rows is not None:
        rows = np.concatenate([np.asarray(r).reshape(-1) for r in db.lidar_rows]).astype(np.int32) if len(db.lidar_rows) else np.zeros(0, np.int32)
    return {"points": db.points.detach().cpu().numpy(), "offsets": np.asarray(db.offsets, np.int64),
            "dims": db.boxes.dims.to(torch.float32).numpy(), "pos_z": db.boxes.pos[:, 2].to(torch.float32).numpy(), "lidar_rows": rows}


def draw_object_count(K, seed, calls, sid):
    """k = 1 + int(u K): how many of the K slots of sample `sid` are used in call `calls`"""
    return 1 + _below(float(draw_uniform(seed, calls, sid, P_COUNT)), K)


def draw_num_keep(n, max_points_dropout, seed, calls, sid, slot):
    """point drop-out: num_keep = max(1, int(n (1 - u max_points_dropout)))"""
    want = float(n) * (1.0 - float(draw_uniform(seed, calls, sid, P_KEEP, slot)) * max_points_dropout)
    return int(want) if want >= 1.0 else 1


def select_rows_host(p, tb, seed, calls, sid, slot, snippet, p1, p2, kept, keep_all):
    """the kept rows of a snippet, ascending, as indices into the snippet"""
    n = int(tb["offsets"][snippet + 1] - tb["offsets"][snippet])
    if p["selection"] == SELECT_DROPOUT and kept < n:
        keys = draw_key32(seed, calls, sid, P_KEY, slot, np.arange(n))
        order = np.lexsort((np.arange(n), keys))  # by key, ties by row
        return np.sort(order[:kept])
    if p["selection"] == SELECT_RAYDROP and not keep_all:
        lidar = tb["lidar_rows"][tb["offsets"][snippet]:tb["offsets"][snippet + 1]].astype(np.int64)
        return np.flatnonzero((lidar - p2) % p1 == 0)
    return np.arange(kept)


def paste_rows_host(points, pose, flow_u, vmin, vmax):
    """the paste body (box_augment_bodies.h: paste_object) for one object: points float32 [n, 4] in the box frame, pose float64 [12],
    flow_u float64 [n, 3] -> (points float32 [n, 4], flow float64 [n, 3] before rounding, box speed float32)"""
    m = [float(v) for v in np.asarray(pose, np.float64).reshape(12)]
    x, y, z = (points[:, i].astype(np.float64) for i in range(3))
    out = np.empty((points.shape[0], 4), np.float32)
    out[:, 0] = (fma(m[2], z, fma(m[1], y, m[0] * x)) + m[3]).astype(np.float32)
    out[:, 1] = (fma(m[6], z, fma(m[4], x, m[5] * y)) + m[7]).astype(np.float32)
    out[:, 2] = (fma(m[10], z, fma(m[8], x, m[9] * y)) + m[11]).astype(np.float32)
    out[:, 3] = points[:, 3]
    span = vmax - vmin
    flow = fma(np.asarray(flow_u, np.float64), span, vmin)
    speed = np.sqrt(fma(flow[:, 2], flow[:, 2], fma(flow[:, 0], flow[:, 0], flow[:, 1] * flow[:, 1])))
    n = points.shape[0]
    if n == 0:
        return out, flow, np.float32(0.0)
    part = np.zeros(_PASTE_THREADS)
    for base in range(0, n, _PASTE_THREADS):  # thread t sums its rows t, t + 256, ... in order
        chunk = speed[base:base + _PASTE_THREADS]
        part[:chunk.shape[0]] = part[:chunk.shape[0]] + chunk
    o = _PASTE_THREADS // 2
    while o > 0:  # the pairwise LDS tree
        part[:o] = part[:o] + part[o:2 * o]
        o //= 2
    return out, flow, np.float32(part[0] / float(n))


def _augment_one_host(p, tb, coors, seed, calls, sid, E, want_flow):
    K, H, W = p["K"], p["h"], p["w"]
    free = free_mask_host(coors, (H, W), p["radius"])
    free_cells = np.flatnonzero(free.reshape(-1))
    num_free = free_cells.shape[0]
    M, P = len(tb["offsets"]) - 1, tb["points"].shape[0]
    u = lambda purpose, obj=0, element=0: float(draw_uniform(seed, calls, sid, purpose, obj, element))  # noqa: E731
    out = {"extra_points": np.full((E, 4), np.nan, np.float32), "extra_flow": np.full((E, 3), np.nan, np.float32),
           "object_offsets": np.zeros(K + 1, np.int32), "box_pos": np.zeros((K, 3), np.float32), "box_dims": np.zeros((K, 3), np.float32),
           "box_rot": np.zeros(K, np.float32), "box_velo": np.zeros(K, np.float32), "box_valid": np.zeros(K, np.uint8),
           "draws": np.zeros((K, DRAW_COLS)), "kept_rows": np.full(E, -1, np.int64), "pose": np.zeros((K, 12)), "free_mask": free}
    k = draw_object_count(K, seed, calls, sid)
    accepted, offset, overflow = [], 0, 0
    for slot in range(K):
        rec = out["draws"][slot]
        rec[0], rec[15] = -1.0, (SLOT_NO_LOCATION if slot < k else SLOT_UNUSED)
        idx = -1
        if slot < k and num_free > 0:
            rec[11] = MAX_ATTEMPTS
            cands = draw_uniform(seed, calls, sid, P_LOCATION, slot, np.arange(MAX_ATTEMPTS))
            for a, ua in enumerate(cands.tolist()):
                cand = _below(ua, num_free)
                if cand not in accepted:
                    idx, rec[11] = cand, a + 1
                    break
        accepted.append(idx)  # (-1 never equals a candidate)
        if idx >= 0:
            cell = int(free_cells[idx])
            ci, cj = divmod(cell, W)
            x = float(cell_center(ci, H, p["range"][0])) + (0.5 - u(P_JITTER, slot, 0)) * p["cell"][0]
            y = float(cell_center(cj, W, p["range"][1])) + (0.5 - u(P_JITTER, slot, 1)) * p["cell"][1]
            snippet = _below(u(P_SNIPPET, slot), M)
            row0 = int(tb["offsets"][snippet])
            n = int(tb["offsets"][snippet + 1]) - row0
            if row0 < 0 or n < 0 or row0 + n > P:
                n = 0
            z = 0.5 * (u(P_HEIGHT, slot) - 0.5) + float(tb["pos_z"][snippet])
            ut = u(P_HEADING, slot)
            theta = 6.283185307179586 * (ut - 0.5)
            sn, cs = (float(v) for v in sincos_turn(ut))
            flip_x = 1.0 if u(P_FLIP, slot, 0) < 0.5 else -1.0
            flip_y = 1.0 if u(P_FLIP, slot, 1) < 0.5 else -1.0
            sx, sy, sz = (1.0 - p["max_scale_delta"] * (2.0 * u(P_SCALE, slot, e) - 1.0) for e in range(3))
            kept, p1, p2, keep_all = n, 0, 0, False
            if p["selection"] == SELECT_RAYDROP:
                p1 = 1 + _below(u(P_NTH, slot), 3)
                p2 = _below(u(P_START, slot), p1)
                lidar = tb["lidar_rows"][row0:row0 + n].astype(np.int64)
                cnt = int(np.count_nonzero((lidar - p2) % p1 == 0))
                keep_all = cnt == 0
                kept = n if keep_all else cnt
            elif p["selection"] == SELECT_DROPOUT:
                p1 = draw_num_keep(n, p["max_points_dropout"], seed, calls, sid, slot)
                kept = min(p1, n)
            pos = np.array([x, y, z]).astype(np.float32)
            fits = offset + kept <= E
            rec[:11] = [cell, snippet, theta, z, flip_x, flip_y, sx, sy, sz, p1, p2]
            rec[12:16] = [x, y, kept, SLOT_PASTED if fits else SLOT_OVERFLOW]
            ax, ay = flip_x * sx, flip_y * sy
            out["pose"][slot] = [cs * ax, -sn * ay, 0.0, float(pos[0]), sn * ax, cs * ay, 0.0, float(pos[1]), 0.0, 0.0, sz, 0.0]
            if fits:
                rows = select_rows_host(p, tb, seed, calls, sid, slot, snippet, p1, p2, kept, keep_all)
                assert rows.shape[0] == kept, (rows.shape, kept)
                flow_u = np.stack([draw_uniform(seed, calls, sid, P_FLOW, slot, 3 * rows + c) for c in range(3)], -1).reshape(kept, 3)
                pts, flow, speed = paste_rows_host(tb["points"][row0 + rows], out["pose"][slot], flow_u, p["vmin"], p["vmax"])
                out["extra_points"][offset:offset + kept] = pts
                out["extra_flow"][offset:offset + kept] = flow.astype(np.float32)
                out["kept_rows"][offset:offset + kept] = row0 + rows
                out["box_pos"][slot], out["box_dims"][slot], out["box_rot"][slot] = pos, tb["dims"][snippet], np.float32(theta)
                out["box_velo"][slot], out["box_valid"][slot] = speed, 1
                offset += kept
            else:
                overflow += 1
        out["object_offsets"][slot + 1] = offset
    out["extra_counts"], out["overflow"] = np.int32(offset), np.int32(overflow)
    if not want_flow:
        del out["extra_flow"]
    return out


def paste_snippets_batch_host(db, pillar_coors, counts, *, cfg, seed, calls=0, sample_ids=None, extra_capacity=None, want_flow=True):
    """The whole batched call in numpy: free mask, draws, point selection, paste.  `pillar_coors` [B, n_max, 2], `counts` [B]; ->
    dict of arrays stacked over the batch: the outputs of `paste_snippets_batch` plus `pose` [B, K, 12] and `free_mask` [B, H, W].
    (`kept_rows` is -1 behind a sample's count here; the device leaves those entries unwritten.)"""
    p, tb = augment_params(cfg), _host_tables(db)
    coors, counts = np.asarray(pillar_coors), np.asarray(counts).reshape(-1)
    B = counts.shape[0]
    assert coors.shape[0] == B and coors.shape[2] == 2, coors.shape
    sample_ids = np.arange(B) if sample_ids is None else np.asarray(sample_ids).reshape(-1)
    E = default_extra_capacity(db, p["K"]) if extra_capacity is None else int(extra_capacity)
    per = [_augment_one_host(p, tb, coors[b, :max(0, min(int(counts[b]), coors.shape[1]))], seed, calls, int(sample_ids[b]), E, want_flow)
           for b in range(B)]
    return {k: np.stack([np.asarray(s[k]) for s in per]) for k in per[0]}


# ---- the device call ---------------------------------------------------------------------------------------------------------------
class DeviceDraws:
    """The generator state of the device draws: an int64 [2] device tensor (seed, calls).  The kernels read it from device memory (a
    kernel argument would be frozen into a captured graph) and the last launch of every call adds 1 to `calls`."""

    def __init__(self, seed, device):
        self.device = torch.device(device)
        self.seed = int(seed)
        self.state = torch.tensor([self.seed, 0], dtype=torch.int64).to(self.device)

    def reset(self, calls=0):
        """set the call number (an asynchronous copy on the current stream: no host synchronisation)"""
        self.state.copy_(torch.tensor([self.seed, int(calls)], dtype=torch.int64), non_blocking=True)
        return self


def _coors3(pillar_coors, counts):
    L.require_cuda(pillar_coors)
    coors = pillar_coors.to(torch.int32).contiguous()
    if coors.dim() == 2:
        coors = coors[None]
    assert coors.dim() == 3 and coors.shape[2] == 2, coors.shape
    B, n_max = coors.shape[0], coors.shape[1]
    if counts is None:
        counts = torch.full((B,), n_max, dtype=torch.int32, device=coors.device)
    counts = counts.to(torch.int32).contiguous()
    assert counts.shape == (B,), counts.shape
    return coors, counts, B, n_max


@torch.no_grad()
def free_location_mask_batch(pillar_coors, counts, grid_hw, radius):
    """-> (free uint8 [B, H, W], row_free_prefix int32 [B, H + 1]): `free_location_mask` of every sample, 4 launches for any B"""
    coors, counts, B, n_max = _coors3(pillar_coors, counts)
    H, W = int(grid_hw[0]), int(grid_hw[1])
    dev = coors.device
    free = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
    prefix = torch.empty((B, H + 1), dtype=torch.int32, device=dev)
    lib = L.lib()
    ws_bytes = int(lib.liso_bev_free_mask_batch_workspace_bytes(B, H, W))
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        L.check(L.TIMER.launch("bev_free_mask_batch", lambda: lib.liso_bev_free_mask_batch(
            opt_ptr(coors if n_max else None), L.ptr(counts), B, n_max, H, W, int(radius), L.ptr(free), L.ptr(prefix), L.ptr(ws), ws_bytes,
            L.stream_ptr())), "bev_free_mask_batch")
    return free, prefix


def _batch_cfg(p, B, n_max, db, E):
    return L.AugmentBatchCfg(B, n_max, p["h"], p["w"], p["radius"], p["K"], len(db), int(db.points.shape[0]), E, p["selection"],
                             p["range"][0], p["range"][1], p["cell"][0], p["cell"][1], p["max_scale_delta"], p["max_points_dropout"],
                             p["vmin"], p["vmax"])


@torch.no_grad()
def paste_snippets_batch(db, pcl, counts, pillar_coors, *, cfg, draws: DeviceDraws, sample_ids=None, extra_capacity=None, want_flow=True):
    """Paste drawn snippets into B sweeps: free mask, draws, point selection and paste in six launches, no host read (capturable).
    `pcl` [B, n_max, C] (only its batch layout is used: `append_clouds` puts the pasted rows behind a cloud), `counts` int32 [B] on the
    device, `pillar_coors` int32 [B, n_max, 2].  -> dict(extra_points [B, E, 4], extra_flow [B, E, 3] (with `want_flow`), extra_counts
    [B], object_offsets [B, K + 1], box_pos / box_dims [B, K, 3], box_rot / box_velo [B, K], box_valid uint8 [B, K], draws float64
    [B, K, 16], overflow int32 [B], kept_rows int64 [B, E]); the columns of `draws`: include/liso_augment.h."""
    p = augment_params(cfg)
    coors, counts, B, n_max = _coors3(pillar_coors, counts)
    if pcl is not None and (pcl.dim() != 3 or pcl.shape[0] != B or pcl.shape[1] != n_max):
        raise L.LisoHipError(f"pcl {tuple(pcl.shape)} does not match pillar_coors {tuple(coors.shape)}")
    dev = coors.device
    if db.points.device != dev or draws.state.device != dev:
        raise L.LisoHipError("the snippet database, the generator state and the sweeps must live on one device")
    tables = db.device_tables()
    if p["selection"] == SELECT_RAYDROP and tables["lidar_rows"] is None:
        raise ValueError("use_raydrop_augm needs the `lidar_rows` of the snippet database")
    P, M = int(db.points.shape[0]), len(db)
    if tables["offsets"].shape != (M + 1,) or tables["dims"].shape != (M, 3) or tables["pos_z"].shape != (M,) or int(db.offsets[-1]) != P \
            or (tables["lidar_rows"] is not None and tables["lidar_rows"].shape != (P,)):
        raise L.LisoHipError("the snippet database's tables do not match its points")
    E = default_extra_capacity(db, p["K"]) if extra_capacity is None else int(extra_capacity)
    if E < 1:
        raise ValueError("extra_capacity must be at least 1")
    K = p["K"]
    if sample_ids is None:
        sample_ids = torch.arange(B, dtype=torch.int64, device=dev)
    sample_ids = sample_ids.to(device=dev, dtype=torch.int64).contiguous()
    assert sample_ids.shape == (B,), sample_ids.shape
    f32, i32 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
    out = {"extra_points": torch.empty((B, E, 4), **f32), "extra_counts": torch.empty((B,), **i32),
           "object_offsets": torch.empty((B, K + 1), **i32), "box_pos": torch.empty((B, K, 3), **f32),
           "box_dims": torch.empty((B, K, 3), **f32), "box_rot": torch.empty((B, K), **f32), "box_velo": torch.empty((B, K), **f32),
           "box_valid": torch.empty((B, K), dtype=torch.uint8, device=dev), "draws": torch.empty((B, K, DRAW_COLS), dtype=torch.float64, device=dev),
           "overflow": torch.empty((B,), **i32), "kept_rows": torch.empty((B, E), dtype=torch.int64, device=dev)}
    if want_flow:
        out["extra_flow"] = torch.empty((B, E, 3), **f32)
    c = _batch_cfg(p, B, n_max, db, E)
    lib = L.lib()
    ws_bytes = int(lib.liso_snippet_augment_batch_workspace_bytes(ctypes.byref(c)))
    if ws_bytes == 0:
        raise L.LisoHipError("the batched augmentation refuses this configuration (grid, radius, max_num_objs, database size)")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        L.check(L.TIMER.launch("snippet_augment_batch", lambda: lib.liso_snippet_augment_batch(
            ctypes.byref(c), opt_ptr(coors if n_max else None), L.ptr(counts), L.ptr(db.points), L.ptr(tables["offsets"]),
            L.ptr(tables["dims"]), L.ptr(tables["pos_z"]), opt_ptr(tables["lidar_rows"]), L.ptr(draws.state), L.ptr(sample_ids),
            L.ptr(out["extra_points"]), opt_ptr(out.get("extra_flow")), L.ptr(out["extra_counts"]), L.ptr(out["object_offsets"]),
            L.ptr(out["box_pos"]), L.ptr(out["box_dims"]), L.ptr(out["box_rot"]), L.ptr(out["box_velo"]), L.ptr(out["box_valid"]),
            L.ptr(out["draws"]), L.ptr(out["overflow"]), L.ptr(out["kept_rows"]), L.ptr(ws), ws_bytes, L.stream_ptr())),
            "snippet_augment_batch")
    return out


@torch.no_grad()
def append_clouds(cloud, counts, extra, extra_counts):
    """-> (out float32 [B, n_max + E, C], out_counts int32 [B]): the first counts[b] rows of cloud[b], the first extra_counts[b] rows of
    extra[b], NaN rows behind; one launch, no host read.  `cloud` [B, n_max, C] and `extra` [B, E, C] float32 (points C = 4, flow C = 3)."""
    L.require_cuda(cloud, extra)
    cloud, extra = cloud.contiguous(), extra.contiguous()
    if cloud.dtype != torch.float32 or extra.dtype != torch.float32 or cloud.dim() != 3 or extra.dim() != 3 or cloud.shape[0] != extra.shape[0] \
            or cloud.shape[2] != extra.shape[2]:
        raise L.LisoHipError(f"append_clouds takes float32 [B, n, C] and [B, E, C], got {tuple(cloud.shape)} and {tuple(extra.shape)}")
    B, n_max, C = cloud.shape
    E = extra.shape[1]
    counts, extra_counts = counts.to(torch.int32).contiguous(), extra_counts.to(torch.int32).contiguous()
    out = torch.empty((B, n_max + E, C), dtype=torch.float32, device=cloud.device)
    out_counts = torch.empty((B,), dtype=torch.int32, device=cloud.device)
    with torch.cuda.device(cloud.device):
        L.check(L.lib().liso_cloud_append_batch(opt_ptr(cloud if n_max else None), L.ptr(counts), opt_ptr(extra if E else None),
                                                L.ptr(extra_counts), B, n_max, E, C, opt_ptr(out if n_max + E else None), L.ptr(out_counts),
                                                L.stream_ptr()), "cloud_append_batch")
    return out, out_counts


class BatchBoxAugmenter:
    """`BoxAugmenter.create_augmented_sample_from_box_snippet_db` for a collated device batch: no host read, capturable with
    `graph_capture.capture`.  `sample_batch` as `assemble_bev_sample` lays it out:
        pcl_ta = {pcl [B, N, 4], pillar_coors [B, N, 2]}, counts int32 [B],
        pcl_full_w_ground_ta / pcl_full_no_ground_ta = {pcl [B, N', 4], counts int32 [B]},
        flow_ta_tb [B, N, 3] (with `need_flow`), sample_ids int64 [B] (optional: 0..B-1)
    -> the reference's dictionary, batched and padded (rows behind a count are NaN / -1): `gt.boxes` a Shape [B, K + P] (pasted slots
    first, then the prediscovered boxes; probs 1; `valid` marks the real ones), the three clouds with the pasted rows appended,
    `pcl_ta` re-cropped by `pillarize_bev` with the flow riding along, `<train_on_box_source>.{boxes, prediscovered_boxes,
    centermaps_*}` through `draw_heat_regression_maps`, and `overflow`."""

    def __init__(self, cfg, db: BoxSnippetDb, need_flow=True, centermaps_output_grid_size=None, seed=0):
        self.cfg, self.db, self.need_flow = cfg, db, need_flow
        self.params = augment_params(cfg)
        self.draws = DeviceDraws(seed, db.points.device)
        grid = np.array(cfg.data.img_grid_size).astype(np.int32)
        self.centermaps_output_grid_size = np.asarray(centermaps_output_grid_size) if centermaps_output_grid_size is not None else grid // 4
        self.extra_capacity = default_extra_capacity(db, self.params["K"])

    @torch.no_grad()
    def __call__(self, sample_batch, prediscovered_boxes: Shape = None):
        from liso_amd.datasets.label_prep import draw_heat_regression_maps
        from liso_amd.datasets.sample_prep import height_range_of, pillarize_bev

        cfg = self.cfg
        ta = sample_batch["pcl_ta"]
        pcl, counts = ta["pcl"], sample_batch["counts"]
        pasted = paste_snippets_batch(self.db, pcl, counts, ta["pillar_coors"], cfg=cfg, draws=self.draws,
                                      sample_ids=sample_batch.get("sample_ids"), extra_capacity=self.extra_capacity, want_flow=self.need_flow)
        B, K = pasted["box_valid"].shape
        extra, extra_counts = pasted["extra_points"], pasted["extra_counts"]
        boxes = Shape(pos=pasted["box_pos"], dims=pasted["box_dims"], rot=pasted["box_rot"][..., None],
                      probs=torch.ones_like(pasted["box_rot"])[..., None], velo=pasted["box_velo"][..., None],
                      valid=pasted["box_valid"].view(torch.bool))
        if prediscovered_boxes is not None:
            pre = prediscovered_boxes
            boxes = boxes.cat(Shape(**{k: (v.to(getattr(boxes, k).dtype) if v is not None else None) for k, v in pre.__dict__.items()}), dim=1)
        else:
            pre = boxes[:, :0]
        cat_pcl, cat_counts = append_clouds(pcl, counts, extra, extra_counts)
        out = {"gt": {"boxes": boxes}, "overflow": pasted["overflow"], "draws": pasted["draws"], "extra_counts": extra_counts}
        for key in ("pcl_full_w_ground_ta", "pcl_full_no_ground_ta"):
            full, full_counts = append_clouds(sample_batch[key]["pcl"], sample_batch[key]["counts"], extra, extra_counts)
            out[key] = {"pcl": full, "counts": full_counts}
        flow = None
        if self.need_flow:
            flow, _ = append_clouds(sample_batch["flow_ta_tb"], counts, pasted["extra_flow"], extra_counts)
        crop = pillarize_bev(cat_pcl, cat_counts, bev_range_m=cfg.data.bev_range_m, img_grid_size=cfg.data.img_grid_size,
                             height_range_m=height_range_of(cfg), flow=flow)
        out["pcl_ta"] = {"pcl": crop["pcl"], "pillar_coors": crop["pillar_coors"]}
        out["counts"] = crop["counts"]
        source = out.setdefault(cfg.data.flow_source, {})
        if self.need_flow:
            source["flow_ta_tb"] = crop["flow"]
        if cfg.network.name not in ("pointrcnn", "pointpillars"):
            if cfg.loss.supervised.centermaps.confidence_target != "gaussian":
                raise NotImplementedError(cfg.loss.supervised.centermaps.confidence_target)
            maps = draw_heat_regression_maps(boxes, self.centermaps_output_grid_size, np.array(cfg.data.bev_range_m, np.float32),
                                             cfg.box_prediction)
            centermaps = {f"centermaps_{k}": v for k, v in maps.items()}
        else:
            centermaps = {}
        out.setdefault(cfg.data.train_on_box_source, {}).update({"boxes": boxes, "prediscovered_boxes": pre, **centermaps})
        return out
