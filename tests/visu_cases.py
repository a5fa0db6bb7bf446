"""Inputs of the summary-picture tests (tests/test_visu_host.py, tests/test_gpu_visu.py) and of scripts/make_visu_golden.py: small,
seeded, and each built around the edges its kernel can go wrong at."""
import numpy as np

H, W = 24, 40  # not square, so that a row / column swap shows
REACH = 4 * max(H, W)


def cfg(max_batches=4):
    """the three settings the pictures read"""
    from liso_amd.utils.config import to_attr

    return to_attr({"logging": {"max_log_img_batches": max_batches}, "data": {"bev_range_m": RANGE2}, "nms_iou_threshold": 0.1})


# ---- lines --------------------------------------------------------------------------------------------------------------------------
def special_lines():
    """[(name, (r0, c0, r1, c1))] on an H x W canvas with the default reach"""
    return [
        ("zero length", (5, 7, 5, 7)),
        ("cross a", (2, 3, 20, 30)),
        ("cross b", (20, 3, 2, 30)),
        ("twice 1", (4, 10, 15, 33)),
        ("twice 2", (4, 10, 15, 33)),
        ("leaves top", (6, 12, -9, 20)),
        ("leaves bottom", (18, 5, 40, 11)),
        ("leaves left", (10, 6, 14, -25)),
        ("leaves right", (3, 30, 9, 70)),
        ("outside within reach", (-10, -5, -3, 50)),
        ("outside, clipped onto one corner", (-20, -30, -4, -2)),
        ("beyond reach", (5, 5, 8, W - 1 + REACH + 1)),
        ("beyond reach, negative", (-REACH - 1, 2, 3, 3)),
        ("steep", (1, 20, 22, 22)),
        ("shallow", (12, 1, 13, 38)),
    ]


def line_scene(n_lines, channels, seed=0):
    """canvas fp32 [3, H, W, C], endpoints int32 [3, L, 2, 2], valid bool [3, L], colors fp64 [3, L, C].  Image 0 starts with the
    special lines (as many as fit) with one of them switched off; image 1 is random lines, some off; image 2 has no valid line."""
    rng = np.random.default_rng(100 + seed + 7 * n_lines + channels)
    canvas = rng.random((3, H, W, channels)).astype(np.float32)
    ends = np.stack([rng.integers(-12, H + 12, (3, n_lines, 2)), rng.integers(-12, W + 12, (3, n_lines, 2))], axis=-1).astype(np.int32)
    spec = np.array([s[1] for s in special_lines()], np.int32).reshape(-1, 2, 2)[:n_lines]
    ends[0, :len(spec)] = spec
    valid = rng.random((3, n_lines)) < 0.85
    valid[0, :len(spec)] = True
    if n_lines > len(spec):
        ends[0, len(spec)] = ((0, 0), (H - 1, W - 1))  # a line with its validity off
        valid[0, len(spec)] = False
    valid[2] = False
    colors = rng.random((3, n_lines, channels))
    return canvas, ends, valid, colors


# ---- boxes --------------------------------------------------------------------------------------------------------------------------
RANGE2 = (12.0, 20.0)  # 0.5 m pixels on H x W
RANGE4 = (-5.0, -11.0, 7.0, 9.0)  # min_x, min_y, max_x, max_y: factors 2 and 2, pixels of 0.5 m
MARGIN = 1e-3


def corner_values_fp64(pos, dims, rot, form, dims_clamp=None):
    """the pre-rounding (row, col) values [.., 5, 2] of the corners, recomputed in fp64"""
    pos, dims, th = np.asarray(pos, np.float64), np.asarray(dims, np.float64), np.asarray(rot, np.float64)[..., 0]
    if dims_clamp is not None:
        dims = np.clip(dims, *dims_clamp)
    hx, hy = 0.5 * dims[..., 0], 0.5 * dims[..., 1]
    lx = np.stack([hx, -hx, -hx, hx, hx + hy], -1)
    ly = np.stack([hy, hy, -hy, -hy, 0 * hy], -1)
    c, s = np.cos(th)[..., None], np.sin(th)[..., None]
    x, y = c * lx - s * ly + pos[..., 0:1], s * lx + c * ly + pos[..., 1:2]
    if form == 2:
        return np.stack([(x + 0.5 * RANGE2[0]) * H / RANGE2[0], (y + 0.5 * RANGE2[1]) * W / RANGE2[1]], -1)
    f = min(H / (RANGE4[2] - RANGE4[0]), W / (RANGE4[3] - RANGE4[1]))
    return np.stack([(x - RANGE4[0]) * f, (y - RANGE4[1]) * f], -1)


def edge_margin(values, form):
    """distance of every value to the nearest rounding edge: k + 0.5 for the rounded form, an integer for the truncated one"""
    v = values + 0.5 if form == 2 else values
    return np.abs(v - np.rint(v))


def box_set(dtype=np.float32, seed=3):
    """numpy dict of a [2, 9] padded box set: pos, dims, rot, probs, valid.  Slot 8 of sample 0 is an invalid slot of NaN, slot 0 of
    either sample has dims below 0.3 m, slot 1 dims above 15 m; yaws are 0, 90, 30 and 45 degrees and a few arbitrary ones.  Every
    box is drawn from a seeded generator until all its corner values, in `dtype`, for both range forms, clamped and not, keep MARGIN
    from their rounding edges (the tests assert that margin on every corner again)."""
    rng = np.random.default_rng(seed)
    yaws = [0.0, np.pi / 2, np.pi / 6, np.pi / 4, -np.pi / 6, 2.0, -1.1, 3.0, 0.3]
    pos, dims, rot = np.zeros((2, 9, 3)), np.zeros((2, 9, 3)), np.zeros((2, 9, 1))
    for b in range(2):
        for s in range(9):
            while True:
                p = np.array([rng.uniform(-5.0, 5.0), rng.uniform(-8.0, 8.0), rng.uniform(-1.5, 0.0)])
                d = np.array([rng.uniform(1.0, 5.0), rng.uniform(0.6, 2.5), rng.uniform(1.0, 2.0)])
                if s == 0:
                    d[:2] = rng.uniform(0.05, 0.28, 2)
                if s == 1:
                    d[0] = rng.uniform(15.5, 19.0)
                r = np.array([yaws[(s + 4 * b) % 9]])
                p, d, r = (v.astype(dtype).astype(np.float64) for v in (p, d, r))
                if all(edge_margin(corner_values_fp64(p, d, r, form, clamp), form).min() >= 20 * MARGIN
                       for form in (2, 4) for clamp in (None, (0.3, 15.0))):
                    break
            pos[b, s], dims[b, s], rot[b, s] = p, d, r
    valid = np.ones((2, 9), bool)
    valid[0, 8] = False
    valid[1, 5] = False
    pos[0, 8], dims[0, 8], rot[0, 8] = np.nan, np.nan, np.nan
    probs = rng.uniform(0.05, 0.95, (2, 9, 1))
    probs[0, 8] = np.nan
    return {"pos": pos.astype(dtype), "dims": dims.astype(dtype), "rot": rot.astype(dtype), "probs": probs.astype(dtype), "valid": valid}


def shifted(boxes, seed):
    """another layer: the same kind of boxes elsewhere (no margin promise: use where host and device share the corner table)"""
    rng = np.random.default_rng(seed)
    out = {k: v.copy() for k, v in boxes.items()}
    out["pos"][..., :2] += rng.uniform(-2.0, 2.0, out["pos"][..., :2].shape).astype(out["pos"].dtype)
    out["rot"] += rng.uniform(-1.0, 1.0, out["rot"].shape).astype(out["rot"].dtype)
    return out


# ---- flow wheel ---------------------------------------------------------------------------------------------------------------------
def flow_cases():
    """fp32 [3, 2, 8, 12]: an all-zero image, an image with one non-zero cell, and one with flows at the six sector angles k * 60
    degrees, at -1e-7 rad and at random directions and lengths"""
    rng = np.random.default_rng(5)
    flow = np.zeros((3, 2, 8, 12), np.float32)
    flow[1, :, 3, 7] = (0.3, -0.4)
    ang = rng.uniform(-np.pi, np.pi, (8, 12))
    mag = rng.uniform(0.0, 3.0, (8, 12))
    ang[0, :7] = [k * np.pi / 3 for k in range(6)] + [-1e-7]
    ang[1, :6] = [k * np.pi / 3 - np.pi for k in range(6)]
    flow[2, 0], flow[2, 1] = mag * np.cos(ang), mag * np.sin(ang)
    flow[2, :, 0, 6] = (2.0, np.float32(2.0) * np.float32(-1e-7))  # atan2 = -1e-7 in fp32 too
    return flow


def flow_wheel_fp64(flow):
    """the flow wheel's formula in fp64 on the fp32 inputs -> [B, 3, H, W]"""
    f = flow.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        mag = np.sqrt(f[:, 0] ** 2 + f[:, 1] ** 2)
        ang = np.arctan2(f[:, 1], f[:, 0])
        hue = np.where(ang >= 0, ang, ang + 2 * np.pi) / (2 * np.pi)
        q = mag / mag.max(axis=(1, 2), keepdims=True)
        val = np.where(q < 1.0, q, 1.0)
    k = hue * 6.0
    x = val * (1.0 - np.abs(np.fmod(k, 2.0) - 1.0))
    sector = np.floor(k).astype(np.int64) % 6
    zero = np.zeros_like(val)
    r = np.choose(sector, [val, x, zero, zero, x, val])
    g = np.choose(sector, [x, val, val, x, zero, zero])
    b = np.choose(sector, [zero, zero, x, val, val, x])
    return np.stack([r, g, b], axis=1)


# ---- top-down and occupancy ---------------------------------------------------------------------------------------------------------
TD_GRID = (16, 24)
TD_MIN, TD_MAX = np.array([-4.0, -5.0], np.float32), np.array([4.0, 9.0], np.float32)  # factors 2 and 24 / 14: the smaller one rules


def topdown_clouds():
    """fp32 clouds [2, 300, 4] (NaN-padded) and intensities [2, 300]: cloud 0 has intensities in [0, 1] (no rescale), cloud 1 in
    [-2, 5] (rescale) and 40 padding rows.  Either holds four points in one pixel and, at each of the four extent edges, one point
    0.5 cm inside (out by the 1 cm margin) and one 1.5 cm inside (in)."""
    rng = np.random.default_rng(11)
    N = 300
    pcl = np.stack([rng.uniform(-5.0, 5.0, (2, N)), rng.uniform(-6.5, 10.5, (2, N)), rng.uniform(-2, 1, (2, N)), rng.random((2, N))], -1)
    pcl = pcl.astype(np.float32)
    inten = np.stack([rng.random(N), rng.uniform(-2.0, 5.0, N)]).astype(np.float32)
    inten[1, 5], inten[1, 6] = -2.0, 5.0
    for b in range(2):
        pcl[b, 10:14, :2] = [(1.3, 2.1), (1.4, 2.3), (1.5, 2.2), (1.35, 2.25)]  # pixel (9, 12) of 14 / 24 m
        k = 20
        for axis in range(2):
            for edge, sign in ((TD_MIN[axis], 1.0), (TD_MAX[axis], -1.0)):
                for inset in (0.005, 0.015):
                    pcl[b, k, :2] = (0.5, 0.7)
                    pcl[b, k, axis] = edge + sign * inset
                    k += 1
    pcl[1, 260:] = np.nan
    inten[1, 260:] = np.nan
    return pcl, inten


def occupancy_points():
    """fp32 points [2, 50, 3] with NaN rows and rows outside the range, and a validity mask"""
    rng = np.random.default_rng(13)
    pts = np.stack([rng.uniform(-7.0, 7.0, (2, 50)), rng.uniform(-11.0, 11.0, (2, 50)), rng.uniform(-1, 1, (2, 50))], -1).astype(np.float32)
    pts[0, 3] = np.nan
    pts[1, 4, 0] = np.nan
    pts[0, 5, :2] = (-6.0, -10.0)  # the range's corner: pixel (0, 0)
    pts[0, 6, :2] = (6.0, 10.0)  # the far corner: clamped to the last pixel
    valid = rng.random((2, 50)) < 0.8
    valid[0, 3:7] = True
    return pts, valid
