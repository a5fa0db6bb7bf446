"""Input builders and host expectations of the pillar-encoder stage tests (tests/test_gpu_pillars_stages.py); nothing here touches a
GPU.  tests/test_pillar_stage_cases.py proves on the CPU that every builder yields what its GPU test relies on.

Geometry is exact in fp32: power-of-two cells on a symmetric range, and every coordinate a builder emits lies on a dyadic lattice
(cell / 64), so the fp32 `floor((p - min) / v)` of the oracle, of the kernel and the same expression in fp64 are one arithmetic.
The only points off that lattice are the hand-placed border probes of `borders()`."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import pillars as OP

PATTERN = 0xA5
MOMENTUM, EPS = float(np.float32(0.01)), float(np.float32(1e-3))  # the ABI takes them as fp32: the references use the values it receives
U32 = 2.0 ** -24  # unit roundoff of fp32


class Geo:
    """a gx x gy grid of square `cell`-metre pillars, centred; z in [-z_cut, z_cut)"""

    def __init__(self, gx, gy, cell, z_cut=4.0):
        self.gx, self.gy, self.cell, self.z_cut = int(gx), int(gy), float(cell), float(z_cut)
        half = np.array([gx * cell / 2, gy * cell / 2, z_cut], np.float64)
        self.pc_range = np.concatenate([-half, half])
        self.voxel_size = np.array([cell, cell, 2 * z_cut], np.float64)
        self.bev_range_m, self.grid = (gx * cell, gy * cell), (self.gx, self.gy)
        assert np.array_equal(OP.pillar_geometry(self.bev_range_m, self.grid, z_cut)[0], self.pc_range)
        for v in list(self.pc_range) + list(self.voxel_size):
            assert float(np.float32(v)) == v  # exact in fp32

    @property
    def cells(self):
        return self.gx * self.gy


def pattern_like(shape, dtype):
    return np.full(int(np.prod(shape)) * np.dtype(dtype).itemsize, PATTERN, np.uint8).view(dtype).reshape(shape)


# ---- points ---------------------------------------------------------------------------------------------------------------------
def lattice_points(rng, geo, cells_xy, C, z_lo=None):
    """one point inside each given (x cell, y cell) -- cells outside the grid give points outside the range -- at a random lattice
    position; channel 3 = an intensity in 0..255, channel 4 = a time in [0, 0.5)"""
    cells_xy = np.asarray(cells_xy, np.int64).reshape(-1, 2)
    n = len(cells_xy)
    p = np.zeros((n, C), np.float64)
    p[:, :2] = geo.pc_range[:2] + (cells_xy + rng.integers(1, 64, (n, 2)) / 64.0) * geo.cell
    if z_lo is None:
        p[:, 2] = -geo.z_cut + rng.integers(1, 64, n) / 64.0 * 2 * geo.z_cut
    else:
        p[:, 2] = z_lo + rng.integers(0, 128, n) / 64.0  # [z_lo, z_lo + 2)
    if C > 3:
        p[:, 3] = rng.integers(0, 256, n)
    if C > 4:
        p[:, 4] = rng.integers(0, 128, n) / 256.0
    q = p.astype(np.float32)
    assert np.array_equal(q.astype(np.float64), p)
    return q


def random_cells(rng, geo, n, margin=1):
    """uniform over the grid and `margin` cells beyond it on every side (those points are dropped)"""
    return np.stack([rng.integers(-margin, geo.gx + margin, n), rng.integers(-margin, geo.gy + margin, n)], 1)


def cell_of(geo, b, x, y):
    return (b * geo.gx + x) * geo.gy + y


# ---- host expectation of liso_pillars_voxelize_f32 -----------------------------------------------------------------------------------
def per_sample(pcls, geo, max_points, max_voxels, dtype=np.float32):
    """oracle voxelisation of every sample on its own -> list of (num_points[P], coors[P, 4] = (b, 0, x, y), point_idx[P, max_points]
    with global point indices, -1 = padding)"""
    out, off = [], 0
    for b, p in enumerate(pcls):
        _, c, n, pi = OP.voxelize_hard(np.asarray(p, dtype), geo.voxel_size, geo.pc_range, max_points, max_voxels)
        c = c[:, [0, 2, 1]]  # (z, y, x) -> (z, x, y), as voxelize_batch
        c = np.concatenate([np.full((len(c), 1), b, np.int32), c.astype(np.int32)], axis=1)
        out.append((n.astype(np.int32), c, np.where(pi >= 0, pi + off, -1)))
        off += len(p)
    return out


def expected_voxelize(pcls, geo, max_points, max_voxels):
    """full output buffers of the entry point over buffers pre-filled with PATTERN: everything the kernels must not write keeps it"""
    B, rows = len(pcls), len(pcls) * max_voxels
    coors, num_points = pattern_like((rows, 4), np.int32), pattern_like((rows,), np.int32)
    slots = pattern_like((rows, max_points), np.int32)
    num_voxels, c2v = np.zeros(B, np.int32), np.zeros(B * geo.cells, np.int32)
    for b, (n, c, pi) in enumerate(per_sample(pcls, geo, max_points, max_voxels)):
        P, r0 = len(n), b * max_voxels
        num_voxels[b] = P
        coors[r0:r0 + P], num_points[r0:r0 + P] = c, n
        blk = slots[r0:r0 + P]
        blk[pi >= 0] = pi[pi >= 0]
        c2v[cell_of(geo, b, c[:, 2], c[:, 3])] = r0 + np.arange(P) + 1
    return dict(coors=coors, num_points=num_points, slots=slots, num_voxels=num_voxels, cell_to_voxel=c2v)


def pillar_sizes(p, geo):
    """{(x, y): number of in-range points} of one sample, by the oracle with room for every point"""
    n, c, _ = per_sample([p], geo, max(len(p), 1), geo.cells)[0]
    return {(int(x), int(y)): int(k) for (x, y), k in zip(c[:, 2:], n)}


def offsets_of(pcls):
    return [0] + [int(v) for v in np.cumsum([len(p) for p in pcls])]


# ---- voxeliser cases: dict(pcls, geo, max_points, max_voxels) -----------------------------------------------------------------------------
def _case(pcls, geo, max_points, max_voxels, **extra):
    return dict(pcls=[np.ascontiguousarray(p, np.float32) for p in pcls], geo=geo, max_points=max_points, max_voxels=max_voxels, **extra)


def _spread_sample(rng, geo, n, C):
    """new cells keep appearing from the first to the last 1024-point tile: point i lies near cell i * cells / n, and the last point
    alone has the last cell"""
    lin = np.minimum((np.arange(n) * geo.cells) // max(n, 1) + rng.integers(0, 3, n), geo.cells - 2)
    lin[-1] = geo.cells - 1
    return lattice_points(rng, geo, np.stack([lin // geo.gy, lin % geo.gy], 1), C)


TILE_EDGE_LENGTHS = {
    "short": [0, 1, 63, 0, 64, 65, 1023, 0, 1024, 1025, 2048, 0],
    "aligned": [0, 1024, 0, 1025],           # offsets [0, 0, 1024, 1024, 2049]
    "long": [0, 66560, 0, 66561, 5],         # 65 tiles; 66 tiles: the last tile's base is summed on a second trip of the strided loop
}


def tile_edges(which):
    rng = np.random.default_rng(len(which))
    geo = Geo(64, 64, 1.0)
    pcls = []
    for n in TILE_EDGE_LENGTHS[which]:
        pcls.append(_spread_sample(rng, geo, n, 4) if n > 4096 else lattice_points(rng, geo, random_cells(rng, geo, n), 4))
    return _case(pcls, geo, 20, 4200)


def runs():
    """consecutive points sharing a cell in runs of 1..200 (they cross the 64-lane waves), out-of-range and NaN points inside runs, the
    sample boundaries inside runs: the last point of a sample and the first of the next have the same (x, y)"""
    rng = np.random.default_rng(11)
    geo = Geo(64, 64, 1.0)
    lengths = list(rng.permutation(np.arange(1, 201))[:60]) + [1, 2, 63, 64, 65, 128, 129, 200]
    chunks, starts, pos = [], [], 0
    for k, n in enumerate(lengths):
        cell = random_cells(rng, geo, 1, margin=0)
        p = lattice_points(rng, geo, np.repeat(cell, n, 0), 4)
        if n >= 5 and k % 3 == 0:
            p[n // 2, 0] = geo.pc_range[3] + 1.0   # out of range, inside the run
        if n >= 5 and k % 3 == 1:
            p[n // 2, 1] = np.nan
        chunks.append(p)
        starts.append(pos)
        pos += n
    pts = np.concatenate(chunks)
    if len(pts) % 64 == 0:
        pts = pts[:-1]
    cuts = []
    for k in (len(lengths) // 3, 2 * len(lengths) // 3):
        while lengths[k] < 8:
            k += 1
        cut = starts[k] + 2       # inside run k, in front of its out-of-range / NaN point
        pts[cut, :2] = pts[cut - 1, :2]
        cuts.append(cut)
    assert len(pts) % 64 and len(pts) % 256
    return _case(np.split(pts, cuts), geo, 20, 4200, cuts=cuts)


def floors_agree(val, mn, v, dtype_val=np.float32):
    """fp32 floor((val - mn) / v) == the same in fp64 (val is an fp32 number)"""
    val = np.float32(val)
    with np.errstate(invalid="ignore", over="ignore"):
        a = np.floor((val - np.float32(mn)) / np.float32(v))
        b = np.floor((np.float64(val) - np.float64(mn)) / np.float64(v))
    return bool(a == b) or (np.isnan(a) and np.isnan(b))


def neighbours(e, mn, v):
    """the fp32 values next to the edge `e` on either side: np.nextafter's, and one step of the coarser of the two fp32 lattices involved
    (the point's own and that of the difference `p - mn` the voxeliser floors).  A raw nextafter neighbour whose fp32 difference
    rounds onto the edge floors differently in fp32 and fp64 (for example just below x_max = 32: 32 - 2^-19 + 32 rounds to 64); those
    are left out, the lattice step takes their place."""
    e32 = np.float32(e)
    s = max(np.spacing(np.float32(abs(e))), np.spacing(np.float32(abs(e - mn))))
    cand = [np.nextafter(e32, np.float32(-np.inf)), np.nextafter(e32, np.float32(np.inf)), np.float32(e - s), np.float32(e + s)]
    return [c for c in cand if floors_agree(c, mn, v)]


def borders():
    rng = np.random.default_rng(21)
    geo = Geo(64, 64, 1.0)
    probes = []
    for axis in range(3):
        mn, mx, v = geo.pc_range[axis], geo.pc_range[axis + 3], geo.voxel_size[axis]
        edges = [mn, mx] + ([-17.0, -16.0, 0.0, 5.0, 31.0] if axis < 2 else [])
        vals = []
        for e in edges:
            vals += [np.float32(e)] + neighbours(e, mn, v)
        vals += [np.float32(-0.0), np.float32(np.inf), np.float32(-np.inf), np.float32(np.nan)]
        for val in vals:
            p = lattice_points(rng, geo, random_cells(rng, geo, 1, margin=0), 4)[0]
            p[axis] = val
            probes.append(p)
    probes = np.stack(probes)
    fill = lattice_points(rng, geo, random_cells(rng, geo, 1500), 4)
    pts = np.concatenate([probes, fill])[rng.permutation(len(probes) + len(fill))]
    return _case([pts[:700], pts[700:]], geo, 20, 4200, probes=probes)


def non_square(gx, gy):
    rng = np.random.default_rng(gx)
    geo = Geo(gx, gy, 0.5)
    return _case([lattice_points(rng, geo, random_cells(rng, geo, n), 4) for n in (2500, 1700)], geo, 20, 4000)


CROWDED_SIZES = (64, 65, 1024, 1025, 2500)
CROWDED_CELLS = ((0, 3), (17, 0), (31, 63), (40, 41), (63, 62))  # in sample 1 of a 64 x 64 grid: scan blocks 4 .. 7


def crowded(max_points):
    rng = np.random.default_rng(31)
    geo = Geo(64, 64, 1.0)

    def background(n):
        c = random_cells(rng, geo, n)
        keep = ~np.isin(c[:, 0] * 64 + c[:, 1], [x * 64 + y for x, y in CROWDED_CELLS])
        return c[keep]

    s0 = lattice_points(rng, geo, background(1500), 4)
    cells = np.concatenate([np.repeat([c], n, 0) for c, n in zip(CROWDED_CELLS, CROWDED_SIZES)] + [background(1500)])
    s1 = lattice_points(rng, geo, cells[rng.permutation(len(cells))], 4)
    return _case([s0, s1], geo, max_points, 4200)


CAP_DISTINCT = (49, 50, 200)


def cap():
    rng = np.random.default_rng(41)
    geo = Geo(64, 64, 1.0)
    pcls = []
    for k in CAP_DISTINCT:
        lin = rng.permutation(geo.cells)[:k]
        lin = np.repeat(lin, rng.integers(1, 7, k))
        lin = lin[rng.permutation(len(lin))]
        pcls.append(lattice_points(rng, geo, np.stack([lin // 64, lin % 64], 1), 4))
    return _case(pcls, geo, 20, 50)


LARGE_BLOCKS = (0, 1, 255, 256, 1023, 1024, 2047, 2048, 4094, 4095)  # global scan-block index = b * 1024 + x on a 1024 x 1024 grid


def large():
    """B = 4 at 1024 x 1024: 4096 scan blocks of 1024 cells.  A pillar in the first and in the last cell of each listed block, ~30 more
    per sample anywhere, 1..30 points each."""
    rng = np.random.default_rng(51)
    geo = Geo(1024, 1024, 0.125)
    pcls = []
    for b in range(4):
        cells = [(blk - b * 1024, y) for blk in LARGE_BLOCKS if blk // 1024 == b for y in (0, 1023)]
        extra = random_cells(rng, geo, 40 - len(cells), margin=0)
        cells = np.concatenate([np.array(cells, np.int64).reshape(-1, 2), extra])
        cells = np.repeat(cells, rng.integers(1, 31, len(cells)), 0)
        pcls.append(lattice_points(rng, geo, cells[rng.permutation(len(cells))], 4))
    return _case(pcls, geo, 20, 64)


def voxeliser_cases():
    """name -> builder of every case of the voxeliser stage test"""
    c = {f"tile_edges-{k}": (lambda k=k: tile_edges(k)) for k in TILE_EDGE_LENGTHS}
    c.update({"runs": runs, "borders": borders, "non_square-96x160": lambda: non_square(96, 160),
              "non_square-160x96": lambda: non_square(160, 96), "cap": cap, "large": large})
    c.update({f"crowded-mp{m}": (lambda m=m: crowded(m)) for m in (1, 20, 32)})
    return c


# ---- clouds for the PFN stages ------------------------------------------------------------------------------------------------------
PFN_RESERVED = {"one": (7, 9), "full": (3, 5), "over": (11, 2)}


def pfn_cloud(seed, geo, C, n, B, max_points=20, z_lo=None, const5=False):
    """B samples of ~n points: uniform background, three blobs of 60 points, in every sample a pillar of exactly one point, one of exactly
    max_points and one of max_points + 7 (their first points come first, so no cap drops them), several points in the four corner
    cells (coordinates next to +-range / 2, where the centre offsets cancel most), an intensity in 0..255"""
    rng = np.random.default_rng(seed)
    res = dict(PFN_RESERVED)
    corners = [(0, 0), (0, geo.gy - 1), (geo.gx - 1, 0), (geo.gx - 1, geo.gy - 1)]
    special = [res["full"]] * (max_points - 1) + [res["over"]] * (max_points + 6) + corners * 3  # (behind the three leading points)
    pcls = []
    for b in range(B):
        bg = random_cells(rng, geo, n)
        bg = bg[~np.isin(bg[:, 0] * geo.gy + bg[:, 1], [x * geo.gy + y for x, y in list(res.values()) + corners])]
        blobs = np.repeat(random_cells(rng, geo, 3, margin=-12), 60, 0)
        rest = np.concatenate([np.array(special), bg, blobs])
        cells = np.concatenate([np.array([res["one"], res["full"], res["over"]]), rest[rng.permutation(len(rest))]])
        p = lattice_points(rng, geo, cells, C, z_lo=z_lo)
        if C > 4 and const5:
            p[:, 4] = 0.375
        pcls.append(p)
    return pcls


def pfn_params(seed, C):
    """weight [64, C + 6], gamma in [0.5, 1.5], beta of both signs, non-trivial running stats (float32 numpy)"""
    r = np.random.default_rng(1000 + seed)
    f32 = np.float32
    return dict(weight=(r.normal(0, 0.3, (64, C + 6))).astype(f32), gamma=r.uniform(0.5, 1.5, 64).astype(f32),
                beta=r.uniform(-0.5, 0.5, 64).astype(f32), running_mean=r.normal(0, 0.5, 64).astype(f32),
                running_var=r.uniform(0.5, 2.0, 64).astype(f32))


# ---- host expectation of liso_pfn_decorate_f32 ---------------------------------------------------------------------------------------
def expected_decorate(pcls, geo, max_points, max_voxels, dtype=torch.float64):
    """-> pt_off int32 [rows + 1], voxel_cell int32 [rows], feature rows [N, C + 6] in `dtype` (pillar order, slot order), point index of
    every row, the oracle's (num, coors) of the kept pillars"""
    B, rows = len(pcls), len(pcls) * max_voxels
    v, n, c, pi = OP.voxelize_batch(pcls, geo.voxel_size, geo.pc_range, max_points, max_voxels)
    feats = OP.pfn_decorate(torch.from_numpy(v).to(dtype), torch.from_numpy(n), torch.from_numpy(c), geo.voxel_size, geo.pc_range)
    valid = np.arange(max_points)[None, :] < n[:, None]
    first = np.concatenate([[0], np.cumsum(np.bincount(c[:, 0], minlength=B))])[:-1]
    row = c[:, 0] * max_voxels + (np.arange(len(n)) - first[c[:, 0]])
    kept = np.zeros(rows, np.int64)
    kept[row] = n
    voxel_cell = np.full(rows, -1, np.int32)
    voxel_cell[row] = cell_of(geo, c[:, 0], c[:, 2], c[:, 3])
    pt_off = np.concatenate([[0], np.cumsum(kept)]).astype(np.int32)
    return dict(pt_off=pt_off, voxel_cell=voxel_cell, rows=feats[torch.from_numpy(valid)].numpy(), point=pi[valid], num=n, coors=c)


# ---- fp64 references of the BN, forward and backward stages from feature rows --------------------------------------------------------------
def pair_index(j, k, D):
    return j * D - j * (j - 1) // 2 + (k - j)


def moments_reference(feat, C):
    """upper triangle of sum [f, 1][f, 1]^T over the rows of `feat` [N, 12] -> (exact-to-fp64 sums [NP], sums of magnitudes [NP]).
    Each product of two fp32 numbers is exact in fp64; the sums are taken in np.longdouble."""
    D = C + 7
    a = np.asarray(feat, np.float64)[:, :D].astype(np.longdouble)
    tot, mag = [], []
    for j in range(D):
        for k in range(j, D):
            pr = a[:, j] * a[:, k]
            tot.append(float(pr.sum()))
            mag.append(float(np.abs(pr).sum()))
    return np.array(tot), np.array(mag)


def bn_reference(feat, C, P, max_points, prm, training):
    """fp64 BatchNorm1d of the Linear output of the rows `feat` [N, 12] of P pillars (torch semantics: the P * max_points - N padded
    rows are zeros and count) -> dict(scale, shift, mean, invstd, running_mean, running_var) in fp64"""
    w, g, bt = (torch.from_numpy(prm[k]).double() for k in ("weight", "gamma", "beta"))
    rm, rv = torch.from_numpy(prm["running_mean"]).double().clone(), torch.from_numpy(prm["running_var"]).double().clone()
    if not training:
        mean, var = rm.clone(), rv.clone()
    else:
        M = P * max_points
        x = torch.from_numpy(np.asarray(feat, np.float64)[:, :C + 6]) @ w.t()
        x = torch.cat([x, torch.zeros((M - x.shape[0], 64), dtype=torch.float64)])
        if M > 1:
            F.batch_norm(x, rm, rv, None, None, True, MOMENTUM, EPS)  # updates rm, rv in place
        mean = x.mean(0) if M else torch.zeros(64, dtype=torch.float64)
        var = x.var(0, unbiased=False) if M else torch.zeros(64, dtype=torch.float64)
    invstd = 1.0 / torch.sqrt(var + EPS)
    out = dict(scale=g * invstd, shift=bt - mean * g * invstd, mean=mean, invstd=invstd, running_mean=rm, running_var=rv,
               shift_term=(mean * g * invstd).abs())
    return {k: v.numpy() for k, v in out.items()}


def forward_reference(feat, pt_off, max_points, C, weight, bn_out):
    """fp64 max over a pillar's rows of relu(scale * (w . f) + shift), the padding candidate relu(shift) included when the pillar holds
    fewer than max_points rows -> (rows that hold points [K], value [K, 64], error bound [K, 64]).
    Bound per row: 16 * 2^-24 * (|scale| * sum_k |w_k f_k| + |shift|); relu and max are 1-Lipschitz, so a pillar's bound is the
    largest bound of its candidates."""
    Fd = C + 6
    f = np.asarray(feat, np.float64)[:, :Fd]
    w = np.asarray(weight, np.float64)
    bn = np.asarray(bn_out, np.float64)
    scale, shift = bn[:64], bn[64:128]
    y = np.maximum(scale * (f @ w.T) + shift, 0.0)
    bound = 16 * U32 * (np.abs(scale) * (np.abs(f) @ np.abs(w).T) + np.abs(shift))
    kept = np.diff(np.asarray(pt_off, np.int64))
    idx = np.flatnonzero(kept > 0)
    if len(idx) == 0:
        return idx, np.zeros((0, 64)), np.zeros((0, 64))
    starts = np.asarray(pt_off, np.int64)[idx]
    val, bnd = np.maximum.reduceat(y, starts, axis=0), np.maximum.reduceat(bound, starts, axis=0)
    pad = (kept[idx] < max_points)[:, None]
    val = np.where(pad, np.maximum(val, np.maximum(shift, 0.0)), val)
    bnd = np.where(pad, np.maximum(bnd, 16 * U32 * np.abs(shift)), bnd)
    return idx, val, bnd


def ulp_of(ref, mant_bits, min_exp):
    """spacing of a binary format with `mant_bits` explicit mantissa bits at |ref| (the subnormal spacing below 2^min_exp)"""
    a = np.maximum(np.abs(np.asarray(ref, np.float64)), 2.0 ** min_exp)
    return np.exp2(np.floor(np.log2(a)) - mant_bits)


# ---- backward -------------------------------------------------------------------------------------------------------------------------
TIE = 1e-4


def _t(prm, dtype, grad):
    out = {k: torch.from_numpy(v).to(dtype).clone() for k, v in prm.items()}
    for k in ("weight", "gamma", "beta"):
        out[k].requires_grad_(grad)
    return out


def near_tie_keep(pcls, geo, max_points, max_voxels, prm, training):
    """-> (keep bool [P, 64], cells [P], stats).  In the fp64 reference, per (pillar, channel): candidates = the pre-activations of the
    pillar's rows and, when it holds fewer than max_points, the padding candidate (pre-activation of a zero row, once).  The upstream
    gradient is dropped where the winner leads the runner-up after the ReLU by less than TIE * max(1, |winner|), or lies within TIE of
    0.  Entries whose winner is below -TIE are kept: every candidate is then switched off by the ReLU, no gradient flows in the
    reference or in the kernel whichever row the max picks, and nothing discontinuous is near."""
    t = _t(prm, torch.float64, False)
    v, n, c, _ = OP.voxelize_batch(pcls, geo.voxel_size, geo.pc_range, max_points, max_voxels)
    P = len(n)
    if P == 0:
        return np.zeros((0, 64), bool), np.zeros(0, np.int64), dict(entries=0, masked=0, full=0, padding_wins=0)
    nt = torch.from_numpy(n)
    feats = OP.pfn_decorate(torch.from_numpy(v).double(), nt, torch.from_numpy(c), geo.voxel_size, geo.pc_range)
    x = F.linear(feats, t["weight"])
    z = F.batch_norm(x.permute(0, 2, 1).contiguous(), t["running_mean"], t["running_var"], t["gamma"], t["beta"], bool(training),
                     MOMENTUM, EPS).permute(0, 2, 1)                      # [P, max_points, 64] pre-activations
    slot = torch.arange(max_points)[None, :]
    z = torch.where((slot > nt[:, None])[..., None], torch.full((), -float("inf"), dtype=torch.float64), z)  # one padding candidate
    if max_points == 1:
        top = torch.cat([z, torch.full_like(z, -float("inf"))], 1)
    else:
        top = torch.topk(z, 2, dim=1).values
    win, second = top[:, 0], top[:, 1]
    lead = torch.relu(win) - torch.relu(second)
    drop = (win > -TIE) & ((lead < TIE * torch.clamp(win.abs(), min=1.0)) | (win.abs() < TIE))
    pad_wins = (nt[:, None] < max_points) & (torch.argmax(z, 1) == nt[:, None].clamp(max=max_points - 1)) & (win > TIE)
    stats = dict(entries=P * 64, masked=int(drop.sum()), full=int((nt == max_points).sum()), padding_wins=int(pad_wins.sum()))
    return (~drop).numpy(), cell_of(geo, c[:, 0], c[:, 2], c[:, 3]).astype(np.int64), stats


def upstream_gradient(seed, B, geo, keep, cells, round_to=None):
    """randn [B, gx, gy, 64] (the kernel's canvas layout), rounded to `round_to` when given, zero at every dropped (pillar, channel)"""
    g = torch.randn((B * geo.cells, 64), generator=torch.Generator().manual_seed(seed), dtype=torch.float32)
    if round_to is not None:
        g = g.to(round_to).float()
    g = g.numpy()
    sub = g[cells]
    sub[~keep] = 0.0
    g[cells] = sub
    return g.reshape(B, geo.gx, geo.gy, 64)


def oracle_gradients(pcls, geo, max_points, max_voxels, prm, training, grad_canvas, dtype):
    """autograd through oracle.pillars.pillar_forward in `dtype` -> dict(weight, gamma, beta) float64 numpy"""
    t = _t(prm, dtype, True)
    bev, _, _ = OP.pillar_forward(pcls, t["weight"], t["gamma"], t["beta"], t["running_mean"], t["running_var"], bool(training),
                                  geo.bev_range_m, geo.grid, geo.z_cut, max_points, max_voxels, dtype=dtype)
    g = torch.from_numpy(grad_canvas).to(dtype).permute(0, 3, 1, 2)
    (bev * g).sum().backward()
    return {k: t[k].grad.double().numpy() for k in ("weight", "gamma", "beta")}


BACKWARD_CASES = [(B, C, tr, "fp32") for B in (1, 3) for C in (3, 4, 5) for tr in (1, 0)] + \
                 [(3, 4, tr, d) for tr in (1, 0) for d in ("bf16", "fp16")] + [(1, 5, 1, "bf16"), (1, 3, 0, "fp16")]
TORCH_DTYPE = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


def backward_case(B, C, training, gdtype):
    """-> dict(pcls, geo, prm, grad canvas fp32 numpy (already rounded to the 16-bit type and masked), stats of the mask)"""
    geo = Geo(64, 64, 1.0)
    seed = 100 * B + C
    pcls = pfn_cloud(seed, geo, C, 4200 // B, B)  # 3000 .. 6000 points in all
    prm = pfn_params(seed, C)
    keep, cells, stats = near_tie_keep(pcls, geo, 20, 40000, prm, training)
    rt = None if gdtype == "fp32" else TORCH_DTYPE[gdtype]
    g = upstream_gradient(seed + 7 * training, B, geo, keep, cells, rt)
    return dict(pcls=pcls, geo=geo, prm=prm, grad=g, stats=stats, max_points=20, max_voxels=40000)
