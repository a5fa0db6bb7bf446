"""The compact pillar canvas (mfma_conv.PillarCanvas: pillar rows + cell -> row map + occupancy; liso_pfn_forward_rows,
liso_sparse_conv_forward_rows) against the dense canvas it replaces on the SLIM inference path: bit for bit, no tolerance.
`mfma_conv.set_compact_canvas(False)` is the oracle."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
MAX_POINTS = 20
VOXEL = 0.5
# (gx, gy, samples, max_voxels): 128 x 64 is not square (an x / y swap shows); max_voxels = 256 drops voxels of the 3000-point sample
CASES = [(64, 64, 2, 40000), (128, 64, 3, 40000), (64, 64, 3, 256)]
COUNTS = (3000, 700, 0)  # points per sample: one sample is empty


def _pcfg(gx, gy, max_voxels):
    from liso_amd import _lib as L

    c = L.PillarCfg()
    c.x_min, c.y_min, c.z_min = -gx * VOXEL / 2, -gy * VOXEL / 2, -5.0
    c.vx, c.vy, c.vz = VOXEL, VOXEL, 10.0
    c.gx, c.gy = gx, gy
    c.max_points, c.max_voxels, c.n_channels = MAX_POINTS, max_voxels, 4
    return c


def _clouds(gx, gy, B, seed):
    """B clouds [n, 4] (numpy) with COUNTS points; sample 0 also holds a pillar in each of the four corner cells and one pillar with
    more than max_points points"""
    rng = np.random.default_rng(seed)
    ext = np.array([gx * VOXEL, gy * VOXEL, 4.0, 1.0], np.float32)
    lo = np.array([-gx * VOXEL / 2, -gy * VOXEL / 2, -2.0, 0.0], np.float32)
    out = []
    for b in range(B):
        p = (rng.random((COUNTS[b % 3], 4), dtype=np.float32) * ext + lo).astype(np.float32)
        if b == 0:
            cx, cy = gx * VOXEL / 2 - VOXEL / 2, gy * VOXEL / 2 - VOXEL / 2
            corners = np.array([[sx * cx, sy * cy, 0.3, 0.5] for sx in (-1, 1) for sy in (-1, 1)], np.float32)
            crowd = np.tile(np.array([[0.25, 0.25, 0.0, 0.1]], np.float32), (MAX_POINTS + 11, 1))
            crowd[:, :3] += (rng.random((MAX_POINTS + 11, 3), dtype=np.float32) - 0.5) * 0.2
            p = np.concatenate([corners, p, crowd], axis=0)
        out.append(p)
    return out


def _cells(p, gx, gy):
    """flattened cell x_idx * gy + y_idx of every point of one cloud (host restatement of the voxeliser's binning; all points in range)"""
    ix = np.floor((p[:, 0] + gx * VOXEL / 2) / VOXEL).astype(np.int64)
    iy = np.floor((p[:, 1] + gy * VOXEL / 2) / VOXEL).astype(np.int64)
    assert ix.min(initial=0) >= 0 and ix.max(initial=0) < gx and iy.min(initial=0) >= 0 and iy.max(initial=0) < gy
    return ix * gy + iy


def _params(seed):
    g = torch.Generator().manual_seed(seed)
    weight = (torch.randn(64, 10, generator=g) * 0.3).to(DEV)
    gamma = (torch.rand(64, generator=g) + 0.5).to(DEV)
    beta = (torch.randn(64, generator=g) * 0.2).to(DEV)
    return weight, gamma, beta


_ENCODED = {}


def _encoded(case, dtype):
    """one sweep of `case` through the pillar encoder, dense and compact from the same voxelisation (computed once per case and dtype,
    read-only for the tests) -> dict"""
    key = (case, dtype)
    if key in _ENCODED:
        return _ENCODED[key]
    from liso_amd.networks.pcl_to_feature_grid import pcl_to_feature_grid as PF
    from liso_amd.utils import mfma_conv as MC

    gx, gy, B, max_voxels = case
    clouds = _clouds(gx, gy, B, seed=gx + B)
    distinct = [len(np.unique(_cells(p, gx, gy))) for p in clouds]
    if max_voxels < 1000:  # proved on the host: this case drops voxels (and only of the samples that have that many)
        assert distinct[0] > max_voxels and distinct[1] > max_voxels, distinct
    else:
        assert max(distinct) <= max_voxels
    corner_cells = {0, gy - 1, (gx - 1) * gy, gx * gy - 1}
    assert corner_cells <= set(_cells(clouds[0], gx, gy).tolist())
    assert np.bincount(_cells(clouds[0], gx, gy)).max() > MAX_POINTS
    pcfg = _pcfg(gx, gy, max_voxels)
    offsets = [0]
    for p in clouds:
        offsets.append(offsets[-1] + len(p))
    cat = torch.from_numpy(np.concatenate(clouds, axis=0)).to(DEV)
    weight, gamma, beta = _params(5)
    with torch.no_grad():
        prep = PF.pillar_prep(cat, offsets, pcfg)
        stats = [(torch.zeros(64, device=DEV), torch.ones(64, device=DEV)) for _ in range(2)]
        dense, occ_d = PF._PillarFeatureScatter.apply(weight, gamma, beta, *stats[0], cat, offsets, pcfg, True, 0.01, 1e-3, dtype, None, prep)
        # the compact canvas as the second sweep of a stacked pair (row_base = B * max_voxels), rows pre-filled with NaNs: rows that are
        # never written must never be read
        both = MC.PillarCanvas.empty(2 * B, (gx, gy), max_voxels, dtype, DEV)
        both.rows.view(torch.uint8).fill_(0xFF)
        both.cell_map.fill_(-7)
        both.occupancy.fill_(-7.0)
        compact = PF.pillar_rows(weight, gamma, beta, *stats[1], cat, offsets, pcfg, True, 0.01, 1e-3, dtype, both[B:], prep)
    torch.cuda.synchronize()
    res = dict(dense=dense, occ=occ_d, compact=compact, both=both, stats=stats, cell_to_voxel=prep[4], clouds=clouds, distinct=distinct)
    _ENCODED[key] = res
    return res


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_compact_rows_scattered_through_the_map_equal_the_dense_canvas(case, dtype):
    """case 1: rows[map - 1] at the cells the map names and zeros elsewhere == the dense canvas; occupancy, BatchNorm running statistics
    equal; the map is the voxeliser's plus the slice's row base; nothing outside the slice was written"""
    gx, gy, B, max_voxels = case
    e = _encoded(case, dtype)
    c = e["compact"]
    assert tuple(c.shape) == (B, 64, gx, gy) and c.row_base == B * max_voxels and c.dtype == dtype
    assert torch.equal(c.occupancy, e["occ"])
    assert torch.equal(c.dense().contiguous(), e["dense"].contiguous())
    v = e["cell_to_voxel"].view(B, gx, gy)
    assert torch.equal(c.cell_map, torch.where(v > 0, v + B * max_voxels, torch.zeros_like(v)))
    assert torch.equal((c.cell_map > 0).float().view(B, 1, gx, gy), c.occupancy)
    for a, b in zip(e["stats"][0], e["stats"][1]):
        assert torch.equal(a, b)
    # the pillars each sample keeps: min(distinct cells, max_voxels); the empty sample none
    kept = [min(d, max_voxels) for d in e["distinct"]]
    assert [int(o.sum()) for o in c.occupancy] == kept
    assert B < 3 or kept[2] == 0
    # the first sweep's half of the stacked canvas is untouched, and so are the rows of unused pillars
    both = e["both"]
    assert bool((both.cell_map[:B] == -7).all()) and bool((both.occupancy[:B] == -7.0).all())
    used = torch.zeros(both.rows.shape[0], dtype=torch.bool, device=DEV)
    used[(c.cell_map[c.cell_map > 0] - 1).long()] = True
    assert bool((both.rows[~used].contiguous().view(torch.uint8) == 0xFF).all())
    assert not bool(torch.isnan(both.rows[used].float()).any())


def _stem_pair(case, dtype, k, co, kind, extra_occupancy):
    from liso_amd.utils import mfma_conv as MC

    gx, gy, B, _ = case
    e = _encoded(case, dtype)
    occ = e["occ"]
    if extra_occupancy:  # every cell that holds a point, dropped voxels included: listed cells without a row must read zeros
        occ = torch.zeros(B, gx * gy, device=DEV)
        for b, p in enumerate(e["clouds"]):
            occ[b, torch.from_numpy(np.unique(_cells(p, gx, gy))).to(DEV)] = 1.0
        occ = occ.view(B, 1, gx, gy)
        assert int(occ.sum()) > int(e["occ"].sum())
    g = torch.Generator().manual_seed(11)
    conv = torch.nn.Conv2d(64, co, k, stride=2, padding=k // 2).to(DEV)
    with torch.no_grad():
        conv.weight.copy_((torch.randn(conv.weight.shape, generator=g) * 0.05).to(DEV))
        conv.bias.copy_((torch.randn(co, generator=g) * 0.1).to(DEV))
    spec = MC.ConvSpec.of(conv)
    shift = (torch.randn(co, generator=g) * 0.1).to(DEV) if kind == "batch" else None
    with torch.no_grad():
        # the compact canvas stands in its stacked pair: the sweep's slice reads the pair's row array through its own map
        res_c = MC._sparse_stem(e["compact"], occ, conv.weight, conv.bias, spec, kind, True, stats_shift=shift)
        res_d = MC._sparse_stem(e["dense"], occ, conv.weight, conv.bias, spec, kind, True, stats_shift=shift)
    torch.cuda.synchronize()
    assert res_c is not None and res_d is not None
    assert not MC.sparse_stem_overflowed(DEV)
    return res_c, res_d


STEMS = [(torch.float32, 7, 32, "instance"), (torch.float32, 7, 32, "none"), (torch.bfloat16, 3, 64, "batch"),
         (torch.float16, 3, 64, "batch"), (torch.float32, 3, 64, "batch")]


@pytest.mark.parametrize("dtype,k,co,kind", STEMS, ids=["7x7-fp32-in", "7x7-fp32-relu", "3x3-bf16", "3x3-fp16", "3x3-fp32"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_stem_forward_from_compact_equals_stem_forward_from_dense(case, dtype, k, co, kind):
    """case 2: output and statistics partial sums of the sparse stem, rows read through the map == dense canvas read at the cells"""
    (yc, pc, _), (yd, pd, _) = _stem_pair(case, dtype, k, co, kind, extra_occupancy=False)
    assert yc.dtype == dtype and torch.equal(yc, yd) and bool(torch.isfinite(yc.float()).all())
    assert float(yc.float().abs().sum()) > 0
    if kind == "none":
        assert pc is None and pd is None
    else:
        assert torch.equal(pc, pd)


@pytest.mark.parametrize("dtype,k,co,kind", STEMS[:1] + STEMS[2:3], ids=["7x7-fp32-in", "3x3-bf16"])
def test_listed_cells_without_a_row_read_zeros(dtype, k, co, kind):
    """the occupancy map names the cells of voxels that were dropped at max_voxels: the dense canvas is zero there, the compact form
    has no row (map 0) and must multiply zeros, not row -1"""
    (yc, pc, _), (yd, pd, _) = _stem_pair(CASES[2], dtype, k, co, kind, extra_occupancy=True)
    assert torch.equal(yc, yd) and torch.equal(pc, pd) and bool(torch.isfinite(yc.float()).all())


def test_rows_entry_points_refuse_bad_arguments():
    """liso_sparse_conv_forward_rows without a map or with a row count outside [1, 2^31); liso_pfn_forward_rows without a map, with a
    negative row base or with row_base + rows beyond int32: LISO_EINVAL before any launch, nothing written"""
    import ctypes

    from liso_amd import _lib as L
    from liso_amd.networks.pcl_to_feature_grid import pcl_to_feature_grid as PF

    lib = L.lib()
    B, H, W, k, co, cap = 1, 64, 64, 3, 64, 256
    rows = torch.zeros(16, 64, dtype=torch.bfloat16, device=DEV)
    cmap = torch.zeros(B, H, W, dtype=torch.int32, device=DEV)
    occ = torch.zeros(B, H, W, dtype=torch.float32, device=DEV)
    packed = torch.zeros(lib.liso_conv_packed_bytes(64, co, 9, L.CONV_BF16), dtype=torch.uint8, device=DEV)
    y = torch.zeros(B, H // 2, W // 2, co, dtype=torch.bfloat16, device=DEV)
    nbytes = lib.liso_sparse_conv_workspace_bytes(B, H, W, k, co, cap, 0)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    st = L.stream_ptr()
    tail = (L.ptr(occ), L.ptr(packed), None, B, H, W, k, co, cap, 0, L.ptr(y), None, None, None, L.ptr(ws), nbytes, st)
    assert lib.liso_sparse_conv_forward_rows(L.ptr(rows), 64, L.ELEM_BF16, None, 16, *tail) == -1
    assert lib.liso_sparse_conv_forward_rows(L.ptr(rows), 64, L.ELEM_BF16, L.ptr(cmap), 0, *tail) == -1
    assert lib.liso_sparse_conv_forward_rows(L.ptr(rows), 64, L.ELEM_BF16, L.ptr(cmap), 1 << 31, *tail) == -1
    torch.cuda.synchronize()
    assert float(y.float().abs().sum()) == 0.0
    # the encoder's side, with the real products of a small cloud
    pcfg = _pcfg(H, W, cap)
    cloud = torch.from_numpy(_clouds(H, W, 2, seed=3)[1]).to(DEV)
    pt_off, feat, voxel_cell, _, cell_to_voxel = PF.pillar_prep(cloud, [0, cloud.shape[0]], pcfg)
    weight, _, _ = _params(5)
    bn = torch.ones(4 * 64, device=DEV)
    out_rows = torch.zeros(cap, 64, device=DEV)
    out_map = torch.zeros(H * W, dtype=torch.int32, device=DEV)
    out_occ = torch.zeros(H * W, device=DEV)

    def call(row_base, map_ptr):
        return lib.liso_pfn_forward_rows(L.ptr(feat), L.ptr(pt_off), L.ptr(voxel_cell), ctypes.byref(pcfg), 1, L.ptr(cell_to_voxel),
                                         L.ptr(weight), L.ptr(bn), L.ptr(out_rows), L.ELEM_F32, row_base, map_ptr, L.ptr(out_occ), st)

    assert call(0, None) == -1
    assert call(-1, L.ptr(out_map)) == -1
    assert call((1 << 31) - cap, L.ptr(out_map)) == -1  # row_base + rows = 2^31: the map's row + 1 would not fit
    torch.cuda.synchronize()
    assert float(out_rows.abs().sum()) == 0.0 and int(out_map.abs().sum()) == 0 and float(out_occ.abs().sum()) == 0.0
    assert call((1 << 31) - cap - 1, L.ptr(out_map)) == 0  # the largest base that fits
    torch.cuda.synchronize()
    assert int(out_map.max()) == (1 << 31) - 1 and float(out_occ.sum()) == cap


def _bits(t):
    t = t.detach().contiguous().reshape(-1)
    return t.view(torch.uint8).clone() if t.is_floating_point() else t.clone()


def test_liso_loop_steps_are_bit_identical_with_the_compact_canvas_on_and_off(monkeypatch):
    """case 5: LisoLoopTrainer at 128 x 128 with ~5k points, three steps with the switch on and off, launched eagerly on one stream
    and as the benchmark launches them (hipGraphs + pipeline: from the second inference on the encoder writes into the graph's static
    PillarCanvas and the graph is replayed): losses, mined boxes and the detector's state are equal in all four runs' pairs, and the
    first graph step equals the first eager one.  The SLIM inference really takes the compact form when the switch is on (both
    encoders' stems), and never when it is off."""
    from liso_amd.datasets.synthetic import slim_pair
    from liso_amd.kabsch.shape_utils import Shape
    from liso_amd.trainer import LisoLoopTrainer
    from liso_amd.utils import mfma_conv as MC
    from liso_amd.utils.config import apply_slim_simple_knn_training, default_cfg

    dev = torch.device(DEV)
    pairs = [slim_pair(70 + i, dev, n_points=5000, grid=128, bev_range_m=50.0) for i in range(3)]
    seen = []
    real = MC._sparse_stem

    def spy(x_raw, *a, **kw):
        res = real(x_raw, *a, **kw)
        seen.append((isinstance(x_raw, MC.PillarCanvas), res is not None))
        return res

    monkeypatch.setattr(MC, "_sparse_stem", spy)

    def run(on, fast, steps=3):
        prev = MC.set_compact_canvas(on)
        try:
            torch.manual_seed(0)
            tr = LisoLoopTrainer(apply_slim_simple_knn_training(default_cfg(grid=128, bev_range_m=50.0)), dev, compute_dtype=torch.bfloat16,
                                 total_steps=10, use_graph=fast, overlap=fast)
            del seen[:]
            losses = [_bits(tr.step(*pairs[i % 3], upcoming=(pairs[(i + 1) % 3], pairs[(i + 2) % 3]))) for i in range(steps)]
            torch.cuda.synchronize()
            b = tr.last_boxes
            valid = b.valid.clone()
            boxes = {k: _bits(getattr(b, k)[valid]) for k in Shape._keys if k != "valid" and getattr(b, k) is not None}  # (the slots beyond the mined boxes are padding)
            boxes["valid"] = valid
            return (losses, boxes, {k: _bits(v) for k, v in tr.detector.net.state_dict().items()}, list(seen))
        finally:
            MC.set_compact_canvas(prev)

    def same(a, b):
        assert all(torch.equal(x, y) for x, y in zip(a[0], b[0]))
        for part in (1, 2):
            assert a[part].keys() == b[part].keys()
            for k in a[part]:
                assert torch.equal(a[part][k], b[part][k]), k

    off, on = run(False, False), run(True, False)
    assert not any(c for c, _ in off[3])
    compact_calls = [ok for c, ok in on[3] if c]
    assert len(compact_calls) >= 2 and all(compact_calls)  # the stems of fnet and cnet
    same(off, on)
    g_off, g_on = run(False, True), run(True, True)
    assert not any(c for c, _ in g_off[3]) and any(c for c, _ in g_on[3])
    same(g_off, g_on)
    assert torch.equal(g_on[0][0], on[0][0])
    assert not MC.sparse_stem_overflowed(dev)
