"""The sub-range entry points of the pillar path (include/liso_pillars.h: liso_pfn_*_sub): a consumer that runs on samples
[sample0, sample0 + batch) of a voxelisation made for a LARGER batch must get, bit for bit, what a stand-alone voxelisation of those
clouds followed by the plain entry point gives -- statistics, dense and compact forward, backward.  No tolerance anywhere."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

GRID, MAX_POINTS, MAX_VOXELS = 32, 20, 256  # 1024 cells of 1 m, at most 256 pillars per sample
SUB_RANGES = [(0, 2), (2, 4), (1, 3), (4, 5), (0, 5)]
_CACHE = {}


def _pcfg(C):
    from liso_amd import _lib as L

    c = L.PillarCfg()
    c.x_min, c.y_min, c.z_min = -16.0, -16.0, -5.0
    c.vx, c.vy, c.vz = 1.0, 1.0, 10.0
    c.gx, c.gy = GRID, GRID
    c.max_points, c.max_voxels, c.n_channels = MAX_POINTS, MAX_VOXELS, C
    return c


def _clouds(C):
    """five clouds of very different sizes: 0: 4000 points over the whole grid (more than MAX_VOXELS pillars: the cap drops some) with
    every 7th point outside the range; 1: one point; 2: empty; 3: 3000 points on 144 cells (about 21 per pillar: many hold
    MAX_POINTS or more); 4: 300 points of which 60 sit in one pillar (more than MAX_POINTS)"""
    g = torch.Generator().manual_seed(100 + C)

    def cloud(n, lo, hi):
        p = torch.randn((n, C), generator=g)
        p[:, :2] = torch.rand((n, 2), generator=g) * (hi - lo) + lo
        p[:, 2] = torch.rand(n, generator=g) * 4.0 - 2.0
        return p

    a = cloud(4000, -16.0, 16.0)
    a[::7, 0] += 40.0
    a[3::50, 2] = 9.0  # (above the z range)
    b = cloud(1, 3.0, 4.0)
    e = torch.zeros((0, C))
    c = cloud(3000, 0.0, 11.9)
    d = cloud(300, -10.0, 10.0)
    d[100:160, :2] = torch.rand((60, 2), generator=g) * 0.9 + 5.05
    return [t.cuda() for t in (a, b, e, c, d)]


def _params(C):
    g = torch.Generator().manual_seed(7 + C)
    return {"weight": (torch.randn((64, C + 6), generator=g) * 0.3).cuda(), "gamma": (torch.rand(64, generator=g) + 0.5).cuda(),
            "beta": (torch.randn(64, generator=g) * 0.2).cuda(), "mean": (torch.randn(64, generator=g) * 0.1).cuda(),
            "var": (torch.rand(64, generator=g) + 0.5).cuda(), "grad": torch.randn((5, GRID, GRID, 64), generator=g).cuda()}


def _prep(clouds, C):
    from liso_amd.networks.pcl_to_feature_grid.pcl_to_feature_grid import pillar_prep

    offsets = [0]
    for p in clouds:
        offsets.append(offsets[-1] + p.shape[0])
    cat = torch.cat(clouds, dim=0).contiguous() if offsets[-1] else torch.zeros((0, C), device="cuda")
    return pillar_prep(cat, offsets, _pcfg(C))


def _consume(prep, C, par, s0, B, sub):
    """statistics (training), dense forward fp32 + bf16, compact forward, backward on samples [s0, s0 + B) of `prep` through the `_sub`
    entry points (`sub`) or -- s0 == 0, the prep holds exactly B samples -- through the plain ones -> every output, by name"""
    from liso_amd import _lib as L

    lib, pcfg, dev = L.lib(), _pcfg(C), torch.device("cuda")
    pt_off, feat, voxel_cell, num_voxels, cell_to_voxel = prep
    assert sub or (s0 == 0 and num_voxels.shape[0] == B)
    st = L.stream_ptr()
    head = (L.ptr(feat), L.ptr(pt_off))
    where = (s0, B) if sub else (B,)
    out = {}
    rm, rv = par["mean"].clone(), par["var"].clone()
    bn_out = torch.zeros(4 * 64, device=dev)
    moments = torch.zeros(80, dtype=torch.float64, device=dev)
    partials = torch.empty(lib.liso_pfn_partials_bytes(), dtype=torch.uint8, device=dev)
    f = lib.liso_pfn_bn_prepare_sub_f32 if sub else lib.liso_pfn_bn_prepare_f32
    L.check(f(*head, ctypes.byref(pcfg), *where, L.ptr(num_voxels), L.ptr(par["weight"]), L.ptr(par["gamma"]), L.ptr(par["beta"]), L.ptr(rm),
              L.ptr(rv), 0.01, 1e-3, 1, L.ptr(bn_out), L.ptr(moments), L.ptr(partials), st), "bn_prepare")
    out.update(bn_out=bn_out, moments=moments, running_mean=rm, running_var=rv)
    head = (*head, L.ptr(voxel_cell), ctypes.byref(pcfg), *where)
    f = lib.liso_pfn_forward_scatter_sub if sub else lib.liso_pfn_forward_scatter
    for name, dtype in (("dense_f32", torch.float32), ("dense_bf16", torch.bfloat16)):
        canvas = torch.full((B, GRID, GRID, 64), 3.0, dtype=dtype, device=dev)  # (every cell must be written: no 3 may survive)
        occ = torch.full((B, 1, GRID, GRID), 3.0, device=dev)
        L.check(f(*head, L.ptr(cell_to_voxel), L.ptr(par["weight"]), L.ptr(bn_out), L.ptr(canvas), L.elem_code(dtype), L.ptr(occ), st), name)
        out[name], out[name + "_occ"] = canvas, occ
    row_base = 7  # (the rows of this call start at row 7 of the array the map indexes)
    rows = torch.zeros((row_base + B * MAX_VOXELS, 64), device=dev)  # (rows of unused pillars are not written: they stay 0 on both sides)
    cmap = torch.full((B, GRID, GRID), -5, dtype=torch.int32, device=dev)
    occ = torch.full((B, 1, GRID, GRID), 3.0, device=dev)
    f = lib.liso_pfn_forward_rows_sub if sub else lib.liso_pfn_forward_rows
    L.check(f(*head, L.ptr(cell_to_voxel), L.ptr(par["weight"]), L.ptr(bn_out), L.ptr(rows[row_base:]), 0, row_base, L.ptr(cmap), L.ptr(occ), st),
            "forward_rows")
    out.update(rows=rows, cell_map=cmap, rows_occ=occ)
    grad = par["grad"][:B].contiguous()  # (the consumer's own gradient canvas: the same values for the same clouds on both sides)
    gw, gg, gb = torch.zeros((64, C + 6), device=dev), torch.zeros(64, device=dev), torch.zeros(64, device=dev)
    f = lib.liso_pfn_backward_sub if sub else lib.liso_pfn_backward
    L.check(f(*head, L.ptr(num_voxels), L.ptr(par["weight"]), L.ptr(par["gamma"]), L.ptr(bn_out), L.ptr(moments), 1, L.ptr(grad), 0, L.ptr(gw),
              L.ptr(gg), L.ptr(gb), L.ptr(partials), st), "backward")
    out.update(grad_weight=gw, grad_gamma=gg, grad_beta=gb)
    torch.cuda.synchronize()
    return out


def _shared(C):
    """the clouds, the parameters and ONE voxelisation of all five clouds per channel count, made once and only read"""
    if C not in _CACHE:
        clouds = _clouds(C)
        _CACHE[C] = (clouds, _params(C), _prep(clouds, C))
    return _CACHE[C]


@pytest.mark.parametrize("C", [4, 5])
def test_the_clouds_are_the_edge_cases_they_claim_to_be(C):
    clouds, _, prep = _shared(C)
    pt_off, _, _, num_voxels, _ = prep
    nv = num_voxels.cpu().tolist()
    assert nv[0] == MAX_VOXELS and nv[1] == 1 and nv[2] == 0 and 0 < nv[4] < MAX_VOXELS, nv  # cloud 0 overflows the pillar cap
    per_pillar = (pt_off[1:] - pt_off[:-1]).view(5, MAX_VOXELS)
    assert int(per_pillar[4].max()) == MAX_POINTS and int(per_pillar[3].max()) == MAX_POINTS  # crowded pillars keep MAX_POINTS points
    kept = per_pillar.sum(dim=1).cpu().tolist()
    assert kept[0] < clouds[0].shape[0] - clouds[0].shape[0] // 7 and kept[4] <= 300 - 40, kept  # out-of-range / surplus points dropped


@pytest.mark.parametrize("C", [4, 5])
@pytest.mark.parametrize("s0,s1", SUB_RANGES)
def test_sub_range_equals_stand_alone_voxelisation(C, s0, s1):
    clouds, par, prep = _shared(C)
    B = s1 - s0
    got = _consume(prep, C, par, s0, B, sub=True)
    alone = _prep([c.clone() for c in clouds[s0:s1]], C)
    ref = _consume(alone, C, par, 0, B, sub=False)
    assert set(got) == set(ref)
    for k in ref:
        assert got[k].shape == ref[k].shape and got[k].dtype == ref[k].dtype, k
        assert torch.equal(got[k], ref[k]), (k, s0, s1, float((got[k].double() - ref[k].double()).abs().max()))
    assert not (ref["dense_f32"] == 3.0).any() and not (ref["dense_f32_occ"] == 3.0).any() and not (ref["cell_map"] < 0).any()
    if (s0, s1) != (1, 3):  # (one point and an empty cloud give one pillar: everything else has gradients to compare)
        assert ref["grad_weight"].abs().sum() > 0 and ref["rows"].abs().sum() > 0


def test_sub_range_arguments_are_checked():
    from liso_amd import _lib as L

    _, par, prep = _shared(4)
    lib, pcfg = L.lib(), _pcfg(4)
    pt_off, feat, voxel_cell, num_voxels, cell_to_voxel = prep
    canvas = torch.empty((1, GRID, GRID, 64), device="cuda")
    occ = torch.empty((1, 1, GRID, GRID), device="cuda")
    bn = torch.zeros(256, device="cuda")
    for s0, B in ((-1, 1), (32, 1), (0, 0), (31, 2)):
        rc = lib.liso_pfn_forward_scatter_sub(L.ptr(feat), L.ptr(pt_off), L.ptr(voxel_cell), ctypes.byref(pcfg), s0, B, L.ptr(cell_to_voxel),
                                              L.ptr(par["weight"]), L.ptr(bn), L.ptr(canvas), 0, L.ptr(occ), L.stream_ptr())
        assert rc < 0, (s0, B, rc)
