"""The builders of tests/pillar_stage_cases.py yield, under the oracle alone, what the GPU stage tests (test_gpu_pillars_stages.py)
rely on: the named pillar sizes, distinct-cell counts, scan blocks, tile counts and runs; fp32 and fp64 voxelisation agree on every
voxeliser case; the near-tie mask of the backward cases stays under 1 %; the host references restate the oracle."""
import numpy as np
import pytest
import torch

from oracle import pillars as OP
from tests import pillar_stage_cases as PC

VOX = PC.voxeliser_cases()


@pytest.mark.parametrize("name", sorted(VOX))
def test_fp32_and_fp64_voxelisation_agree(name):
    """a builder that fails here has put a point where fp32 and fp64 floor differently"""
    c = VOX[name]()
    a = PC.per_sample(c["pcls"], c["geo"], c["max_points"], c["max_voxels"], np.float32)
    b = PC.per_sample(c["pcls"], c["geo"], c["max_points"], c["max_voxels"], np.float64)
    for (n32, c32, p32), (n64, c64, p64) in zip(a, b):
        assert np.array_equal(n32, n64) and np.array_equal(c32, c64) and np.array_equal(p32, p64)
    assert sum(len(p) for p in c["pcls"]) > 0


def test_tile_edge_lengths():
    for which, lengths in PC.TILE_EDGE_LENGTHS.items():
        c = PC.tile_edges(which)
        assert [len(p) for p in c["pcls"]] == lengths
    every = sum(PC.TILE_EDGE_LENGTHS.values(), [])
    assert set([1, 63, 64, 65, 1023, 1024, 1025, 2048, 66560]) <= set(every)
    assert PC.offsets_of(PC.tile_edges("aligned")["pcls"]) == [0, 0, 1024, 1024, 2049]
    for lengths in PC.TILE_EDGE_LENGTHS.values():  # an empty sample first, in the middle, last (or in front of the last)
        assert lengths[0] == 0 and 0 in lengths[1:-1]
    assert PC.TILE_EDGE_LENGTHS["short"][-1] == 0
    c = PC.tile_edges("long")
    assert -(-66560 // 1024) == 65 and -(-66561 // 1024) == 66  # more than 64 tiles; 66: a second trip of the 64-strided base loop
    for p in (c["pcls"][1], c["pcls"][3]):  # pillars are first seen in the first and in the last tile, so every tile's base matters
        n, cc, pi = PC.per_sample([p], c["geo"], 20, 4200)[0]
        first_tile = pi[:, 0] // 1024
        assert first_tile.min() == 0 and first_tile.max() == (len(p) - 1) // 1024 and len(np.unique(first_tile)) == first_tile.max() + 1


def test_runs_cross_waves_and_sample_boundaries():
    c = PC.runs()
    pts = np.concatenate(c["pcls"])
    assert len(pts) % 64 and len(pts) % 256 and len(c["pcls"]) == 3
    for cut in c["cuts"]:
        assert np.array_equal(pts[cut - 1, :2], pts[cut, :2]) and np.isfinite(pts[cut - 1:cut + 1]).all()
        assert cut in PC.offsets_of(c["pcls"])
    cell = np.floor(pts[:, 0] + 32) * 64 + np.floor(pts[:, 1] + 32)
    ok = np.isfinite(cell) & (np.abs(pts[:, 0]) < 32)
    cell = np.where(ok, cell, -1)
    edges = np.flatnonzero(np.diff(cell) != 0) + 1
    run_len = np.diff(np.concatenate([[0], edges, [len(cell)]]))
    assert run_len.max() >= 100 and run_len.min() == 1
    starts = np.concatenate([[0], edges])
    assert any(s // 64 != (s + n - 1) // 64 for s, n in zip(starts, run_len))  # a run over a wave boundary
    bad = np.flatnonzero(~ok)
    assert len(bad) >= 10 and np.isnan(pts[bad]).any() and (pts[bad, 0] > 32).any()
    inside = [i for i in bad if 0 < i < len(cell) - 1 and cell[i - 1] == cell[i + 1] >= 0]
    assert len(inside) >= 10  # dropped points with the same cell on either side


def test_border_probes():
    c = PC.borders()
    pr, geo = c["probes"], c["geo"]
    for axis in range(3):
        mn, mx = np.float32(geo.pc_range[axis]), np.float32(geo.pc_range[axis + 3])
        col = pr[:, axis]
        for v in (mn, mx, np.nextafter(mn, np.float32(-np.inf)), np.nextafter(mn, np.float32(np.inf)), np.nextafter(mx, np.float32(np.inf))):
            assert (col == v).any(), (axis, v)
        assert ((col < mx) & (col > mx - np.float32(1e-3))).any()  # just inside the upper border
        assert np.isposinf(col).any() and np.isneginf(col).any() and np.isnan(col).any()
        assert ((col == 0) & np.signbit(col)).any()
    n, cc, pi = PC.per_sample([np.concatenate(c["pcls"])], geo, 20, 4200)[0]
    kept = set(pi[pi >= 0].tolist())
    allp = np.concatenate(c["pcls"])
    on_min = [i for i in range(len(allp)) if allp[i, 0] == -32 and np.isfinite(allp[i]).all()]
    on_max = [i for i in range(len(allp)) if allp[i, 0] == 32]
    assert on_min and on_max and all(i in kept for i in on_min) and not any(i in kept for i in on_max)


def test_crowded_pillar_sizes_and_blocks():
    for mp in (1, 20, 32):
        c = PC.crowded(mp)
        assert len(c["pcls"]) == 2 and c["max_points"] == mp
        sizes = PC.pillar_sizes(c["pcls"][1], c["geo"])
        assert tuple(sizes[cell] for cell in PC.CROWDED_CELLS) == PC.CROWDED_SIZES == (64, 65, 1024, 1025, 2500)
        assert all(PC.cell_of(c["geo"], 1, x, y) // 1024 > 0 for x, y in PC.CROWDED_CELLS)
        assert sum(PC.pillar_sizes(c["pcls"][0], c["geo"]).values()) > 1000  # points in front of them: their segments start behind a non-zero total
        order = np.concatenate([np.flatnonzero((np.floor(c["pcls"][1][:, 0] + 32) == x) & (np.floor(c["pcls"][1][:, 1] + 32) == y))
                                for x, y in PC.CROWDED_CELLS[2:3]])
        assert order.max() - order.min() > 2 * len(order)  # shuffled among the background


def test_cap_distinct_cells():
    c = PC.cap()
    assert c["max_voxels"] == 50
    assert tuple(len(PC.pillar_sizes(p, c["geo"])) for p in c["pcls"]) == PC.CAP_DISTINCT == (49, 50, 200)
    want = PC.expected_voxelize(c["pcls"], c["geo"], c["max_points"], c["max_voxels"])
    assert list(want["num_voxels"]) == [49, 50, 50]
    p = c["pcls"][2]
    n, cc, pi = PC.per_sample([p], c["geo"], 20, 50)[0]
    kept = np.zeros(len(p), bool)
    kept[pi[pi >= 0]] = True
    assert (~kept[:-1] & kept[1:]).sum() > 20  # dropped pillars' points lie between kept ones


def test_large_case_scan_blocks():
    c = PC.large()
    geo = c["geo"]
    assert (geo.gx, geo.gy, len(c["pcls"]), c["max_voxels"]) == (1024, 1024, 4, 64) and 4 * geo.cells == 4096 * 1024
    blocks = set()
    for b, p in enumerate(c["pcls"]):
        sizes = PC.pillar_sizes(p, geo)
        assert 35 <= len(sizes) <= 40 and 1 <= min(sizes.values()) and max(sizes.values()) <= 30
        for (x, y) in sizes:
            cell = PC.cell_of(geo, b, x, y)
            if cell % 1024 in (0, 1023):
                blocks.add((cell // 1024, cell % 1024))
    for blk in PC.LARGE_BLOCKS:
        assert (blk, 0) in blocks and (blk, 1023) in blocks
    assert PC.LARGE_BLOCKS == (0, 1, 255, 256, 1023, 1024, 2047, 2048, 4094, 4095)


def test_non_square_cases():
    for gx, gy in ((96, 160), (160, 96)):
        c = PC.non_square(gx, gy)
        sizes = PC.pillar_sizes(c["pcls"][0], c["geo"])
        assert (c["geo"].gx, c["geo"].gy) == (gx, gy) and gx != gy
        assert max(x for x, _ in sizes) == gx - 1 and max(y for _, y in sizes) == gy - 1  # the longer axis is used beyond the shorter extent


@pytest.mark.parametrize("C", [3, 4, 5])
def test_pfn_cloud_and_decorate_expectation(C):
    geo = PC.Geo(64, 64, 1.0)
    pcls = PC.pfn_cloud(3, geo, C, 3000, 2)
    for mv in (1023, 40000):
        e = PC.expected_decorate(pcls, geo, 20, mv)
        for b, p in enumerate(pcls):
            sizes = PC.pillar_sizes(p, geo)
            assert sizes[PC.PFN_RESERVED["one"]] == 1 and sizes[PC.PFN_RESERVED["full"]] == 20 and sizes[PC.PFN_RESERVED["over"]] == 27
            assert all(sizes[k] >= 3 for k in ((0, 0), (0, 63), (63, 0), (63, 63)))
            assert e["voxel_cell"][b * mv] == PC.cell_of(geo, b, *PC.PFN_RESERVED["one"])  # the reserved pillars come first: no cap drops them
        kept = np.diff(e["pt_off"])
        assert {1, 20} <= set(kept.tolist()) and kept.max() == 20 and e["pt_off"][-1] == len(e["rows"])
        assert (e["voxel_cell"] >= 0).sum() == (kept > 0).sum() == len(e["num"])
        if mv == 1023:
            assert (kept > 0).all()  # the cap is hit: every row holds a pillar
        cat = np.concatenate(pcls)
        assert np.abs(cat[:, :2]).max() > 31.9
        if C > 3:
            assert cat[:, 3].max() > 200 and np.array_equal(e["rows"][:, 3:C], cat[e["point"], 3:C].astype(np.float64))
        assert np.array_equal(e["rows"][:, C + 3:C + 6], e["rows"][:, 0:3])
        # the fp64 rows and the oracle's fp32 rows are the same function
        e32 = PC.expected_decorate(pcls, geo, 20, mv, dtype=torch.float32)
        assert np.abs(e32["rows"] - e["rows"]).max() <= 16 * PC.U32 * 32.0


def test_stage_references_restate_the_oracle():
    """moments / BatchNorm / forward references (written for device rows) against oracle.pillars.pfn_layer on the oracle's own rows"""
    C, geo = 5, PC.Geo(64, 64, 1.0)
    pcls = PC.pfn_cloud(9, geo, C, 1500, 2)
    prm = PC.pfn_params(9, C)
    e = PC.expected_decorate(pcls, geo, 20, 40000)
    feat = np.zeros((len(e["rows"]), 12))
    feat[:, :C + 6], feat[:, C + 6] = e["rows"], 1.0
    P = len(e["num"])
    tot, mag = PC.moments_reference(feat, C)
    assert len(tot) == (C + 7) * (C + 8) // 2 and tot[-1] == len(feat) and (mag >= np.abs(tot) - 1e-9).all()
    assert tot[PC.pair_index(C + 6, C + 6, C + 7)] == len(feat)
    for training in (True, False):
        bn = PC.bn_reference(feat, C, P, 20, prm, training)
        t = {k: torch.from_numpy(v).double() for k, v in prm.items()}
        v, n, c, _ = OP.voxelize_batch(pcls, geo.voxel_size, geo.pc_range, 20, 40000)
        feats = OP.pfn_decorate(torch.from_numpy(v).double(), torch.from_numpy(n), torch.from_numpy(c), geo.voxel_size, geo.pc_range)
        want = OP.pfn_layer(feats, t["weight"], t["gamma"], t["beta"], t["running_mean"], t["running_var"], training, PC.MOMENTUM, PC.EPS).numpy()
        idx, val, bnd = PC.forward_reference(feat, e["pt_off"], 20, C, prm["weight"], np.concatenate([bn["scale"], bn["shift"]]))
        assert len(idx) == P and np.abs(val - want).max() <= 1e-9 * max(1.0, np.abs(want).max()) and (bnd > 0).all()
        if training:
            assert np.allclose(bn["running_mean"], t["running_mean"].numpy(), rtol=1e-12, atol=1e-14)
            assert np.allclose(bn["running_var"], t["running_var"].numpy(), rtol=1e-12, atol=1e-14)
            assert not np.allclose(bn["running_mean"], prm["running_mean"])
    empty = PC.bn_reference(np.zeros((0, 12)), C, 0, 20, prm, True)
    assert (empty["mean"] == 0).all() and np.allclose(empty["invstd"], 1 / np.sqrt(PC.EPS)) and np.array_equal(empty["running_var"], prm["running_var"].astype(np.float64))


@pytest.mark.parametrize("B,C,training,gdtype", PC.BACKWARD_CASES)
def test_near_tie_mask_stays_under_one_percent(B, C, training, gdtype):
    c = PC.backward_case(B, C, training, gdtype)
    s = c["stats"]
    assert 3000 <= sum(len(p) for p in c["pcls"]) <= 6000
    assert s["entries"] > 0 and s["masked"] <= 0.01 * s["entries"], s
    assert s["full"] >= B and s["padding_wins"] > 0, s  # full pillars, and pillars where the padding candidate wins
    assert c["prm"]["beta"].min() < 0 < c["prm"]["beta"].max() and 0.5 <= c["prm"]["gamma"].min() and c["prm"]["gamma"].max() <= 1.5
    g = c["grad"]
    assert g.shape == (B, 64, 64, 64) and g.dtype == np.float32
    if gdtype != "fp32":
        assert np.array_equal(torch.from_numpy(g).to(PC.TORCH_DTYPE[gdtype]).float().numpy(), g)


def test_backward_reference_fp32_and_fp64_are_close_and_masked_entries_are_zero():
    c = PC.backward_case(1, 4, 1, "fp32")
    keep, cells, _ = PC.near_tie_keep(c["pcls"], c["geo"], 20, 40000, c["prm"], 1)
    g = c["grad"].reshape(-1, 64)
    assert (g[cells][~keep] == 0).all() and (g[cells][keep] != 0).all()
    g64 = PC.oracle_gradients(c["pcls"], c["geo"], 20, 40000, c["prm"], 1, c["grad"], torch.float64)
    g32 = PC.oracle_gradients(c["pcls"], c["geo"], 20, 40000, c["prm"], 1, c["grad"], torch.float32)
    for k in g64:
        assert np.isfinite(g64[k]).all() and np.abs(g64[k]).max() > 0
        assert np.abs(g32[k] - g64[k]).max() <= 1e-3 * np.abs(g64[k]).max(), k
