"""liso_pillars_voxelize_f32 (liso_amd/csrc/pillars.hip) bit for bit against the oracle's voxeliser on clouds built around the first
kernel of the pass: assign_kernel issues one returning add and one max per run of equal cells in a wave and hands every member of the
run base + offset.  Counts, first points, coors, num_points, the slots (arrival order) and cell_to_voxel are properties of the index
set and must not depend on how the points were grouped, nor on the order the atomics ran in: one pillar taking a whole cloud (more
than max_points), equal cells interleaved lane by lane (every run one point long, the same counters hit from many lanes), runs that
span a wave boundary (two adds), points outside the range inside the runs, an empty second cloud, a second cloud that starts inside
a wave, and the pillar cap below and above the pillar count.  Every device buffer lies between guard bands (tests/guarded_alloc.py)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import pillar_stage_cases as PC
from tests.guarded_alloc import guarded

pytestmark = pytest.mark.gpu
DEV = "cuda"
GEO = PC.Geo(24, 40, 0.5)  # non-square
MAX_POINTS = 20
SIZES = (1, 64, 65, 4096)


def _L():
    from liso_amd import _lib as L

    return L


def dev(a):
    src = torch.from_numpy(np.ascontiguousarray(a))
    t = torch.empty(tuple(src.shape), dtype=src.dtype, device=DEV)
    t.copy_(src)
    return t


def poisoned(shape, dtype):
    t = torch.empty(tuple(shape), dtype=dtype, device=DEV)
    t.view(-1).view(torch.uint8).fill_(PC.PATTERN)
    return t


def assert_bits(what, got, want):
    got = got.cpu().numpy()
    want = np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.size} of {got.size} elements differ, first at flat index {i} (shape {got.shape}): "
                             f"got {got.reshape(-1)[i]!r}, want {want.reshape(-1)[i]!r}")


def cells_of(pattern, n):
    """(x cell, y cell) of every point, [n, 2]; cells outside the grid give points outside the range"""
    j = np.arange(n)
    gx, gy = GEO.gx, GEO.gy
    if pattern == "one pillar":
        c = np.full(n, 7 * gy + 3)
    elif pattern == "interleaved lane by lane":  # 2, 3 and 5 pillars taking turns, a different mix in every wave
        k = 2 + (j // 64) % 3 + (j // 64) % 2
        c = (j % k) * 41 + (j // 64) % 5
    elif pattern == "groups across wave boundaries":  # runs of 48 (a run covers lanes 48..63 | 0..31) that come back 96 points later
        c = (j // 48) % 2 * 100 + 13
    elif pattern == "every point its own pillar":
        c = j % (gx * gy)
    else:
        raise KeyError(pattern)
    xy = np.stack([c // gy, c % gy], 1)
    if pattern != "one pillar" or n > 1:
        out = j % 9 == 4  # points outside the range, inside the groups
        xy[out] = np.array([[-1, 0], [gx, 3], [2, -1], [5, gy]])[j[out] % 4]
    return xy


PATTERNS = ("one pillar", "interleaved lane by lane", "groups across wave boundaries", "every point its own pillar")


def make_cfg(max_voxels):
    c = _L().PillarCfg()
    c.x_min, c.y_min, c.z_min = (float(v) for v in GEO.pc_range[:3])
    c.vx, c.vy, c.vz = (float(v) for v in GEO.voxel_size)
    c.gx, c.gy, c.max_points, c.max_voxels, c.n_channels = GEO.gx, GEO.gy, MAX_POINTS, max_voxels, 4
    return c


def voxelize(pcls, cfg):
    L = _L()
    lib = L.lib()
    B, offsets = len(pcls), PC.offsets_of(pcls)
    points = dev(np.concatenate(pcls))
    nbytes = lib.liso_pillars_voxelize_workspace_bytes(ctypes.byref(cfg), B, offsets[-1])
    assert nbytes > 0
    rows, i32 = B * cfg.max_voxels, torch.int32
    out = dict(coors=poisoned((rows, 4), i32), num_points=poisoned((rows,), i32), slots=poisoned((rows, cfg.max_points), i32),
               num_voxels=poisoned((B,), i32), cell_to_voxel=poisoned((B * cfg.gx * cfg.gy,), i32))
    ws = poisoned((nbytes,), torch.uint8)
    rc = lib.liso_pillars_voxelize_f32(L.ptr(points), (ctypes.c_int * len(offsets))(*offsets), B, ctypes.byref(cfg), L.ptr(out["coors"]),
                                       L.ptr(out["num_points"]), L.ptr(out["slots"]), L.ptr(out["num_voxels"]),
                                       L.ptr(out["cell_to_voxel"]), L.ptr(ws), nbytes, L.stream_ptr())
    assert rc == 0
    return out


@pytest.mark.parametrize("second", ["alone", "empty second cloud", "second cloud of 65"])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_voxeliser_bit_for_bit_however_the_cells_interleave(pattern, second):
    for n in SIZES:
        rng = np.random.default_rng(n + len(pattern))
        pcls = [PC.lattice_points(rng, GEO, cells_of(pattern, n), 4)]
        if second == "empty second cloud":
            pcls.append(np.zeros((0, 4), np.float32))
        elif second == "second cloud of 65":  # the second sample starts inside a wave of the first one's last points
            pcls.append(PC.lattice_points(rng, GEO, cells_of("interleaved lane by lane", 65), 4))
        pillars = max(len(PC.pillar_sizes(p, GEO)) for p in pcls)
        for max_voxels in sorted({max(pillars - 1, 1), pillars + 3}):  # the cap below and above the pillar count
            want = PC.expected_voxelize(pcls, GEO, MAX_POINTS, max_voxels)
            with guarded() as gd:
                out = voxelize(pcls, make_cfg(max_voxels))
                gd.check()
            for k in ("num_voxels", "coors", "num_points", "cell_to_voxel", "slots"):
                assert_bits(f"{pattern}, {second}, n={n}, max_voxels={max_voxels}: {k}", out[k], want[k])
