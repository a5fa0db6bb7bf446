"""GPU: the cone test and the order-preserving compaction (liso_ground_cone_f32, liso_ground_compact_f32 through
remove_ground_points) at their edges, against numpy boolean selection in fp64: cloud lengths around the scan's chunk of 2048,
3, 4 and 5 floats per row, counts below the padded length, NaN rows in the middle, nothing and everything kept, and the cone's
output written over its `or_with` input.  The kept rows must be identical and in order, NaN behind them, the counts exact.
The clouds (tests/ground_stage_cases.py: removal_batch) meet the near-tie condition, asserted on the CPU as well."""
import numpy as np
import pytest
import torch

import ground_stage_cases as C
from liso_amd import _lib as L
from liso_amd.jcp.jcp import cone_device, remove_ground_points

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
CONE = (-1.70, 0.8)


def check_removal(batch, counts, ground, out, kept, is_ground):
    """ground: expected bool per counted row, per cloud"""
    B, N, _ = batch.shape
    out, kept, is_ground = out.cpu().numpy(), kept.cpu().numpy(), is_ground.cpu().numpy()
    assert out.shape == batch.shape and out.dtype == np.float32 and kept.dtype == np.int32 and is_ground.dtype == np.bool_
    for b in range(B):
        n = int(counts[b])
        rows = batch[b, :n]
        valid = ~np.isnan(rows[:, :3]).any(-1)
        want = rows[valid & ~ground[b]]
        assert np.array_equal(is_ground[b, :n], ground[b] & valid) and not is_ground[b, n:].any(), b
        assert kept[b] == want.shape[0], (b, kept[b], want.shape[0])
        assert np.array_equal(out[b, : kept[b]], want), b  # identical rows, in order, every column
        assert np.isnan(out[b, kept[b]:]).all(), b


@pytest.mark.parametrize("stride", [3, 4, 5])
@pytest.mark.parametrize("N", C.REMOVAL_N)
def test_removal_around_the_scan_chunk(N, stride):
    batch, counts = C.removal_batch(N, stride)
    ground = []
    for b in range(3):
        n = int(counts[b])
        if n == 0:
            ground.append(np.zeros(0, bool))
            continue
        jcp, info = C.removal_host(N, b)
        assert C.near_tie_figures(info)[0] == 0 and min(C.near_tie_figures(info)[1:]) >= 1e-9, (N, b)
        ground.append(jcp | C.cone_labels(batch[b, :n, :3], *CONE))
    t = torch.from_numpy(np.array(batch)).to(DEV)
    out, kept, is_ground = remove_ground_points(t, cone=CONE, counts=torch.from_numpy(counts).to(DEV), **C.REMOVAL_PARAMS)
    print(f"N {N}, stride {stride}: counts {counts.tolist()}, kept {kept.tolist()}")
    check_removal(batch, counts, ground, out, kept, is_ground)
    if N > 1:
        assert all(0 < int(k) < int(n) for k, n in zip(kept, counts))


@pytest.mark.parametrize("N", [2047, 2049])
def test_nothing_kept_and_everything_kept(N):
    batch, counts = C.removal_batch(N, 4)
    t = torch.from_numpy(np.array(batch)).to(DEV)
    dcounts = torch.from_numpy(counts).to(DEV)
    # a cone threshold above every point: all ground
    out, kept, is_ground = remove_ground_points(t, cone=(1e9, 0.0), counts=dcounts, **C.REMOVAL_PARAMS)
    check_removal(batch, counts, [np.ones(int(n), bool) for n in counts], out, kept, is_ground)
    assert not kept.any() and torch.isnan(out).all()
    # every point beyond the 70 m the range image covers and above the cone: none ground, the valid rows move up over the NaN rows
    far = np.array(batch)
    far[..., 0] += np.float32(200.0)
    out, kept, is_ground = remove_ground_points(torch.from_numpy(far).to(DEV), cone=(-1e9, 0.0), counts=dcounts, **C.REMOVAL_PARAMS)
    check_removal(far, counts, [np.zeros(int(n), bool) for n in counts], out, kept, is_ground)
    nan_rows = [int(np.isnan(far[b, : counts[b], :3]).any(-1).sum()) for b in range(3)]
    assert nan_rows[0] == 3 and nan_rows[1] == 1 and kept.tolist() == [int(n) - k for n, k in zip(counts, nan_rows)]


@pytest.mark.parametrize("stride", [3, 5])
@pytest.mark.parametrize("N", C.REMOVAL_N)
def test_cone_written_over_its_or_input(N, stride):
    batch, counts = C.removal_batch(N, stride)
    g = np.random.default_rng(N)
    prior = g.random((3, N)) < 0.3
    want, want_alone = np.zeros((3, N), bool), np.zeros((3, N), bool)
    for b in range(3):
        n = int(counts[b])
        valid = ~np.isnan(batch[b, :n, :3]).any(-1)
        want_alone[b, :n] = C.cone_labels(batch[b, :n, :3], *CONE) & valid
        want[b, :n] = (prior[b, :n] & valid) | want_alone[b, :n]
    t = torch.from_numpy(np.array(batch)).to(DEV)
    dcounts = torch.from_numpy(counts).to(DEV)
    dprior = torch.from_numpy(prior).to(DEV)
    apart = cone_device(t, *CONE, counts=dcounts, or_with=dprior)
    assert np.array_equal(apart.cpu().numpy(), want)
    assert np.array_equal(dprior.cpu().numpy(), prior)  # the input is left alone when the output is elsewhere
    alone = cone_device(t, *CONE, counts=dcounts)
    assert np.array_equal(alone.cpu().numpy(), want_alone) and (N == 1 or 0 < int(want_alone.sum()) < int(counts.sum()))
    # out aliasing or_with, through the C entry point
    inout = dprior.clone().view(torch.uint8)
    slope = float(np.tan(CONE[1] / 180.0 * np.pi))
    with torch.cuda.device(DEV):
        L.check(L.lib().liso_ground_cone_f32(3, N, stride, L.ptr(t), L.ptr(dcounts), CONE[0], slope, L.ptr(inout), L.ptr(inout), L.stream_ptr()),
                "ground cone in place")
    assert np.array_equal(inout.cpu().numpy().astype(bool), want) and set(np.unique(inout.cpu().numpy()).tolist()) <= {0, 1}
