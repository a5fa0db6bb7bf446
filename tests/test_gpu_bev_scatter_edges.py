"""liso_bev_dynamic_flow_f32 (liso_amd/csrc/flow_cluster.hip) bit for bit against int64 sums in numpy, at the sizes and cell
patterns where the scatter takes another path: a block merges the equal cells of its 1024-point chunk in an LDS table of 512 slots
(16 linear probes) before it touches global memory, and a cell without a slot adds directly.

The inputs are chosen so that the host restatement has no rounding of its own to argue about: the odometry is the identity
(inv(odom) - I = 0, the static flow is exactly 0 whether or not the compiler contracts the fp64 products), and the flow components
are multiples of 1/16 m up to +-100 m (squares and their sum are exact in fp32, so |flow| is one correctly rounded sqrt).  The
fixed-point sums are integers: any grouping gives the same bits.  The workspace holds one 40-byte record per pillar and is exactly
the size the query names.  Every device buffer lies between guard bands (tests/guarded_alloc.py)."""
import numpy as np
import pytest
import torch

from tests.guarded_alloc import guarded

pytestmark = pytest.mark.gpu
DEV = "cuda"
PATTERN = 0xA5
EWORKSPACE = -2
CHUNK, SLOTS, SLOT_BITS, PROBES = 1024, 512, 9, 16
SIZES = (1, 63, 64, 65, 1023, 1024, 1025, 5000)


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
    t.view(-1).view(torch.uint8).fill_(PATTERN)
    return t


def assert_bits(what, got, want):
    got = got.cpu().numpy()
    want = np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero(got.reshape(-1).view(np.uint32) != want.reshape(-1).view(np.uint32))
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.size} of {got.size} elements differ, first at flat index {i}: "
                             f"got {got.reshape(-1)[i]!r}, want {want.reshape(-1)[i]!r}")


def home_slot(cell):
    """the table slot a cell id hashes to (flow_cluster.hip: 32-bit multiplicative hash, top SLOT_BITS bits)"""
    return ((np.asarray(cell, np.uint64) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - SLOT_BITS)


def cell_patterns(n, cells):
    """name -> per-point cell index inside one sample, [n]"""
    j = np.arange(n)
    slot = home_slot(np.arange(cells))
    crowd = np.flatnonzero((slot >= 100) & (slot < 108))  # more keys than the 8 + PROBES - 1 slots they can reach
    out = {
        "one cell": np.full(n, cells - 2),
        "every point its own cell": j % cells,  # (48 x 64: 1024 distinct cells per chunk, twice the table)
        "two cells alternating": np.where(j % 2 == 0, 3, cells - 1),
        "runs of 100 across waves and chunks": (j // 100) * 7 % cells,
        "random": np.random.default_rng(n).integers(0, cells, n),
    }
    if crowd.size > 8 + PROBES:
        out["colliding keys"] = crowd[j % crowd.size]
    return out


def reference(valid, rows, cols, flow, B, h, w):
    """dynamicness [B,h,w,1], nonrigid flow [B,h,w,3]: int64 fixed-point sums per pillar, the kernel's divide rule"""
    f = flow.astype(np.float32)
    length = np.sqrt(f[..., 0] * f[..., 0] + f[..., 1] * f[..., 1] + f[..., 2] * f[..., 2]).astype(np.float32)
    q = np.rint(np.concatenate([length[..., None], f], -1).astype(np.float64) * 16777216.0).astype(np.int64)  # [B,N,4]
    ok = (valid != 0) & (rows >= 0) & (rows < h) & (cols >= 0) & (cols < w)
    cell = (np.arange(B)[:, None] * h + rows) * w + cols
    sums = np.zeros((B * h * w, 4), np.int64)
    np.add.at(sums, cell[ok], q[ok])
    cnt = np.bincount(cell[ok], minlength=B * h * w)
    v = (sums.astype(np.float64) / 16777216.0).astype(np.float32)
    many = cnt > 1
    v[many] = v[many] / cnt[many, None].astype(np.float32)
    v = v.reshape(B, h, w, 4)
    return v[..., :1].copy(), v[..., 1:].copy()


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("h,w", [(8, 8), (48, 64)])
def test_scatter_means_bit_for_bit(h, w, B):
    L = _L()
    lib = L.lib()
    nbytes = lib.liso_bev_dynamic_flow_workspace_bytes(B, h, w)
    assert nbytes == 40 * B * h * w
    ome = dev(np.zeros((B, 4, 4), np.float64))
    for n in SIZES:
        rng = np.random.default_rng(1000 * n + 10 * h + B)
        for what, cell in cell_patterns(n, h * w).items():
            cell = np.stack([(cell + 5 * b) % (h * w) for b in range(B)])  # [B,n]
            rows, cols = (cell // w).astype(np.int32), (cell % w).astype(np.int32)
            j = np.arange(n)
            valid = np.broadcast_to((j % 7 != 3).astype(np.uint8), (B, n)).copy()
            outside = j % 11 == 5
            rows[:, outside] = np.array([-1, h, 0, 2 ** 30])[j[outside] % 4]
            cols[:, outside] = np.array([0, 0, w, -(2 ** 30)])[j[outside] % 4]
            flow = (rng.integers(-1600, 1601, (B, n, 3)) / 16.0).astype(np.float32)
            pts = rng.uniform(-50, 50, (B, n, 3)).astype(np.float32)
            want_dyn, want_nrf = reference(valid, rows, cols, flow, B, h, w)
            tag = f"{what}, n={n}"
            with guarded() as gd:
                args = dev(pts), dev(valid), dev(np.stack([rows, cols], -1)), dev(flow)
                dyn, nrf = poisoned((B, h, w, 1), torch.float32), poisoned((B, h, w, 3), torch.float32)
                ws = poisoned((nbytes,), torch.uint8)
                rc = lib.liso_bev_dynamic_flow_f32(L.ptr(args[0]), 3, L.ptr(args[1]), L.ptr(args[2]), L.ptr(args[3]), 3, L.ptr(ome),
                                                   B, n, h, w, L.ptr(dyn), L.ptr(nrf), L.ptr(ws), nbytes, L.stream_ptr())
                assert rc == 0, (tag, rc)
                assert_bits(f"dynamicness ({tag})", dyn, want_dyn)
                assert_bits(f"nonrigid flow ({tag})", nrf, want_nrf)
                gd.check()


def test_the_patterns_reach_the_paths_they_are_named_for():
    """the overflow path needs more distinct cells in a chunk than the table holds, or more colliding keys than a probe sequence"""
    own = cell_patterns(CHUNK, 48 * 64)["every point its own cell"]
    assert np.unique(own[:CHUNK]).size > SLOTS
    crowd = cell_patterns(CHUNK, 48 * 64)["colliding keys"]
    assert np.unique(crowd).size > 8 + PROBES - 1 and np.all((home_slot(crowd) >= 100) & (home_slot(crowd) < 108))


def test_a_workspace_below_the_record_size_is_refused():
    L = _L()
    lib = L.lib()
    B, n, h, w = 1, 4, 8, 8
    z = torch.zeros(64, dtype=torch.float64, device=DEV)
    nbytes = 40 * B * h * w - 1
    assert nbytes == lib.liso_bev_dynamic_flow_workspace_bytes(B, h, w) - 1
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    rc = lib.liso_bev_dynamic_flow_f32(L.ptr(z), 3, L.ptr(z), L.ptr(z), L.ptr(z), 3, L.ptr(z), B, n, h, w, L.ptr(z), L.ptr(z),
                                       L.ptr(ws), nbytes, L.stream_ptr())
    assert rc == EWORKSPACE
