"""liso_kabsch_trafos_counted_f32 (liso_amd/csrc/kabsch.hip) at the edges of kabsch_solve_kernel: one wave per slot adds the slot's
row of the block partials in fp64 -- lane l takes the blocks l, l + 64, ..., eight loads in flight -- and reduces the uniform moments
only where the epsilon rule needs them (a slot whose fp32 weight is below 1e-12).

  slots   S = 1, 17, 64 (+ the background slot S)
  blocks  1, 63, 64, 65 and 512 point blocks per sample (128 points per tile): lanes without a block, exactly one block per lane,
          the second round of the lane-strided loop, all eight rounds (two tiles per block)
  weights a box 4 km away (sigmoid masks: weight exactly 0), boxes whose only point lies so far outside that the weight is
          ~0.93e-12 / ~1.14e-12 (either side of the rule; the test checks from cum_wts that each landed on its side), ordinary boxes

The order of the summation is part of the result's bits, so the outputs must EQUAL tests/golden/kabsch_solve_edges.npz: the
outputs of the build before the kernel was changed, recorded on an MI355X by `python -m tests.test_gpu_kabsch_solve_edges <out.npz>`.
A numpy restatement cannot give those bits (the kernels are compiled with contraction on), so the oracle (oracle/kabsch.py, fp32 like
the reference) is compared at the 1e-3 relative tolerance of tests/test_gpu_kabsch.py: the weights of every slot, and the transforms
of the slots where the alignment is well conditioned -- uniform weights by the rule, or at least FIRM points' worth of weight: the
cross-covariance sum w (y - my)(x - mx)^T with y = x + flow is then the points' own spread (~0.5 m^2 in a 2 m box) plus a smaller flow
term (0.3 m noise), both singular values are of that order, and fp32 rounding of the moments (1e-6) moves R by about as little.  A box
that holds one or two points has a singular cross-covariance and no defined rotation; only its weight is compared."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
REL = 1e-3
FIRM = 20.0
SLOPE, BUFFER = 15.0, 0.25
SLOTS = (1, 17, 64)
BLOCKS = {1: 100, 63: 63 * 128 - 5, 64: 64 * 128, 65: 64 * 128 + 1, 512: 513 * 128 - 51}  # point blocks -> points per sample
KINDS = ("boxed", "zero", "below", "above", "boxed")
T_OUT = {"below": 27.70, "above": 27.50}  # slope * distance outside the box: sigmoid -> e^-t, 1e-12 = e^-27.631
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "kabsch_solve_edges.npz")


def kind_of(S, nblk, s):
    return KINDS[(s + (list(BLOCKS).index(nblk) if S == 1 else 0)) % len(KINDS)]


def case(S, nblk):
    """-> dict of numpy inputs: pts [B,N,3], flow [B,N,2], valid [B,N], pos / dims [B,S,3], rot [B,S,1]"""
    N = BLOCKS[nblk]
    B = 1 if nblk == 512 else 2
    rng = np.random.default_rng(1000 * S + nblk)
    pts = np.concatenate([rng.uniform(-45, 45, (B, N, 2)), rng.uniform(-2, 1, (B, N, 1))], -1).astype(np.float32)
    flow = (rng.normal(0, 0.3, (B, N, 2)) + np.array([0.5, -0.2])).astype(np.float32)
    valid = rng.random((B, N)) > 0.1
    pos = np.concatenate([rng.uniform(-35, 35, (B, S, 2)), np.full((B, S, 1), -0.7)], -1).astype(np.float32)
    dims = rng.uniform(2.0, 5.0, (B, S, 3)).astype(np.float32)
    rot = rng.uniform(-3.1, 3.1, (B, S, 1)).astype(np.float32)
    spare = 0  # the first rows of every cloud become the single points of the below / above slots
    for s in range(S):
        k = kind_of(S, nblk, s)
        if k == "boxed":
            continue
        dims[:, s], rot[:, s] = 4.0, 0.0  # half extents 1.5 m at scale 0.75
        if k == "zero":
            pos[:, s, :2] = 4000.0
        else:  # boxes 10 m apart beyond the cloud: every other point is > 100 slope units outside (sigmoid == 0 in fp32)
            pos[:, s, 0], pos[:, s, 1] = 70.0 + 10.0 * spare, 0.0
            pts[:, spare] = pos[:, s] + np.array([1.5 + T_OUT[k] / SLOPE, 0.0, 0.0], np.float32)
            valid[:, spare] = True
            spare += 1
    assert spare < N
    return dict(pts=pts, flow=flow, valid=valid, pos=pos, dims=dims, rot=rot)


def run(c):
    """the entry point on one case -> (trafos [B,S+1,4,4] f64, cum_wts [B,S+1] f32) as numpy"""
    from liso_amd import _lib as L

    lib = L.lib()
    B, N, _ = c["pts"].shape
    S = c["pos"].shape[1]
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in c.items()}
    val = d["valid"].to(torch.uint8).contiguous()
    rot = d["rot"][..., 0].contiguous()
    cfg = L.KabschCfg(B, N, S, 3, 2, SLOPE, 1.0 - BUFFER, 1.0 + BUFFER, 1)  # sigmoid masks
    T = torch.full((B, S + 1, 4, 4), float("nan"), dtype=torch.float64, device="cuda")
    cum = torch.full((B, S + 1), float("nan"), dtype=torch.float32, device="cuda")
    nbytes = lib.liso_kabsch_workspace_bytes(ctypes.byref(cfg))
    ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device="cuda")
    rc = lib.liso_kabsch_trafos_counted_f32(ctypes.byref(cfg), L.ptr(d["pts"]), L.ptr(val), L.ptr(d["flow"]), L.ptr(d["pos"]), L.ptr(d["dims"]),
                                            L.ptr(rot), None, L.ptr(T), L.ptr(cum), None, L.ptr(ws), nbytes, L.stream_ptr())
    assert rc == 0, rc
    return T.cpu().numpy(), cum.cpu().numpy()


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("nblk", list(BLOCKS))
@pytest.mark.parametrize("S", SLOTS)
def test_solve_equals_the_recorded_bits_and_agrees_with_the_oracle(S, nblk, golden):
    from oracle import kabsch as OK

    c = case(S, nblk)
    T, cum = run(c)
    N = c["pts"].shape[1]
    # every slot landed on the side of the epsilon rule it was built for
    rule = np.float32(np.float64(np.float32(1e-12)) * N)
    for s in range(S):
        k = kind_of(S, nblk, s)
        if k in ("zero", "below"):
            assert np.all(cum[:, s] == rule), (s, k, cum[:, s], rule)
        elif k == "above":
            assert np.all((cum[:, s] >= np.float32(1e-12)) & (cum[:, s] < np.float32(1.3e-12))), (s, cum[:, s])
    assert np.all(cum[:, S] > 1.0)  # the background slot holds the cloud
    # the bits of the build before the change
    want_T, want_cum = golden[f"T_{S}_{nblk}"], golden[f"cum_{S}_{nblk}"]
    assert T.shape == want_T.shape and cum.shape == want_cum.shape
    assert T.tobytes() == want_T.tobytes(), f"{int((T.view(np.uint64) != want_T.view(np.uint64)).sum())} of {T.size} trafo entries differ"
    assert cum.tobytes() == want_cum.tobytes(), f"{int((cum.view(np.uint32) != want_cum.view(np.uint32)).sum())} of {cum.size} weights differ"
    # the host restatement
    t = {k: torch.from_numpy(v) for k, v in c.items()}
    oT, ocum, _ = OK.kabsch_trafos(t["pos"], t["dims"], t["rot"], t["pts"], t["valid"], t["flow"], slope=SLOPE, buffer=BUFFER, softness="sigmoid")
    oT, ocum = oT.numpy(), ocum.numpy()
    assert np.abs(cum - ocum).max() <= REL * np.abs(ocum).max()
    assert np.all(np.abs(cum - ocum) <= REL * np.abs(ocum) + 1e-30)
    firm = (ocum >= FIRM) | (np.abs(ocum - rule) <= REL * rule)
    assert firm[:, S].all() and firm.sum() >= firm.shape[0]
    assert np.abs(T - oT)[firm].max() <= REL * max(np.abs(oT[firm]).max(), 1e-12)


if __name__ == "__main__":  # records the fixture: run on the build whose bits are to be kept
    out = {}
    for S_ in SLOTS:
        for nblk_ in BLOCKS:
            out[f"T_{S_}_{nblk_}"], out[f"cum_{S_}_{nblk_}"] = run(case(S_, nblk_))
    np.savez_compressed(sys.argv[1], **out)
    print("wrote", sys.argv[1], sum(v.nbytes for v in out.values()), "bytes")
