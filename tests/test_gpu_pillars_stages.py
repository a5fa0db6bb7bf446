"""Every entry point of include/liso_pillars.h (liso_amd/csrc/pillars.hip) on its own: the voxeliser bit for bit against
oracle.pillars at the sizes where its kernels take another path, each float stage against fp64 within a bound derived from its
arithmetic.  Builders and host expectations: tests/pillar_stage_cases.py (proved on the CPU by tests/test_pillar_stage_cases.py).
Outputs are pre-filled with a byte pattern and compared in full; every device buffer lies between guard bands
(tests/guarded_alloc.py)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import pillar_stage_cases as PC
from tests.fp16_checks import assert_fp16_rounded
from tests.guarded_alloc import guarded

pytestmark = pytest.mark.gpu
DEV = "cuda"
EINVAL, EWORKSPACE = -1, -2
NAN_PATTERN = 0xFF  # all-ones bytes: a NaN in fp32, fp16 and bf16
VOX = PC.voxeliser_cases()
U = PC.U32


def _L():
    from liso_amd import _lib as L

    return L


def dev(a):
    src = torch.from_numpy(np.ascontiguousarray(a))
    t = torch.empty(tuple(src.shape), dtype=src.dtype, device=DEV)
    t.copy_(src)
    return t


def poisoned(shape, dtype, pattern=PC.PATTERN):
    t = torch.empty(tuple(shape), dtype=dtype, device=DEV)
    t.view(-1).view(torch.uint8).fill_(pattern)
    return t


def host(t):
    return t.cpu().numpy()


def assert_bits(what, got, want):
    got = host(got) if torch.is_tensor(got) else np.asarray(got)
    want = np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        u = {1: np.uint8, 4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
        bad = np.flatnonzero(got.reshape(-1).view(u) != want.reshape(-1).view(u))
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.size} of {got.size} elements differ, first at flat index {i} "
                             f"(shape {got.shape}): got {got.reshape(-1)[i]!r}, want {want.reshape(-1)[i]!r}")


def assert_pattern(what, t, pattern=PC.PATTERN):
    raw = host(t.contiguous().view(-1).view(torch.uint8))
    assert (raw == pattern).all(), f"{what}: {int((raw != pattern).sum())} bytes were written"


def make_cfg(geo, max_points, max_voxels, C):
    c = _L().PillarCfg()
    c.x_min, c.y_min, c.z_min = (float(v) for v in geo.pc_range[:3])
    c.vx, c.vy, c.vz = (float(v) for v in geo.voxel_size)
    c.gx, c.gy, c.max_points, c.max_voxels, c.n_channels = geo.gx, geo.gy, max_points, max_voxels, C
    return c


def c_offsets(offsets):
    return (ctypes.c_int * len(offsets))(*offsets)


def vox_outputs(B, cfg, cells=None):
    rows = B * cfg.max_voxels
    i32 = torch.int32
    return dict(coors=poisoned((rows, 4), i32), num_points=poisoned((rows,), i32), slots=poisoned((rows, cfg.max_points), i32),
                num_voxels=poisoned((B,), i32), cell_to_voxel=poisoned((B * cfg.gx * cfg.gy if cells is None else cells,), i32))


def call_voxelize(points, offsets, B, cfg, out, ws, ws_bytes):
    L = _L()
    return L.lib().liso_pillars_voxelize_f32(L.ptr(points), c_offsets(offsets), B, ctypes.byref(cfg), L.ptr(out["coors"]),
                                             L.ptr(out["num_points"]), L.ptr(out["slots"]), L.ptr(out["num_voxels"]),
                                             L.ptr(out["cell_to_voxel"]), L.ptr(ws), ws_bytes, L.stream_ptr())


def voxelize(pcls, cfg):
    """the entry point on poisoned outputs and a poisoned workspace of exactly the bytes it asks for -> (points, outputs)"""
    L = _L()
    B, offsets = len(pcls), PC.offsets_of(pcls)
    points = dev(np.concatenate(pcls))
    nbytes = L.lib().liso_pillars_voxelize_workspace_bytes(ctypes.byref(cfg), B, offsets[-1])
    assert nbytes > 0
    out, ws = vox_outputs(B, cfg), poisoned((nbytes,), torch.uint8)
    assert call_voxelize(points, offsets, B, cfg, out, ws, nbytes) == 0
    return points, out


# ---- 1. liso_pillars_voxelize_f32 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(VOX))
def test_voxelize_bit_for_bit(name):
    """num_voxels, coors, num_points, the kept point of every slot and cell_to_voxel equal the oracle's; every slot behind
    num_points[v], every row >= num_voxels[b] keeps the pattern; cells without a kept pillar (those of cap-dropped pillars too) hold 0"""
    c = VOX[name]()
    want = PC.expected_voxelize(c["pcls"], c["geo"], c["max_points"], c["max_voxels"])
    cfg = make_cfg(c["geo"], c["max_points"], c["max_voxels"], 4)
    with guarded() as gd:
        points, out = voxelize(c["pcls"], cfg)
        gd.check()
    for k in ("num_voxels", "coors", "num_points", "cell_to_voxel", "slots"):
        assert_bits(f"{name}: {k}", out[k], want[k])
    assert_bits(f"{name}: points (input)", points, np.concatenate(c["pcls"]))


def test_voxelize_refuses_more_than_4096_scan_blocks():
    """B = 4 at 1024 x 1024 is the limit (the `large` case above runs it); one more column of cells is refused, nothing written"""
    L = _L()
    geo = PC.Geo(1024, 1024, 0.125)
    cfg = make_cfg(geo, 20, 64, 4)
    assert L.lib().liso_pillars_voxelize_workspace_bytes(ctypes.byref(cfg), 4, 100) > 0
    cfg.gy = 1025
    assert L.lib().liso_pillars_voxelize_workspace_bytes(ctypes.byref(cfg), 4, 100) == 0
    pts = PC.lattice_points(np.random.default_rng(0), geo, [[5, 5]] * 100, 4)
    with guarded() as gd:
        points, out, ws = dev(pts), vox_outputs(4, cfg, cells=1024), poisoned((1 << 16,), torch.uint8)
        assert call_voxelize(points, [0, 25, 50, 75, 100], 4, cfg, out, ws, 1 << 16) == EINVAL
        gd.check()
    for k, t in list(out.items()) + [("workspace", ws)]:
        assert_pattern(k, t)


def test_voxelize_refusals_leave_the_outputs_untouched():
    L = _L()
    geo = PC.Geo(64, 64, 1.0)
    pts = PC.lattice_points(np.random.default_rng(1), geo, PC.random_cells(np.random.default_rng(2), geo, 300), 4)
    good = dict(n_channels=4, max_points=20, max_voxels=100, batch=2, offsets=[0, 100, 300])
    bad = [dict(n_channels=2), dict(n_channels=6), dict(max_points=0), dict(max_points=33), dict(batch=0), dict(batch=33),
           dict(max_voxels=0), dict(offsets=[0, 200, 100]), dict(offsets=[1, 100, 300]), dict(short=1)]
    with guarded() as gd:
        points = dev(pts)
        ref_cfg = make_cfg(geo, 20, 100, 4)
        nbytes = L.lib().liso_pillars_voxelize_workspace_bytes(ctypes.byref(ref_cfg), 2, 300)
        out, ws = vox_outputs(2, ref_cfg), poisoned((nbytes,), torch.uint8)
        for change in bad:
            k = dict(good, **change)
            cfg = make_cfg(geo, k["max_points"], k["max_voxels"], k["n_channels"])
            offsets = k["offsets"] + [300] * (k["batch"] + 1 - len(k["offsets"]))  # (batch 33: the ABI reads batch + 1 offsets)
            rc = call_voxelize(points, offsets, k["batch"], cfg, out, ws, nbytes - k.get("short", 0))
            assert rc == (EWORKSPACE if "short" in change else EINVAL), (change, rc)
            if "short" not in change and "offsets" not in change:
                assert L.lib().liso_pillars_voxelize_workspace_bytes(ctypes.byref(cfg), k["batch"], 300) == 0, change
        gd.check()
        for name, t in list(out.items()) + [("workspace", ws)]:
            assert_pattern(name, t)
        assert call_voxelize(points, good["offsets"], 2, ref_cfg, out, ws, nbytes) == 0  # the same buffers are accepted unchanged
        gd.check()
    assert int(out["num_voxels"].sum()) > 0


# ---- the stages behind the voxeliser, each on the device outputs of the one in front -------------------------------------------------------
def decorate(points, cfg, B, vox):
    L = _L()
    rows = B * cfg.max_voxels
    n_feat = max(points.shape[0], 1)
    pt_off, voxel_cell = poisoned((rows + 1,), torch.int32), poisoned((rows,), torch.int32)
    feat = poisoned((n_feat, 12), torch.float32)
    nbytes = L.lib().liso_pfn_decorate_workspace_bytes(B, cfg.max_voxels)
    ws = poisoned((nbytes,), torch.uint8)
    assert L.lib().liso_pfn_decorate_f32(L.ptr(points), ctypes.byref(cfg), B, L.ptr(vox["coors"]), L.ptr(vox["num_points"]),
                                         L.ptr(vox["slots"]), L.ptr(vox["num_voxels"]), L.ptr(pt_off), L.ptr(feat), L.ptr(voxel_cell),
                                         L.ptr(ws), nbytes, L.stream_ptr()) == 0
    return dict(pt_off=pt_off, feat=feat, voxel_cell=voxel_cell)


def bn_prepare(cfg, B, vox, dec, prm, training):
    """-> dict(bn_out, moments, running_mean, running_var): device tensors, the first two poisoned before the call"""
    L = _L()
    d = {k: dev(v) for k, v in prm.items()}
    bn_out, moments = poisoned((256,), torch.float32), poisoned((80,), torch.float64)
    partials = poisoned((L.lib().liso_pfn_partials_bytes(),), torch.uint8)
    assert L.lib().liso_pfn_bn_prepare_f32(L.ptr(dec["feat"]), L.ptr(dec["pt_off"]), ctypes.byref(cfg), B, L.ptr(vox["num_voxels"]),
                                           L.ptr(d["weight"]), L.ptr(d["gamma"]), L.ptr(d["beta"]), L.ptr(d["running_mean"]),
                                           L.ptr(d["running_var"]), PC.MOMENTUM, PC.EPS, int(training), L.ptr(bn_out), L.ptr(moments),
                                           L.ptr(partials), L.stream_ptr()) == 0
    return dict(bn_out=bn_out, moments=moments, running_mean=d["running_mean"], running_var=d["running_var"], weight=d["weight"],
                gamma=d["gamma"])


def prepare(pcls, geo, max_points, max_voxels, C):
    cfg = make_cfg(geo, max_points, max_voxels, C)
    points, vox = voxelize(pcls, cfg)
    return cfg, points, vox, decorate(points, cfg, len(pcls), vox)


# ---- 2. liso_pfn_decorate_f32 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [3, 4, 5])
@pytest.mark.parametrize("B,max_voxels", [(1, 1023), (1, 1024), (1, 1025), (2, 40000)])
def test_decorate_rows(B, max_voxels, C):
    """pt_off (the exclusive sum of the kept counts; 79 scan blocks at B = 2 x 40 000 rows) and voxel_cell bit for bit; of a row: the
    constant 1, the zero padding, the aliased centre columns and the extras bit for bit, every float column within
    16 * 2^-24 * max|coordinate| of the fp64 row.
    Derivation: a centre term p - (idx * v + off) carries at most three fp32 roundings (product, sum, difference), each at most
    2^-24 of a magnitude <= max|coordinate| (+ half a cell); a cluster term p - mean: the 5-level butterfly sum of <= 32 values has
    a relative error <= 5 * 2^-24 of sum|p| <= n * max|coordinate|, the division by n brings that to 5 * 2^-24 * max|coordinate| and
    adds one rounding, the difference one more: 7 roundings.  16 covers both with room for the half cell."""
    geo = PC.Geo(64, 64, 1.0)
    pcls = PC.pfn_cloud(10 * B + C, geo, C, 3000, B)
    e = PC.expected_decorate(pcls, geo, 20, max_voxels)
    want_vox = PC.expected_voxelize(pcls, geo, 20, max_voxels)
    with guarded() as gd:
        cfg, points, vox, dec = prepare(pcls, geo, 20, max_voxels, C)
        gd.check()
    for k in ("num_voxels", "coors", "num_points", "slots"):
        assert_bits(k, vox[k], want_vox[k])
    assert_bits("pt_off", dec["pt_off"], e["pt_off"])
    assert_bits("voxel_cell", dec["voxel_cell"], e["voxel_cell"])
    N, F = int(e["pt_off"][-1]), C + 6
    feat, cat = host(dec["feat"]), np.concatenate(pcls)
    assert_pattern("feat rows behind the last kept point", dec["feat"][N:])
    rows = feat[:N]
    assert_bits("column F", rows[:, F], np.ones(N, np.float32))
    assert_bits("padding columns", rows[:, F + 1:], np.zeros((N, 11 - F), np.float32))
    assert_bits("aliased centre columns", rows[:, C + 3:C + 6], rows[:, 0:3])
    assert_bits("extras", rows[:, 3:C], cat[e["point"], 3:C])
    coord = float(np.abs(cat[e["point"], :3]).max())
    err = np.abs(rows[:, :F].astype(np.float64) - e["rows"])
    assert err.max() <= 16 * U * coord, (err.max() / (U * coord), np.unravel_index(err.argmax(), err.shape))


# ---- 3. liso_pfn_bn_prepare_f32 --------------------------------------------------------------------------------------------------------
def bn_case(which, C):
    geo = PC.Geo(64, 64, 1.0)
    if which == "one_point":
        return geo, [PC.lattice_points(np.random.default_rng(5), geo, [[20, 30]], C)], 40
    if which == "empty":  # no pillar at all: every point out of range, one sample without points
        far = PC.lattice_points(np.random.default_rng(6), geo, [[70, 3], [-4, 9], [64, 64]], C)
        return geo, [far, np.zeros((0, C), np.float32)], 40
    return geo, PC.pfn_cloud(50 + C, geo, C, 2500, 2, const5=(which == "const5")), 3000


@pytest.mark.parametrize("training", [1, 0])
@pytest.mark.parametrize("which,C", [("cloud", 3), ("cloud", 4), ("cloud", 5), ("const5", 5), ("one_point", 4), ("empty", 4)])
def test_bn_prepare(which, C, training):
    """Against fp64 from the device's own feature rows, so only this stage is judged.
    moments: the products of two fp32 numbers are exact in fp64, the kernel and the reference differ in the order of the sum alone:
    |err| <= n * 2^-53 * sum|products|, n <= 10^5 rows -> 1e-11 * sum|products| (rtol 1e-11 of the sum of magnitudes: several
    moments, such as sum(p - mean), cancel to rounding noise and have no digits of their own).
    bn_out: fp64 arithmetic rounded once to fp32 (training) / a few fp32 operations (eval): 4 * 2^-24 * |ref|, for shift plus the same
    factor of its subtrahend |mean * gamma * invstd|.  Running stats: torch.nn.functional.batch_norm in fp64 over the padded rows
    (M = pillars * max_points, unbiased variance, momentum 0.01), 4 fp32 ulps of the result.  (`one_point` found the blend done in
    fp32: where the batch mean opposes the running mean the two terms cancel, 7.4 ulps; the kernel now blends in fp64.)"""
    geo, pcls, max_voxels = bn_case(which, C)
    prm = PC.pfn_params(C, C)
    B = len(pcls)
    with guarded() as gd:
        cfg, points, vox, dec = prepare(pcls, geo, 20, max_voxels, C)
        bn = bn_prepare(cfg, B, vox, dec, prm, training)
        gd.check()
    P, N = int(host(vox["num_voxels"]).sum()), int(host(dec["pt_off"])[-1])
    assert (P, N) == {"one_point": (1, 1), "empty": (0, 0)}.get(which, (P, N)) and (which in ("one_point", "empty") or P > 1000)
    feat = host(dec["feat"])[:N]
    if which == "const5":
        assert (feat[:, 4] == np.float32(0.375)).all()
    ref = PC.bn_reference(feat, C, P, 20, prm, training)
    got = host(bn["bn_out"]).astype(np.float64).reshape(4, 64)
    assert np.isfinite(got).all()
    for i, k in enumerate(("scale", "shift", "mean", "invstd")):
        lim = 4 * U * (np.abs(ref[k]) + (ref["shift_term"] if k == "shift" else 0.0))
        err = np.abs(got[i] - ref[k])
        assert (err <= lim).all(), (k, float((err / np.maximum(lim, 1e-300)).max()) * 4, "x 2^-24 relative")
    rm, rv = host(bn["running_mean"]), host(bn["running_var"])
    if not training:
        assert_bits("running_mean", rm, prm["running_mean"])
        assert_bits("running_var", rv, prm["running_var"])
        assert_pattern("moments", bn["moments"])
        return
    NP = (C + 7) * (C + 8) // 2
    mom = host(bn["moments"])
    tot, mag = PC.moments_reference(feat, C)
    assert (np.abs(mom[:NP] - tot) <= 1e-11 * mag).all(), float((np.abs(mom[:NP] - tot) / np.maximum(mag, 1e-300)).max())
    assert_bits("moments behind the triangle", mom[NP:], np.zeros(80 - NP))
    if which == "empty":
        assert (got[2] == 0).all() and (mom == 0).all()
        assert_bits("running_mean", rm, prm["running_mean"])
        assert_bits("running_var", rv, prm["running_var"])
        return
    for name, g, r in (("running_mean", rm, ref["running_mean"]), ("running_var", rv, ref["running_var"])):
        ulps = np.abs(g.astype(np.float64) - r) / np.spacing(np.abs(r).astype(np.float32)).astype(np.float64)
        assert ulps.max() <= 4, (name, float(ulps.max()))
        assert not np.array_equal(g, prm[name])


# ---- 4. liso_pfn_forward_scatter -------------------------------------------------------------------------------------------------------
FWD_CASES = {"rows1023": (PC.Geo(64, 64, 1.0), 1, 1023, 4),     # rows no multiple of 4; the cap drops pillars
             "grid50x30": (PC.Geo(50, 30, 1.0), 3, 501, 3),     # non-square; 4500 cells, no multiple of 256; 1503 rows
             "stride": (PC.Geo(64, 64, 1.0), 3, 40000, 5)}      # sample 2's rows start at 80 000: the second trip of the stride loop
ELEM = {"fp32": (torch.float32, np.float32), "fp16": (torch.float16, np.float16), "bf16": (torch.bfloat16, None)}


def crafted_params(C):
    """every pre-activation negative, shift > 0: x = (w_2 + w_{C+5}) * z with z in [1, 3), scale in [-2, -1], shift in (0.05, 0.5]"""
    r = np.random.default_rng(77)
    w = np.zeros((64, C + 6), np.float32)
    w[:, 2], w[:, C + 5] = r.uniform(0.5, 1.0, 64), r.uniform(0.5, 1.0, 64)
    bn = np.concatenate([r.uniform(-2, -1, 64), r.uniform(0.05, 0.5, 64), np.zeros(64), np.ones(64)]).astype(np.float32)
    return w, bn


@pytest.mark.parametrize("elem", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("params", ["random", "crafted"])
@pytest.mark.parametrize("case", sorted(FWD_CASES))
def test_forward_scatter(case, params, elem):
    """Against fp64 max over the pillar's rows of relu(scale * (w . f) + shift) from the device's feat / weight / bn_out, the padding
    candidate relu(shift) included when num < max_points.
    Bound per element: the kernel's x is an F <= 11 term fp32 FMA chain, |x - w . f| <= 11 * 2^-24 * sum_k |w_k f_k| (to first order),
    one more FMA gives scale * x + shift with |err| <= |scale| * 11 * 2^-24 * sum|w_k f_k| + 2^-24 * |scale * x + shift|
    <= 12 * 2^-24 * (|scale| * sum|w_k f_k| + |shift|); 16 leaves the second-order terms room.  relu and max do not enlarge it.
    `crafted`: every pre-activation negative with shift > 0 -- a full pillar (no padding row) must give 0, any other pillar shift.
    `random`: random weights, BatchNorm of the batch with beta of both signs (padding wins where shift > 0, never where shift < 0).
    16-bit canvases: half an ulp of the format at the fp64 value on top of that bound."""
    L = _L()
    geo, B, max_voxels, C = FWD_CASES[case]
    pcls = PC.pfn_cloud(len(case) + C, geo, C, 2500, B, z_lo=1.0 if params == "crafted" else None)
    tdtype, ndtype = ELEM[elem]
    with guarded() as gd:
        cfg, points, vox, dec = prepare(pcls, geo, 20, max_voxels, C)
        if params == "crafted":
            w, bn = crafted_params(C)
            weight, bn_out = dev(w), dev(bn)
        else:
            bnp = bn_prepare(cfg, B, vox, dec, PC.pfn_params(C, C), 1)
            weight, bn_out = bnp["weight"], bnp["bn_out"]
        canvas = poisoned((B, geo.gx, geo.gy, 64), tdtype, NAN_PATTERN)
        occupancy = poisoned((B, 1, geo.gx, geo.gy), torch.float32, NAN_PATTERN)
        assert L.lib().liso_pfn_forward_scatter(L.ptr(dec["feat"]), L.ptr(dec["pt_off"]), L.ptr(dec["voxel_cell"]), ctypes.byref(cfg), B,
                                                L.ptr(vox["cell_to_voxel"]), L.ptr(weight), L.ptr(bn_out), L.ptr(canvas),
                                                L.elem_code(tdtype), L.ptr(occupancy), L.stream_ptr()) == 0
        gd.check()
    pt_off, voxel_cell, c2v = host(dec["pt_off"]), host(dec["voxel_cell"]), host(vox["cell_to_voxel"])
    N = int(pt_off[-1])
    idx, val, bnd = PC.forward_reference(host(dec["feat"])[:N], pt_off, 20, C, host(weight), host(bn_out))
    cells = voxel_cell[idx]
    assert (cells >= 0).all() and len(idx) == (voxel_cell >= 0).sum() == (c2v > 0).sum() and np.array_equal(c2v[cells] - 1, idx)
    nv = host(vox["num_voxels"])
    assert (nv > 0).all() and (case != "stride" or idx.max() >= 80000) and (case != "rows1023" or nv[0] == 1023)
    assert_bits("occupancy", occupancy.view(-1), (c2v > 0).astype(np.float32))
    flat = canvas.view(-1, 64)
    empty = torch.from_numpy(c2v == 0).to(DEV)
    bits = flat[empty].contiguous().view(torch.uint8)
    assert int(bits.count_nonzero()) == 0, "a cell without a kept pillar is not +0.0 in every channel"
    got = host(flat[torch.from_numpy(cells).to(DEV).long()].double())
    assert np.isfinite(got).all()
    kept = np.diff(pt_off.astype(np.int64))[idx]
    if params == "crafted":
        full = kept == 20
        assert full.any() and (~full).any() and (val[full] == 0).all() and (val[~full] > 0).all()
        assert (got[full] == 0).all(), "a full pillar has no padding row: every pre-activation is negative, the result is 0"
    else:
        shift = host(bn_out).astype(np.float64)[64:128]
        assert (shift > 0).any() and (shift < 0).any() and (kept < 20).any() and (kept == 20).any()
        assert (val[kept < 20][:, shift > 0] >= shift[shift > 0]).all() and (val > np.maximum(shift, 0)).any()
    err = np.abs(got - val)
    if elem == "fp32":
        assert (err <= bnd).all(), float((err / bnd).max())
        return
    mant, min_exp = (10, -14) if elem == "fp16" else (7, -126)
    lim = 0.5 * PC.ulp_of(np.abs(val) + bnd, mant, min_exp) + bnd
    assert (err <= lim).all(), float((err / lim).max())
    if elem == "fp16":
        assert_fp16_rounded(torch.from_numpy(got), torch.from_numpy(val), float(bnd.max() / np.abs(val).max()))


# ---- 5. liso_pfn_backward ----------------------------------------------------------------------------------------------------------------
def backward(cfg, B, vox, dec, bn, training, grad_canvas):
    L = _L()
    F = cfg.n_channels + 6
    gw, gg, gb = poisoned((64, F), torch.float32, NAN_PATTERN), poisoned((64,), torch.float32, NAN_PATTERN), poisoned((64,), torch.float32, NAN_PATTERN)
    partials = poisoned((L.lib().liso_pfn_partials_bytes(),), torch.uint8)
    assert L.lib().liso_pfn_backward(L.ptr(dec["feat"]), L.ptr(dec["pt_off"]), L.ptr(dec["voxel_cell"]), ctypes.byref(cfg), B,
                                     L.ptr(vox["num_voxels"]), L.ptr(bn["weight"]), L.ptr(bn["gamma"]), L.ptr(bn["bn_out"]),
                                     L.ptr(bn["moments"]), int(training), L.ptr(grad_canvas), L.elem_code(grad_canvas.dtype), L.ptr(gw),
                                     L.ptr(gg), L.ptr(gb), L.ptr(partials), L.stream_ptr()) == 0
    return dict(weight=gw, gamma=gg, beta=gb)


@pytest.mark.parametrize("B,C,training,gdtype", PC.BACKWARD_CASES)
def test_backward_against_fp64_autograd(B, C, training, gdtype):
    """grad_weight / grad_gamma / grad_beta against fp64 autograd through oracle.pillars.pillar_forward from the same points, in
    training mode and in eval mode (non-trivial running stats), the upstream gradient in fp32 / bf16 / fp16 (rounded first; the
    reference gets the rounded values).  The upstream gradient is zero at every (pillar, channel) whose max or ReLU is nearly tied in
    the reference (pillar_stage_cases.near_tie_keep; at most 1 % of the entries).
    Tolerance, per tensor: the kernel sums up to 1024 fp32 block partials in another order than torch, so no closed form: with
    e32 = max|fp32 oracle - fp64 oracle| on the CPU, max|kernel - fp64 oracle| <= 8 * e32, not below 2^-20 * max|fp64 oracle|.
    Measured on an MI355X, e32 / kernel error of grad_weight (w), grad_gamma (g), grad_beta (b); the largest kernel error is
    2.2 x e32 (g, B3 C4 eval bf16), nowhere near 8 x:
      B1 C3 train fp32: w 2.2e-03/3.0e-04  g 4.5e-05/3.2e-05  b 1.6e-05/6.9e-06
      B1 C3 eval  fp32: w 1.9e-03/3.0e-04  g 1.5e-04/1.4e-04  b 1.6e-05/8.1e-06
      B1 C4 train fp32: w 2.2e-03/2.8e-04  g 4.3e-05/3.8e-05  b 1.1e-05/8.9e-06
      B1 C4 eval  fp32: w 1.9e-02/9.9e-04  g 4.0e-04/3.4e-04  b 1.8e-05/6.6e-06
      B1 C5 train fp32: w 3.7e-03/6.6e-04  g 4.5e-05/4.4e-05  b 1.5e-05/8.8e-06
      B1 C5 eval  fp32: w 2.1e-02/1.5e-03  g 6.6e-04/5.7e-04  b 1.4e-05/8.8e-06
      B3 C3 train fp32: w 3.0e-02/2.2e-03  g 1.6e-04/1.3e-04  b 2.2e-05/8.0e-06
      B3 C3 eval  fp32: w 2.7e-03/2.4e-04  g 1.2e-04/2.1e-04  b 1.7e-05/8.9e-06
      B3 C4 train fp32: w 5.1e-03/7.1e-04  g 4.6e-05/6.4e-05  b 2.0e-05/6.7e-06
      B3 C4 eval  fp32: w 3.3e-02/1.8e-03  g 3.9e-04/4.3e-04  b 2.0e-05/9.6e-06
      B3 C5 train fp32: w 6.9e-03/7.2e-04  g 4.6e-05/5.1e-05  b 1.7e-05/8.3e-06
      B3 C5 eval  fp32: w 2.5e-02/1.7e-03  g 7.5e-04/7.5e-04  b 2.4e-05/8.1e-06
      B3 C4 train bf16: w 6.4e-03/6.8e-04  g 4.6e-05/6.1e-05  b 7.6e-06/3.8e-06
      B3 C4 train fp16: w 3.2e-03/4.8e-04  g 6.2e-05/5.7e-05  b 1.9e-05/3.8e-06
      B3 C4 eval  bf16: w 1.9e-02/2.0e-03  g 4.1e-04/9.2e-04  b 5.7e-06/4.8e-06
      B3 C4 eval  fp16: w 4.1e-02/1.6e-03  g 3.2e-04/6.3e-04  b 1.2e-05/4.5e-06
      B1 C5 train bf16: w 3.8e-03/1.3e-03  g 5.7e-05/7.2e-05  b 4.8e-06/3.8e-06
      B1 C3 eval  fp16: w 2.4e-03/2.1e-04  g 1.5e-04/1.8e-04  b 1.0e-05/3.1e-06"""
    c = PC.backward_case(B, C, training, gdtype)
    s = c["stats"]
    assert s["masked"] <= 0.01 * s["entries"], s
    geo, prm = c["geo"], c["prm"]
    with guarded() as gd:
        cfg, points, vox, dec = prepare(c["pcls"], geo, 20, 40000, C)
        bn = bn_prepare(cfg, B, vox, dec, prm, training)
        got = backward(cfg, B, vox, dec, bn, training, dev(c["grad"]).to(PC.TORCH_DTYPE[gdtype]).contiguous())
        gd.check()
    ref = PC.oracle_gradients(c["pcls"], geo, 20, 40000, prm, training, c["grad"], torch.float64)
    r32 = PC.oracle_gradients(c["pcls"], geo, 20, 40000, prm, training, c["grad"], torch.float32)
    report, ok = [], True
    for k in ("weight", "gamma", "beta"):
        g = host(got[k]).astype(np.float64)
        assert np.isfinite(g).all(), k
        e32, err, top = np.abs(r32[k] - ref[k]).max(), np.abs(g - ref[k]).max(), np.abs(ref[k]).max()
        lim = max(8 * e32, 2.0 ** -20 * top)
        ok &= bool(err <= lim)
        report.append(f"grad_{k}: e32 {e32:.3e} kernel {err:.3e} limit {lim:.3e} max|ref| {top:.3e}")
    msg = f"B={B} C={C} training={training} {gdtype}: " + "; ".join(report)
    print(msg)
    assert ok, msg


@pytest.mark.parametrize("training", [1, 0])
def test_backward_without_any_pillar(training):
    geo, pcls, max_voxels = bn_case("empty", 4)
    prm = PC.pfn_params(4, 4)
    with guarded() as gd:
        cfg, points, vox, dec = prepare(pcls, geo, 20, max_voxels, 4)
        bn = bn_prepare(cfg, 2, vox, dec, prm, training)
        grad = dev(np.random.default_rng(3).normal(size=(2, 64, 64, 64)).astype(np.float32))
        got = backward(cfg, 2, vox, dec, bn, training, grad)
        gd.check()
    assert int(host(vox["num_voxels"]).sum()) == 0
    for k, t in got.items():
        assert_bits(f"grad_{k}", t, np.zeros(tuple(t.shape), np.float32))
