"""GPU: the grouped, two-gradient BatchNorm(+ReLU) backward (include/liso_bn.h: liso_bn_relu_bwd_multi) against today's composition --
liso_bn_relu_bwd_strided per group and per gradient, then `a + b` of the results in torch.  Every (group, gradient) pair of the grouped
call keeps the single call's geometry and summation order, and the sums of two gradients are formed as torch's add forms them, so every
comparison here is BITWISE: no tolerance anywhere.  Also: the merged-statistics destination of liso_conv_bn_finalize_merged."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 64  # elements of guard band on either side of every output (a multiple of 16 bytes in every dtype)
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}


def _bits(t):
    return t.detach().contiguous().reshape(-1).view(torch.uint8).cpu()


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


class Guarded:
    """a buffer of `n` elements between two guard bands filled with a pattern no kernel writes"""

    def __init__(self, n, dtype, dev):
        self.full = torch.empty(n + 2 * GUARD, dtype=dtype, device=dev)
        self.full.view(torch.uint8).fill_(0xA5)
        self.inner = self.full[GUARD:GUARD + n]
        self.inner.view(torch.uint8).fill_(0x5A)  # (not zero: every output must be WRITTEN)

    def intact(self):
        b = self.full.view(torch.uint8)
        e = self.full.element_size() * GUARD
        return bool((b[:e] == 0xA5).all()) and bool((b[-e:] == 0xA5).all())


def _group_stats(x, dev):
    """x [m, C] -> (gamma, stats = scale | shift | mean | invstd)"""
    C = x.shape[1]
    xf = x.float()
    mean = xf.mean(dim=0)
    invstd = (xf.var(dim=0, unbiased=False) + 1e-3).rsqrt()
    gamma = torch.rand(C, device=dev) + 0.5
    beta = torch.randn(C, device=dev) * 0.1
    return gamma, torch.cat([gamma * invstd, beta - mean * gamma * invstd, mean, invstd]).contiguous()


def _wide(m, ct, lead, trail, dtype, dev, fill=None):
    """[m, lead + ct + trail] tensor and its [m, ct] channel slice behind `lead` channels"""
    w = torch.randn(m, lead + ct + trail, device=dev).to(dtype) if fill is None else torch.full((m, lead + ct + trail), fill, device=dev).to(dtype)
    return w, w[:, lead:lead + ct]


def _reference(lib, L, x, gs, cs, gammas, stats, training, relu):
    """today's composition: one strided call per (group, gradient), the two gradients' results added in torch"""
    m, dev, code = x.shape[0], x.device, L.elem_code(x.dtype)
    dx = torch.empty(m, sum(cs), dtype=x.dtype, device=dev)
    grads, off = [], 0
    for C, gamma, st in zip(cs, gammas, stats):
        per = []
        for g in gs:
            nbytes = lib.liso_bn_workspace_bytes(C)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            d = torch.empty(m, C, dtype=x.dtype, device=dev)
            gg, gb = torch.empty(C, device=dev), torch.empty(C, device=dev)
            xs_, gs_ = x[:, off:off + C], g[:, off:off + C]
            L.check(lib.liso_bn_relu_bwd_strided(L.ptr(gs_), g.stride(0), L.ptr(xs_), x.stride(0), code, m, C, L.ptr(gamma), L.ptr(st), training,
                                                 relu, L.ptr(d), C, L.ptr(gg), L.ptr(gb), L.ptr(ws), nbytes, L.stream_ptr()), "bn_relu_bwd_strided")
            per.append((d, gg, gb))
        if len(per) == 2:
            per = [(per[0][0] + per[1][0], per[0][1] + per[1][1], per[0][2] + per[1][2])]
        dx[:, off:off + C] = per[0][0]
        grads.append((per[0][1], per[0][2]))
        off += C
    return dx, grads


def _multi(lib, L, x, gs, cs, gammas, stats, training, relu, dx_view, jobs=()):
    """the grouped call; every output sits between guard bands -> ([(dgamma, dbeta)], ok flag of the guards)"""
    m, dev, code = x.shape[0], x.device, L.elem_code(x.dtype)
    tab = (L.BnGroup * len(cs))()
    outs, off = [], 0
    for k, (C, gamma, st) in enumerate(zip(cs, gammas, stats)):
        gg, gb = Guarded(C, torch.float32, dev), Guarded(C, torch.float32, dev)
        outs.append((gg, gb))
        tab[k].c_off, tab[k].c = off, C
        tab[k].gamma, tab[k].stats, tab[k].grad_gamma, tab[k].grad_beta = gamma.data_ptr(), st.data_ptr(), gg.inner.data_ptr(), gb.inner.data_ptr()
        off += C
    nbytes = lib.liso_bn_multi_workspace_bytes(tab, len(cs), len(gs))
    assert nbytes > 0
    ws = Guarded(nbytes, torch.uint8, dev)
    gb_ = gs[1] if len(gs) == 2 else None
    L.check(lib.liso_bn_relu_bwd_multi(L.ptr(gs[0]), gs[0].stride(0), L.ptr(gb_) if gb_ is not None else None, gb_.stride(0) if gb_ is not None else 0,
                                       L.ptr(x), x.stride(0), code, m, tab, len(cs), training, relu, L.ptr(dx_view), dx_view.stride(0),
                                       L.ptr(ws.inner), nbytes, jobs[0].ride() if len(jobs) > 0 else None,
                                       jobs[1].ride() if len(jobs) > 1 else None, L.stream_ptr()), "bn_relu_bwd_multi")
    torch.cuda.synchronize()
    ok = ws.intact() and all(a.intact() and b.intact() for a, b in outs)
    return [(a.inner.clone(), b.inner.clone()) for a, b in outs], ok


def _case(lib, L, dtype, sliced, m, cs, n_grads, relu, training, dev, jobs=()):
    ct, vec = sum(cs), (4 if dtype == torch.float32 else 8)
    tag = (str(dtype), sliced, m, cs, n_grads, relu, training)
    # (sliced: x, dy_a, dy_b and dx are channel slices of four wider tensors with four different row strides)
    lead = [vec, 2 * vec, 0, 3 * vec] if sliced else [0, 0, 0, 0]
    trail = [2 * vec, vec, 3 * vec, 0] if sliced else [0, 0, 0, 0]
    _, x = _wide(m, ct, lead[0], trail[0], dtype, dev)
    x.mul_(0.5).add_(0.1)
    gs = [_wide(m, ct, lead[1 + n], trail[1 + n], dtype, dev)[1] for n in range(n_grads)]
    gammas, stats, off = [], [], 0
    for C in cs:
        gamma, st = _group_stats(x[:, off:off + C], dev)
        gammas.append(gamma)
        stats.append(st)
        off += C
    width = lead[3] + ct + trail[3]
    dxg = Guarded(m * width, dtype, dev)
    before = dxg.inner.clone().view(m, width)
    dx_view = dxg.inner.view(m, width)[:, lead[3]:lead[3] + ct]
    ref_dx, ref_grads = _reference(lib, L, x, gs, cs, gammas, stats, training, relu)
    got_grads, ok = _multi(lib, L, x, gs, cs, gammas, stats, training, relu, dx_view, jobs)
    assert ok and dxg.intact(), ("guard band overwritten", tag)
    after = dxg.inner.view(m, width)
    assert _same(after[:, :lead[3]], before[:, :lead[3]]) and _same(after[:, lead[3] + ct:], before[:, lead[3] + ct:]), ("dx outside its channels", tag)
    assert _same(ref_dx, dx_view.contiguous()), ("dx", tag)
    for k, ((rg, rb), (gg, gb)) in enumerate(zip(ref_grads, got_grads)):
        assert _same(rg, gg), ("grad_gamma", k, tag)
        assert _same(rb, gb), ("grad_beta", k, tag)


@pytest.mark.parametrize("sliced", [False, True], ids=["dense", "sliced"])
@pytest.mark.parametrize("dt", list(DTYPES))
def test_grouped_call_equals_the_per_group_per_gradient_calls_bitwise(dt, sliced):
    """m = 1, 127, 129, 300 (a single short block, one row under and over kRowsPerBlock = 128, a last block with a remainder) x one and
    three small groups x one and two gradients x ReLU on / off x training 1 / 0; four 64-channel and three 128-channel groups at
    m = 129"""
    from liso_amd import _lib as L

    lib, dev, dtype = L.lib(), torch.device("cuda"), DTYPES[dt]
    small = [(4,), (4, 12, 8)] if dtype == torch.float32 else [(8,), (8, 16, 24)]
    torch.manual_seed(11)
    for m in (1, 127, 129, 300):
        for cs in small + ([(64, 64, 64, 64), (128, 128, 128)] if m == 129 else []):
            for n_grads in (1, 2):
                for relu in (1, 0):
                    for training in (1, 0):
                        _case(lib, L, dtype, sliced, m, cs, n_grads, relu, training, dev)


def test_more_than_one_row_block_and_segmented_finalize():
    """m = 128 * 64 + 5 rows: 64 row blocks of 129 rows -- the 32-channel finalize segments (nblk >= 64) of a 64- and a 128-channel
    group, the chunked partial-sum merge, and a short last block"""
    from liso_amd import _lib as L

    lib, dev = L.lib(), torch.device("cuda")
    torch.manual_seed(12)
    for dtype in (torch.bfloat16, torch.float32):
        _case(lib, L, dtype, True, 128 * 64 + 5, (64, 128), 2, 1, 1, dev)


def test_riding_weight_gradient_reductions_equal_the_separate_reduction_bitwise():
    """two deferred weight gradients (one with more than 16 splits, one with at most 16: both instantiations of the reduction) ride in
    the grouped call's finalize launch: dw / dbias equal liso_conv_wgrad's, and the BatchNorm results equal the composition's"""
    from liso_amd import _lib as L
    from liso_amd.utils import mfma_conv as MC

    lib, dev = L.lib(), torch.device("cuda")
    torch.manual_seed(13)
    picked = {}
    for B in (2, 4):
        for ci, co, hw, bias in ((64, 64, 64, False), (256, 256, 32, True), (64, 64, 16, True), (128, 128, 32, False), (64, 64, 256, False)):
            spec = MC.ConvSpec(3, 3, stride=1, padding=1)
            x = (torch.randn(B, hw, hw, ci, device=dev) * 0.5 + 0.1).to(torch.bfloat16).permute(0, 3, 1, 2)
            dy = torch.randn(B, hw, hw, co, device=dev).to(torch.bfloat16).permute(0, 3, 1, 2)
            dw0, db0 = MC.conv_wgrad(x, dy, (co, ci, 3, 3), spec, want_bias=bias)
            dw1, db1, job = MC.conv_wgrad(x, dy, (co, ci, 3, 3), spec, want_bias=bias, defer_reduce=True)
            assert job is not None
            if (job.job.splits > 16) not in picked:
                picked[job.job.splits > 16] = (job, dw0, db0, dw1, db1)
            else:
                job.flush()
            if len(picked) == 2:
                break
        if len(picked) == 2:
            break
    assert set(picked) == {False, True}, "the layers must cover the > 16 and the <= 16 splits reduction"
    jobs = [picked[True][0], picked[False][0]]
    _case(lib, L, torch.bfloat16, False, 300, (8, 16, 24), 2, 1, 1, dev, jobs=jobs)
    torch.cuda.synchronize()
    assert all(j.done for j in jobs)
    for _, dw0, db0, dw1, db1 in picked.values():
        assert _same(dw0, dw1)
        assert (db0 is None and db1 is None) or _same(db0, db1)


def test_grouped_entry_point_refuses_what_it_cannot_run():
    from liso_amd import _lib as L

    lib = L.lib()
    x = torch.zeros(16, 64, device="cuda", dtype=torch.bfloat16)
    f = torch.zeros(4 * 64, device="cuda")
    tab = (L.BnGroup * 1)()
    tab[0].c_off, tab[0].c = 0, 64
    tab[0].gamma = tab[0].stats = tab[0].grad_gamma = tab[0].grad_beta = f.data_ptr()
    nbytes = lib.liso_bn_multi_workspace_bytes(tab, 1, 2)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")

    def call(n_groups=1, ws_bytes=nbytes, xs=64, job=None):
        return lib.liso_bn_relu_bwd_multi(L.ptr(x), 64, L.ptr(x), 64, L.ptr(x), xs, 1, 16, tab, n_groups, 1, 1, L.ptr(x), 64, L.ptr(ws), ws_bytes,
                                          job, None, L.stream_ptr())

    assert call(n_groups=0) != 0 and call(n_groups=5) != 0
    assert call(ws_bytes=nbytes - 1) != 0
    assert call(xs=56) != 0  # (the group's channels do not fit a row of x)
    bad = L.WgradReduceJob()  # all zero: no slab, no dw
    assert call(job=ctypes.byref(bad)) != 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("cs,lead", [((8, 8, 8), 0), ((16, 16, 16, 16), 0), ((8, 24), 16)], ids=["3x8", "4x16", "offset"])
def test_merged_statistics_destination_equals_the_concatenation_bitwise(cs, lead):
    """liso_conv_bn_finalize_merged writes each group's own [4 C] statistics as liso_conv_bn_finalize does AND its four vectors into a
    merged scale | shift | mean | invstd buffer over all groups at the group's channel offset: that buffer == torch.cat of the groups'
    slices, kind by kind (`lead`: channels of the merged buffer in front of the first group, left untouched)"""
    from liso_amd import _lib as L

    lib, dev = L.lib(), torch.device("cuda")
    torch.manual_seed(14)
    rows, ct, n = 70, sum(cs), 5000
    cop = (ct + 63) // 64 * 64
    partial = torch.randn(rows, 2, cop, device=dev)
    partial[:, 1].abs_().mul_(40.0)  # (sums of squares: keep the variances positive)
    total = lead + ct
    merged, mgam = Guarded(4 * total, torch.float32, dev), Guarded(total, torch.float32, dev)
    gammas = []
    own, off = [], 0
    for C in cs:
        gamma, beta = torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev)
        ref = torch.empty(4 * C, device=dev)
        st = Guarded(4 * C, torch.float32, dev)
        part = ctypes.c_void_p(partial.data_ptr() + 4 * off)
        L.check(lib.liso_conv_bn_finalize(part, rows, C, cop, n, None, L.ptr(gamma), L.ptr(beta), None, None, 0.1, 1e-3, L.ptr(ref), L.stream_ptr()),
                "conv_bn_finalize")
        L.check(lib.liso_conv_bn_finalize_merged(part, rows, C, cop, n, None, L.ptr(gamma), L.ptr(beta), None, None, 0.1, 1e-3, L.ptr(st.inner),
                                                 L.ptr(merged.inner), L.ptr(mgam.inner), total, lead + off, L.stream_ptr()),
                "conv_bn_finalize_merged")
        gammas.append(gamma)
        torch.cuda.synchronize()
        assert st.intact() and _same(ref, st.inner.clone())
        own.append(ref)
        off += C
    assert merged.intact() and mgam.intact()
    assert _same(torch.cat(gammas), mgam.inner[lead:].clone())
    got = merged.inner.view(4, total)
    want = torch.stack([torch.cat([s[k * C:(k + 1) * C] for s, C in zip(own, cs)]) for k in range(4)])
    assert _same(want, got[:, lead:].contiguous())
    assert bool((got[:, :lead].contiguous().view(torch.uint8) == 0x5A).all())
