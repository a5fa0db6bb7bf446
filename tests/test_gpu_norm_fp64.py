"""GPU: the roots of the normalisation kernels' bitwise test chain -- liso_bn_relu_fwd, liso_in_relu_fwd, liso_bn_relu_bwd,
liso_in_relu_bwd_sum (liso_amd/csrc/bn.hip, chain_bodies.h), liso_conv_bn_finalize, liso_conv_in_finalize and
liso_residual_affine_relu_f32 (conv_mfma.hip) -- against the fp64 references of tests/norm_cases.py, at the geometries where each
path differs, within bounds derived there from the kernels' summation structure (never from their output; proved meaningful on the
CPU by tests/test_norm_cases.py).  Every output is pre-filled with a pattern between guard bands, must be written in full, and a
second call must give the same bits.  Each test prints its largest error as a fraction of its bound (`NORM_RATIO ...`, pytest -s)."""
import pytest
import torch

from tests import norm_cases as NC
from tests.fp16_checks import require_fp16
from tests.test_gpu_bn_multi import Guarded, _same

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _L(dt="fp32"):
    if dt == "fp16":
        return require_fp16()
    from liso_amd import _lib as L

    return L


def _id(case):
    return "-".join(str(v) for v in case)


def _written(g):
    """no element of the output still holds the fill pattern"""
    b = g.inner.view(torch.uint8).view(-1, g.inner.element_size())
    return not bool((b == 0x5A).all(dim=1).any())


def _filled(values, dev=DEV):
    """an in/out vector between guard bands"""
    g = Guarded(values.numel(), values.dtype, dev)
    g.inner.copy_(values.reshape(-1))
    return g


def _report(path, dt, case, ratio):
    print(f"NORM_RATIO {path} {dt} {_id(case)} {ratio:.4f}")


def _stats_dict(stats, c, rm=None, rv=None):
    s = stats.view(4, c)
    d = dict(scale=s[0], shift=s[1], mean=s[2], invstd=s[3])
    if rm is not None:
        d["running_mean"], d["running_var"] = rm, rv
    return d


def _check_apply(x, y, stats32, relu, dt, tag):
    """y against round_T(relu?(x * scale + shift)) in fp64 from the fp32 statistics the call returned"""
    z = NC.apply_reference(x, stats32, relu)
    ok, outside = NC.within(y, z, NC.apply_allowance(z, dt))
    assert ok, (tag, outside, float(((y.double() - z).abs() / NC.spacing(z, dt)).nan_to_num(nan=float("inf")).max()))


# ---- 1. liso_bn_relu_fwd ---------------------------------------------------------------------------------------------------------------------
def _bn_fwd(L, x, gamma, beta, rm, rv, training, relu, m, c):
    """the call on poisoned outputs and a poisoned workspace, all between guard bands -> (y, stats)"""
    lib = L.lib()
    nbytes = lib.liso_bn_workspace_bytes(c)
    y, st, ws = Guarded(m * c, x.dtype, DEV), Guarded(4 * c, torch.float32, DEV), Guarded(nbytes, torch.uint8, DEV)
    L.check(lib.liso_bn_relu_fwd(L.ptr(x), L.elem_code(x.dtype), m, c, L.ptr(gamma), L.ptr(beta), L.ptr(rm.inner), L.ptr(rv.inner), NC.MOMENTUM,
                                 NC.EPS, training, relu, L.ptr(y.inner), L.ptr(st.inner), L.ptr(ws.inner), nbytes, L.stream_ptr()), "bn_relu_fwd")
    torch.cuda.synchronize()
    assert y.intact() and st.intact() and ws.intact() and rm.intact() and rv.intact(), "guard band overwritten"
    assert _written(y) and _written(st), "an output element was not written"
    return y, st


@pytest.mark.parametrize("case", NC.FWD_CASES, ids=_id)
def test_bn_forward_training_statistics_and_apply(case):
    dt, c, m, relu = case
    L = _L(dt)
    geo, seed = NC.Geo(m, c, dt), NC.case_seed(*case)
    x = NC.make_x(m, c, dt, seed)[0].to(DEV)
    gamma, beta, rm0, rv0 = (t.to(DEV) for t in NC.make_params(c, seed))
    rm, rv = _filled(rm0), _filled(rv0)
    y, st = _bn_fwd(L, x, gamma, beta, rm, rv, 1, relu, m, c)
    ref = NC.fwd_stats_reference(x, gamma, beta, rm0, rv0, geo)
    bnd = NC.fwd_stats_bounds(x, ref, gamma, rm0, rv0, geo)
    got = _stats_dict(st.inner, c, rm.inner, rv.inner)
    ratio = NC.worst_ratio(ref, got, bnd)
    _report("bn_fwd_stats", dt, case, ratio)
    assert ratio <= 1.0, {k: NC.worst_ratio(ref, got, {k: v}) for k, v in bnd.items()}
    if m == 1:
        assert _same(rm.inner, rm0) and _same(rv.inner, rv0)  # a single row: the running statistics keep their bits
    _check_apply(x, y.inner.view(m, c), st.inner, relu, dt, case)
    # reproducible: the same call again, from the same running statistics
    rm2, rv2 = _filled(rm0), _filled(rv0)
    y2, st2 = _bn_fwd(L, x, gamma, beta, rm2, rv2, 1, relu, m, c)
    assert _same(y.inner, y2.inner) and _same(st.inner, st2.inner) and _same(rm.inner, rm2.inner) and _same(rv.inner, rv2.inner)


@pytest.mark.parametrize("case", NC.EVAL_FWD_CASES, ids=_id)
def test_bn_forward_eval_statistics_and_apply(case):
    dt, c, m, relu = case
    L = _L(dt)
    seed = NC.case_seed(*case)
    x = NC.make_x(m, c, dt, seed)[0].to(DEV)
    params = NC.make_params(c, seed)
    gamma, beta, rm0, rv0 = (t.to(DEV) for t in params)
    rm, rv = _filled(rm0), _filled(rv0)
    y, st = _bn_fwd(L, x, gamma, beta, rm, rv, 0, relu, m, c)
    assert _same(rm.inner, rm0) and _same(rv.inner, rv0)
    ref = NC.eval_stats_reference(*params)
    bnd = NC.eval_stats_bounds(ref, params[0], params[2])
    got = {k: v.cpu() for k, v in _stats_dict(st.inner, c).items()}
    ratio = NC.worst_ratio(ref, got, bnd)
    _report("bn_fwd_eval_stats", dt, case, ratio)
    assert ratio <= 1.0, {k: NC.worst_ratio(ref, got, {k: v}) for k, v in bnd.items()}
    _check_apply(x, y.inner.view(m, c), st.inner, relu, dt, case)
    y2, st2 = _bn_fwd(L, x, gamma, beta, rm, rv, 0, relu, m, c)
    assert _same(y.inner, y2.inner) and _same(st.inner, st2.inner)


# ---- 2. liso_in_relu_fwd ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", NC.IN_FWD_CASES, ids=_id)
def test_instance_norm_forward_per_sample(case):
    dt, c, m, relu = case
    L, G = _L(dt), NC.GROUPS
    lib, geo, seed = L.lib(), NC.Geo(m, c, dt), NC.case_seed(*case)
    x = NC.make_x(m, c, dt, seed, groups=G).to(DEV)
    gamma, beta, _, _ = (t.to(DEV) for t in NC.make_params(c, seed))
    nbytes = lib.liso_in_workspace_bytes(G, c)

    def call():
        y, st, ws = Guarded(G * m * c, x.dtype, DEV), Guarded(G * 4 * c, torch.float32, DEV), Guarded(nbytes, torch.uint8, DEV)
        L.check(lib.liso_in_relu_fwd(L.ptr(x), L.elem_code(x.dtype), G, m, c, L.ptr(gamma), L.ptr(beta), NC.EPS, relu, L.ptr(y.inner),
                                     L.ptr(st.inner), L.ptr(ws.inner), nbytes, L.stream_ptr()), "in_relu_fwd")
        torch.cuda.synchronize()
        assert y.intact() and st.intact() and ws.intact(), "guard band overwritten"
        assert _written(y) and _written(st), "an output element was not written"
        return y, st

    y, st = call()
    worst = 0.0
    for k in range(G):
        ref = NC.fwd_stats_reference(x[k], gamma, beta, None, None, geo)
        bnd = NC.fwd_stats_bounds(x[k], ref, gamma, None, None, geo)
        got = _stats_dict(st.inner.view(G, 4 * c)[k], c)
        ratio = NC.worst_ratio(ref, got, bnd)
        worst = max(worst, ratio)
        assert ratio <= 1.0, (k, {n: NC.worst_ratio(ref, got, {n: v}) for n, v in bnd.items()})
        _check_apply(x[k], y.inner.view(G, m, c)[k], st.inner.view(G, 4 * c)[k], relu, dt, (case, k))
    _report("in_fwd_stats", dt, case, worst)
    y2, st2 = call()
    assert _same(y.inner, y2.inner) and _same(st.inner, st2.inner)


# ---- 3. liso_bn_relu_bwd, liso_in_relu_bwd_sum -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", NC.BWD_CASES, ids=_id)
def test_bn_backward(case):
    dt, c, m, relu, training = case
    L = _L(dt)
    lib, geo = L.lib(), NC.Geo(m, c, dt)
    d = {k: v.to(DEV) for k, v in NC.make_bwd_case(dt, c, m, relu, training, NC.case_seed(*case)).items()}
    x, dy, stats = d["x"][0], d["dy"][0], d["stats"][0]
    nbytes = lib.liso_bn_workspace_bytes(c)

    def call():
        dx, gg, gb = Guarded(m * c, x.dtype, DEV), Guarded(c, torch.float32, DEV), Guarded(c, torch.float32, DEV)
        ws = Guarded(nbytes, torch.uint8, DEV)
        L.check(lib.liso_bn_relu_bwd(L.ptr(dy), L.ptr(x), L.elem_code(x.dtype), m, c, L.ptr(d["gamma"]), L.ptr(stats), training, relu,
                                     L.ptr(dx.inner), L.ptr(gg.inner), L.ptr(gb.inner), L.ptr(ws.inner), nbytes, L.stream_ptr()), "bn_relu_bwd")
        torch.cuda.synchronize()
        assert dx.intact() and gg.intact() and gb.intact() and ws.intact(), "guard band overwritten"
        assert _written(dx) and _written(gg) and _written(gb), "an output element was not written"
        return dx, gg, gb

    dx, gg, gb = call()
    ref = NC.bwd_reference(x, dy, d["gamma"], stats, training, relu, geo)
    bnd = NC.bwd_bounds(ref, geo, training)
    got = dict(dx=dx.inner.view(m, c), grad_gamma=gg.inner, grad_beta=gb.inner)
    each = {k: NC.worst_ratio(ref, got, {k: v}) for k, v in bnd.items()}
    _report("bn_bwd", dt, case, max(each.values()))
    print("   ", {k: round(v, 4) for k, v in each.items()})
    assert max(each.values()) <= 1.0, each
    dx2, gg2, gb2 = call()
    assert _same(dx.inner, dx2.inner) and _same(gg.inner, gg2.inner) and _same(gb.inner, gb2.inner)


@pytest.mark.parametrize("case", NC.IN_BWD_SUM_CASES, ids=_id)
def test_instance_norm_backward_summed_gradients(case):
    dt, c, m, relu = case
    L, G = _L(dt), NC.GROUPS
    lib, geo = L.lib(), NC.Geo(m, c, dt)
    d = {k: v.to(DEV) for k, v in NC.make_bwd_case(dt, c, m, relu, 1, NC.case_seed(*case), groups=G).items()}
    nbytes = lib.liso_in_workspace_bytes(G, c)

    def call():
        dx, gg, gb = Guarded(G * m * c, d["x"].dtype, DEV), Guarded(c, torch.float32, DEV), Guarded(c, torch.float32, DEV)
        ws = Guarded(nbytes, torch.uint8, DEV)
        L.check(lib.liso_in_relu_bwd_sum(L.ptr(d["dy"]), L.ptr(d["x"]), L.elem_code(d["x"].dtype), G, m, c, L.ptr(d["gamma"]), L.ptr(d["stats"]),
                                         relu, L.ptr(dx.inner), L.ptr(gg.inner), L.ptr(gb.inner), L.ptr(ws.inner), nbytes, L.stream_ptr()),
                "in_relu_bwd_sum")
        torch.cuda.synchronize()
        assert dx.intact() and gg.intact() and gb.intact() and ws.intact(), "guard band overwritten"
        assert _written(dx) and _written(gg) and _written(gb), "an output element was not written"
        return dx, gg, gb

    dx, gg, gb = call()
    ref, bnd = NC.in_bwd_sum_reference(d, relu, geo)
    got = dict(dx=dx.inner.view(G, m, c), grad_gamma=gg.inner, grad_beta=gb.inner)
    each = {k: NC.worst_ratio(ref, got, {k: v}) for k, v in bnd.items()}
    _report("in_bwd_sum", dt, case, max(each.values()))
    assert max(each.values()) <= 1.0, each
    dx2, gg2, gb2 = call()
    assert _same(dx.inner, dx2.inner) and _same(gg.inner, gg2.inner) and _same(gb.inner, gb2.inner)


# ---- 4. liso_conv_bn_finalize, liso_conv_in_finalize -----------------------------------------------------------------------------------------
def _compare_finalize(got_stats, co, ref, bnd, extra, tag):
    got = {k: v.cpu() for k, v in dict(_stats_dict(got_stats, co), **extra).items()}
    each = {k: NC.worst_ratio(ref, got, {k: v}) for k, v in bnd.items()}
    assert max(each.values()) <= 1.0, (tag, each)
    return max(each.values())


@pytest.mark.parametrize("rows", NC.CONV_ROWS)
def test_conv_bn_finalize(rows):
    """every co x with / without stats_shift x with / without running statistics; n = 1 through the running-statistics branch"""
    L = _L()
    lib, worst = L.lib(), 0.0
    for co in NC.CONV_CO:
        gamma, beta, rm0, rv0 = NC.make_params(co, rows + co)
        for with_shift in (False, True):
            for running in (False, True):
                for single in ((False, True) if running else (False,)):
                    tag = (rows, co, with_shift, running, single)
                    part, shift, n, co_pad = NC.conv_partials(rows, co, 31 * rows + co, with_shift, single=single)
                    ref, bnd = NC.conv_finalize_reference(part[0], co, n[0], shift, gamma, beta, rm0 if running else None, rv0 if running else None)
                    pd, gd, bd = part.to(DEV), gamma.to(DEV), beta.to(DEV)
                    sd = shift.to(DEV) if with_shift else None
                    outs = []
                    for _ in range(2):
                        st = Guarded(4 * co, torch.float32, DEV)
                        rm, rv = (_filled(rm0), _filled(rv0)) if running else (None, None)
                        L.check(lib.liso_conv_bn_finalize(L.ptr(pd), rows, co, co_pad, n[0], L.ptr(sd) if with_shift else None, L.ptr(gd), L.ptr(bd),
                                                          L.ptr(rm.inner) if running else None, L.ptr(rv.inner) if running else None,
                                                          NC.MOMENTUM, NC.EPS, L.ptr(st.inner), L.stream_ptr()), "conv_bn_finalize")
                        torch.cuda.synchronize()
                        assert st.intact() and _written(st) and (not running or (rm.intact() and rv.intact())), tag
                        outs.append((st, rm, rv))
                    st, rm, rv = outs[0]
                    extra = dict(running_mean=rm.inner, running_var=rv.inner) if running else {}
                    worst = max(worst, _compare_finalize(st.inner, co, ref, bnd, extra, tag))
                    assert _same(st.inner, outs[1][0].inner) and (not running or (_same(rm.inner, outs[1][1].inner) and _same(rv.inner, outs[1][2].inner)))
    _report("conv_bn_finalize", "fp32", (rows,), worst)


@pytest.mark.parametrize("rows", NC.CONV_ROWS)
def test_conv_in_finalize(rows):
    """three samples with their own block data, every co, with and without gamma / beta"""
    L, B = _L(), NC.GROUPS
    lib, worst = L.lib(), 0.0
    for co in NC.CONV_CO:
        gamma, beta, _, _ = NC.make_params(co, rows + co + 1)
        for affine in (False, True):
            tag = (rows, co, affine)
            part, _, n, co_pad = NC.conv_partials(rows, co, 17 * rows + co, False, samples=B)
            assert len(set(n)) == 1
            pd, gd, bd = part.to(DEV), gamma.to(DEV), beta.to(DEV)
            outs = []
            for _ in range(2):
                st = Guarded(B * 4 * co, torch.float32, DEV)
                L.check(lib.liso_conv_in_finalize(L.ptr(pd), rows, B, co, co_pad, n[0], L.ptr(gd) if affine else None, L.ptr(bd) if affine else None,
                                                  NC.EPS, L.ptr(st.inner), L.stream_ptr()), "conv_in_finalize")
                torch.cuda.synchronize()
                assert st.intact() and _written(st), tag
                outs.append(st)
            for k in range(B):
                ref, bnd = NC.conv_finalize_reference(part[k], co, n[0], None, gamma if affine else None, beta if affine else None, None, None)
                worst = max(worst, _compare_finalize(outs[0].inner.view(B, 4 * co)[k], co, ref, bnd, {}, tag + (k,)))
            assert _same(outs[0].inner, outs[1].inner)
    _report("conv_in_finalize", "fp32", (rows,), worst)


# ---- 5. liso_residual_affine_relu_f32 --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [4, 12, 96])
@pytest.mark.parametrize("pixels", [1, 77])
def test_residual_affine_relu(pixels, c):
    """every combination of NULL / given scale and of the ReLU flags; per-sample vectors with strides larger than c"""
    L, batch = _L(), 3
    lib = L.lib()
    g = torch.Generator().manual_seed(100 * pixels + c)
    a, b = (torch.randn(batch, pixels, c, generator=g) * 2.0 for _ in range(2))
    sa, sb = c + 4, c + 8
    vec = {k: torch.randn(batch, s, generator=g) for k, s in (("a_scale", sa), ("a_shift", sa), ("b_scale", sb), ("b_shift", sb))}
    ad, bd = a.to(DEV), b.to(DEV)
    vd = {k: v.to(DEV) for k, v in vec.items()}
    for has_a in (0, 1):
        for has_b in (0, 1):
            for a_relu in (0, 1):
                for b_relu in (0, 1):
                    tag = (pixels, c, has_a, has_b, a_relu, b_relu)
                    ref = NC.residual_reference(a, vec["a_scale"][:, :c] if has_a else None, vec["a_shift"][:, :c] if has_a else None, a_relu,
                                                b, vec["b_scale"][:, :c] if has_b else None, vec["b_shift"][:, :c] if has_b else None, b_relu)
                    outs = []
                    for _ in range(2):
                        out = Guarded(batch * pixels * c, torch.float32, DEV)
                        L.check(lib.liso_residual_affine_relu_f32(L.ptr(ad), L.ptr(vd["a_scale"]) if has_a else None, L.ptr(vd["a_shift"]) if has_a else None,
                                                                  sa, a_relu, L.ptr(bd), L.ptr(vd["b_scale"]) if has_b else None,
                                                                  L.ptr(vd["b_shift"]) if has_b else None, sb, b_relu, L.ptr(out.inner), batch, pixels, c,
                                                                  L.stream_ptr()), "residual_affine_relu")
                        torch.cuda.synchronize()
                        assert out.intact() and _written(out), tag
                        outs.append(out)
                    got = outs[0].inner.view(batch, pixels, c).cpu().double()
                    ok, outside = NC.within(got, ref, NC.spacing(ref, "fp32"))
                    assert ok, (tag, outside)
                    assert bool((got >= 0).all()) and 0.1 < float((got > 0).double().mean()) < 1.0
                    assert _same(outs[0].inner, outs[1].inner)
