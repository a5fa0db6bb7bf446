"""GPU: the edges of the fp16 format through every detector kernel that stores fp16 (LISO_CONV_F16 / element code 2).

The convolution cases use integer operands scaled by powers of two, so every product and every fp32 partial sum is exact and the only
rounding is the final fp32 -> fp16 store.  The expected value is the exact fp64 result converted to fp16, and the kernels must match it
value for value:
  ties       outputs in [2048, 8192), where the fp16 spacing is 2 or 4: round to nearest even, not toward zero, not bf16-style;
  overflow   outputs around 65504 / 65520: >= 65520 is +-inf, [65504, 65520) is 65504, nothing saturates;
  subnormal  fp16 subnormal inputs (n * 2^-24), and normal inputs whose products land below 2^-14: outputs keep their subnormal bits.
The same edges through BatchNorm's fp16 output (bn_act; statistics in fp32, so against the fp64 result with its rounding allowance) and
through the fp16 data gradient of the BatchNorm backward (eval mode: one exact product per element) and of the convolution."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from tests.fp16_checks import require_fp16, ulp16

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MAXH = 65504.0


def _cl(t):
    return t.to(DEV).contiguous(memory_format=torch.channels_last)


# forward families that store fp16 -- (B, Ci, Co, H, W, k, stride, pad, transposed, kernel kind of liso_conv_kernel_kind):
# Ci * k^2 ~ 2300 where the kernel allows it (the small-pixel 3x3 / 2 kernel takes <= 128 channels)
FAMILIES = {
    "roles_3x3": (1, 256, 64, 12, 40, 3, 1, 1, False, 1),
    "igemm_3x3_s2": (1, 256, 64, 16, 16, 3, 2, 1, False, 0),
    "1x1": (1, 2304, 64, 8, 32, 1, 1, 0, False, 2),
    "2x2_s2": (1, 576, 64, 16, 32, 2, 2, 0, False, 2),
    "transposed_2x2_s2": (1, 2304, 64, 8, 16, 2, 2, 0, True, 2),
    "3x3_s2_small_pixels": (1, 128, 64, 16, 64, 3, 2, 1, False, 2),
}
CASES = ["ties", "overflow", "subnormal_inputs", "subnormal_products"]
TARGET = {"ties": 4096.0, "overflow": 65512.0}


def _kind(x, Co, spec):
    from liso_amd import _lib as L
    from liso_amd.utils import mfma_conv as MC

    mode = MC._mode(x.dtype)
    xv, xps = MC.as_nhwc(x, MC._vec(mode))
    B, hi, wi, ci = xv.shape
    ho, wo = spec.out_hw(hi, wi)
    build = MC.scatter_desc if spec.transposed else MC.gather_desc
    d = build(spec, B, hi, wi, ci, xps, ho, wo, Co, Co, 0, mode, False, False, False)
    return L.lib().liso_conv_kernel_kind(ctypes.byref(d))


def _operands(case, B, R, O, H, W, k, special_taps, occ=None, seed=0):
    """x [B, R, H, W] and w [O, R, k, k] (forward layout: O outputs, R reduction channels) for one case, fp16-exact.
    ties / overflow: channel 1 of x is 4 and w[:, 1] at `special_taps` a per-output shift t (an integer: exact), chosen so that the
    median output lands on the case's target; overflow adds channel 0 = 255 with weight 256.  Output o carries the sign (-1)^o."""
    g = torch.Generator().manual_seed(seed)
    sign = 1.0 - 2.0 * (torch.arange(O) % 2).double()
    if case == "ties":
        x = torch.randint(0, 4, (B, R, H, W), generator=g).double()
        w = torch.randint(0, 4, (O, R, k, k), generator=g).double()
    elif case == "overflow":
        x = torch.randint(0, 2, (B, R, H, W), generator=g).double()
        w = torch.randint(0, 2, (O, R, k, k), generator=g).double()
    elif case == "subnormal_inputs":  # fp16 subnormals times small integers
        x = torch.randint(-3, 4, (B, R, H, W), generator=g).double() * 2.0 ** -24
        w = torch.randint(-1, 2, (O, R, k, k), generator=g).double()
    else:  # normal fp16 operands, products a * b * 2^-24 below 2^-14
        x = torch.randint(-3, 4, (B, R, H, W), generator=g).double() * 2.0 ** -12
        w = torch.randint(-1, 2, (O, R, k, k), generator=g).double() * 2.0 ** -12
    if occ is not None:
        x = x * occ
    if case in TARGET:
        w[:, :2] = 0.0
        x[:, 1] = 4.0
        if case == "overflow":
            x[:, 0] = 255.0
            for ty, tx in special_taps:
                w[:, 0, ty, tx] = 256.0
        if occ is not None:
            x[:, :2] *= occ[:, 0:1]
    w = w * sign.view(-1, 1, 1, 1)
    return x, w, sign


def _shift(case, w, sign, ref0, special_taps, where=None):
    """the per-output shift weight that puts the median of |output| (over `where`: the outputs that read the special channels) at
    the case's target"""
    if case not in TARGET:
        return w
    v = ref0 * sign.view(1, -1, 1, 1)
    med = float((v if where is None else v[where.expand_as(v)]).median())
    t = max(-2048.0, min(2048.0, round((TARGET[case] - med) / 4.0)))
    w = w.clone()
    for ty, tx in special_taps:
        w[:, 1, ty, tx] = sign * t
    return w


def _check_edges(case, y16, ref):
    """y16 (fp16, any device) == exact fp64 result rounded to fp16, and the case really exercises its edge"""
    y, r = y16.detach().cpu(), ref.detach().cpu()
    assert y.dtype == torch.float16 and y.shape == r.shape
    exp16 = r.to(torch.float16)  # (every exact value is fp32-representable here: one rounding)
    a = r.abs()
    if case == "ties":
        sp = torch.where(a >= 4096, 4.0, 2.0).double()
        ties = (a >= 2048) & (a < 8192) & (torch.remainder(a, sp) == sp / 2)
        assert int(ties.sum()) >= max(16, r.numel() // 100), "too few exact ties"
    elif case == "overflow":
        assert int((a >= 65520).sum()) > 0 and int(((a >= MAXH) & (a < 65520)).sum()) > 0 and int((a < MAXH).sum()) > 0
        assert bool((r > 0).any()) and bool((r < 0).any())
    else:
        sub = (a > 0) & (a < 2.0 ** -14)
        assert int(sub.sum()) >= r.numel() // 4, "too few subnormal outputs"
    bad = y.float() != exp16.float()
    if bool(bad.any()):
        i = int(bad.flatten().nonzero()[0])
        raise AssertionError(f"{int(bad.sum())} of {y.numel()} outputs differ from the exact result rounded to fp16; first: exact "
                             f"{float(r.flatten()[i])!r} expected {float(exp16.flatten()[i])!r} got {float(y.flatten()[i])!r}")


def _taps(k, transposed, padded):
    # taps that every output pixel reads: the centre of a padded window, any tap of a non-overlapping one; a transposed convolution
    # with kernel = stride reaches each output through exactly one tap, so the special channels carry all of them
    if transposed:
        return [(ty, tx) for ty in range(k) for tx in range(k)]
    return [(k // 2, k // 2)] if padded else [(0, 0)]


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("family", list(FAMILIES))
def test_conv_forward_fp16_store_edges(family, case):
    require_fp16()
    from liso_amd.utils import mfma_conv as MC

    B, Ci, Co, H, W, k, s, p, tr, kind = FAMILIES[family]
    spec = MC.ConvSpec(k, k, s, p, tr)
    taps = _taps(k, tr, p > 0)
    x, w, sign = _operands(case, B, Ci, Co, H, W, k, taps, seed=Ci + k)

    def layout(wf):  # forward [O, R, k, k] -> the module's weight layout
        return wf.transpose(0, 1).contiguous() if tr else wf

    def exact(wf):
        return (F.conv_transpose2d if tr else F.conv2d)(x, layout(wf), None, stride=s, padding=p)

    w = _shift(case, w, sign, exact(w), taps)
    ref = exact(w)
    xd = _cl(x.half())
    assert torch.equal(xd.double().cpu(), x) and torch.equal(w.half().double(), w)  # (operands exact in fp16)
    assert _kind(xd, Co, spec) == kind, f"{family} does not take the kernel it is meant to test"
    y16, _ = MC.conv_forward(xd, layout(w).float().to(DEV), None, spec)
    _check_edges(case, y16, ref)


@pytest.mark.parametrize("case", CASES)
def test_sparse_first_rpn_layer_fp16_store_edges(case, monkeypatch):
    """the sparse canvas kernel of the first RPN layer (3x3 / 2, 64 -> 64, fp16 raw output through fused_conv with its BatchNorm)"""
    require_fp16()
    from liso_amd.utils import mfma_conv as MC

    B, H, W = 1, 32, 64
    g = torch.Generator().manual_seed(11)
    occ = (torch.rand(B, 1, H, W, generator=g) < 0.6).double()
    taps = [(1, 1)]
    x, w, sign = _operands(case, B, 64, 64, H, W, 3, taps, occ=occ, seed=5)

    def exact(wf):
        return F.conv2d(x, wf, None, stride=2, padding=1)

    w = _shift(case, w, sign, exact(w), taps, where=occ[:, :, ::2, ::2].bool())  # (the window centres that are occupied)
    ref = exact(w)
    calls = []
    real = MC._sparse_stem

    def spy(*a, **kw):
        r = real(*a, **kw)
        calls.append(r is not None)
        return r

    monkeypatch.setenv("LISO_SPARSE_STEM", "1")
    monkeypatch.setattr(MC, "_sparse_stem", spy)
    conv = torch.nn.Conv2d(64, 64, 3, stride=2, padding=1, bias=False).to(DEV)
    bn = torch.nn.BatchNorm2d(64, eps=1e-3, momentum=0.01).to(DEV).train()
    with torch.no_grad():
        conv.weight.copy_(w.float())
    with torch.no_grad():
        y, _ = MC.fused_conv(_cl(x.half()), None, conv, out_bn=bn, spec=MC.ConvSpec(3, 3, 2, 1), occupancy=occ.float().to(DEV))
    assert calls == [True], "the sparse kernel did not run"
    _check_edges(case, y, ref)


@pytest.mark.parametrize("case", ["ties", "overflow"])
@pytest.mark.parametrize("family", ["roles_3x3", "2x2_s2"])
def test_conv_data_gradient_fp16_store_edges(family, case):
    """conv_dgrad with the default out_dtype (dy.dtype: fp16): dx[r] = sum over (o, taps) of dy[o] * w[o, r] (reduction over the
    forward's output channels)"""
    require_fp16()
    from liso_amd.utils import mfma_conv as MC

    if family == "roles_3x3":
        B, Ci, Co, H, W, k, s, p = 1, 64, 256, 12, 40, 3, 1, 1
    else:
        B, Ci, Co, H, W, k, s, p = 1, 64, 576, 16, 32, 2, 2, 0
    spec = MC.ConvSpec(k, k, s, p, False)
    Ho, Wo = spec.out_hw(H, W)
    # the data gradient is a convolution of dy (Co "reduction" channels) -- a transposed one for stride 2: then each dx pixel is
    # reached through one tap, which the special channels must cover
    taps = _taps(k, s > 1, p > 0)
    dy, wt, sign = _operands(case, B, Co, Ci, Ho, Wo, k, taps, seed=Co)  # wt: [Ci, Co, k, k] (output = dx channels)

    def exact(wf):  # wf [Ci, Co, k, k] -> conv weight [Co, Ci, k, k]
        return torch.nn.grad.conv2d_input((B, Ci, H, W), wf.transpose(0, 1), dy, stride=s, padding=p)

    wt = _shift(case, wt, sign, exact(wt), taps)  # (3x3 / 1 / 1 reads its taps mirrored: the centre stays the centre)
    ref = exact(wt)
    dyd = _cl(dy.half())
    assert torch.equal(dyd.double().cpu(), dy) and torch.equal(wt.half().double(), wt)
    dx = MC.conv_dgrad(dyd, wt.transpose(0, 1).contiguous().float().to(DEV), spec, (B, Ci, H, W))
    assert dx.dtype == torch.float16
    _check_edges(case, dx, ref)


# ---- BatchNorm: bn_act's fp16 output (training statistics in fp32) and the fp16 data gradient of liso_bn_relu_bwd -------------------
def _bn_forward(gamma, beta, seed=2):
    from liso_amd.networks.centerpoint.fused_bn import bn_act

    torch.manual_seed(seed)
    C = gamma.numel()
    x = (torch.randn(2, C, 16, 24) * 2 + 0.5).half()
    bn = torch.nn.BatchNorm2d(C).to(DEV).train()
    with torch.no_grad():
        bn.weight.copy_(gamma), bn.bias.copy_(beta)
    y = bn_act(_cl(x), bn, relu=False)
    assert y.dtype == torch.float16
    x64 = x.double()
    mean, var = x64.mean(dim=(0, 2, 3), keepdim=True), x64.var(dim=(0, 2, 3), unbiased=False, keepdim=True)
    ref = (x64 - mean) / torch.sqrt(var + bn.eps) * gamma.double().view(1, -1, 1, 1) + beta.double().view(1, -1, 1, 1)
    return y.cpu(), ref


def _nearest(y, ref, slack):
    """finite outputs within half an fp16 ulp of the fp64 value, plus `slack` for the fp32 statistics"""
    f = torch.isfinite(y)
    err = (y.double() - ref).abs()[f]
    lim = (0.5 * ulp16(ref) + slack)[f]
    assert bool((err <= lim).all()), float((err / lim).max())


@pytest.mark.parametrize("case", ["ties", "overflow", "subnormal"])
def test_bn_act_fp16_output_edges(case):
    require_fp16()
    C = 64
    sign = 1.0 - 2.0 * (torch.arange(C) % 2).float()
    if case == "ties":  # gamma * xhat + beta in [2048, 8192)
        gamma, beta = torch.full((C,), 1000.0) * sign, torch.full((C,), 5000.0) * sign
    elif case == "overflow":  # crosses 65520
        gamma, beta = torch.full((C,), 300.0), torch.full((C,), 65512.0) * sign
    else:  # |y| < 2^-14
        gamma, beta = torch.full((C,), 2.0 ** -20) * sign, torch.zeros(C)
    y, ref = _bn_forward(gamma, beta)
    a = ref.abs()
    if case == "overflow":
        hi, lo = a > 65520 * (1 + 1e-3), a < MAXH * (1 - 1e-3)
        assert int(hi.sum()) > 0 and int(lo.sum()) > 0
        assert bool(torch.isinf(y[hi]).all()) and bool((y[hi].sign() == ref[hi].sign()).all()), "saturated instead of overflowing"
        assert bool(torch.isfinite(y[lo]).all())
    else:
        assert bool(torch.isfinite(y).all())
    if case == "subnormal":
        assert int((a < 2.0 ** -14).sum()) >= ref.numel() // 2 and int(((y != 0) & (y.abs() < 2.0 ** -14)).sum()) >= ref.numel() // 4
    _nearest(y, ref, 2e-5 * float(a.max()))


@pytest.mark.parametrize("case", CASES)
def test_bn_backward_fp16_data_gradient_edges(case, monkeypatch):
    """liso_bn_relu_bwd in eval mode: dx = gamma * invstd * dy, one exact fp32 product per element (invstd = 1), so the fp16 store is
    the only rounding and dx must equal the exact product rounded to fp16"""
    require_fp16()
    from liso_amd.utils import mfma_conv as MC

    C, B, H, W = 64, 2, 16, 24
    g = torch.Generator().manual_seed(4)
    sign = (1.0 - 2.0 * (torch.arange(C) % 2).double()).view(1, -1, 1, 1)
    if case == "ties":  # 3 * dy in [2048, 8192)
        dy, gam = torch.randint(683, 2731, (B, C, H, W), generator=g).double(), 3.0
    elif case == "overflow":  # 17 * dy around 65520 (dy in [3700, 4000): even, multiples of 34 reach [65504, 65520))
        dy, gam = torch.randint(1850, 2000, (B, C, H, W), generator=g).double() * 2, 17.0
    elif case == "subnormal_inputs":
        dy, gam = torch.randint(-300, 301, (B, C, H, W), generator=g).double() * 2.0 ** -24, 3.0
    else:
        dy, gam = torch.randint(-300, 301, (B, C, H, W), generator=g).double() * 2.0 ** -12, 3.0 * 2.0 ** -12
    dy = (dy * sign).half().double()
    x = torch.randn(B, C, H, W, generator=g).half()
    gamma = torch.nn.Parameter(torch.full((C,), gam, device=DEV))
    ones, zeros = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
    grp = {"gamma": gamma, "beta": None, "stats": torch.cat([gamma.detach(), zeros, zeros, ones]).contiguous()}
    dyd = _cl(dy.half())
    assert torch.equal(dyd.double().cpu(), dy)
    dx, _, _ = MC._bn_backward_group(dyd, _cl(x), grp, False, False)
    _check_edges(case, dx, dy * gam)
