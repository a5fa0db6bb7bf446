"""GPU: fp16 as the third storage type of the detector path (LISO_CONV_F16 / element code 2) and its device-resident loss scale.

Per kernel against fp64 on fp16-rounded operands (and bit for bit on small-integer data, where fp16 is exact: a wrong lane or k mapping
of the f16 MFMA shows up there), the whole detector against the exact fp32 path at full size, the fp16 train step (eager, one graph,
two graphs), overflow handling of the loss scale, BASELINE configs[4] in its stated dtype, and guard bands around the new launches.
Every test first checks on the host that fp16 is supported before it allocates or launches anything."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.guarded_alloc import guarded

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
HEADS = ("pos", "dims", "rot", "probs")


def _require_fp16():
    from liso_amd import _lib as L

    assert hasattr(L, "CONV_F16") and hasattr(L, "elem_code"), "fp16 storage is not built"
    assert L.elem_code(torch.float16) == L.ELEM_F16 == 2
    return L


def _ref_conv(x, w, b, s, p, transposed):
    x, w = x.double(), w.double()
    b = b.double() if b is not None else None
    return F.conv_transpose2d(x, w, b, stride=s, padding=p) if transposed else F.conv2d(x, w, b, stride=s, padding=p)


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-12))


def _cl(t):
    return t.cuda().contiguous(memory_format=torch.channels_last)


# (B, Ci, Co, H, W, k, stride, pad, transposed): the detector's geometries (rpn.py, center_head.py) and ragged maps
GEOMS = [
    (2, 64, 64, 64, 64, 3, 1, 1, False),      # backbone 3x3 (conv_roles_kernel)
    (1, 64, 64, 40, 72, 3, 2, 1, False),      # stride-2 stage entry
    (2, 128, 128, 32, 32, 1, 1, 0, False),    # 1x1
    (2, 64, 128, 32, 64, 2, 2, 0, False),     # deblock conv k2 s2
    (2, 256, 128, 16, 16, 2, 2, 0, True),     # transposed k2 s2
    (1, 384, 64, 32, 32, 3, 1, 1, False),     # head shared conv
    (2, 64, 3, 32, 32, 3, 1, 1, False),       # head output conv
    (1, 16, 32, 19, 45, 3, 1, 1, False),      # ragged map, partial tiles
    (3, 32, 96, 9, 7, 3, 2, 1, False),
]


@pytest.mark.parametrize("geom", GEOMS)
def test_fp16_forward_dgrad_wgrad_vs_fp64(geom):
    L = _require_fp16()
    from liso_amd.utils import mfma_conv as MC

    B, Ci, Co, H, W, k, s, p, tr = geom
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, Ci, H, W, generator=g).half().float()
    w = (torch.randn((Ci, Co, k, k) if tr else (Co, Ci, k, k), generator=g) / (Ci * k * k) ** 0.5).half().float()
    b = torch.randn(Co, generator=g) * 0.3
    spec = MC.ConvSpec(k, k, s, p, tr)
    xd, wd, bd = _cl(x.half()), w.cuda(), b.cuda()
    y32, _ = MC.conv_forward(xd, wd, bd, spec, out_dtype=torch.float32)
    ref = _ref_conv(x, w, b, s, p, tr)
    # fp16 x fp16 products are exact in fp32: only the fp32 accumulation rounds (bf16's budget: 2e-5)
    assert _rel(y32, ref) <= 2e-5, _rel(y32, ref)
    y16, _ = MC.conv_forward(xd, wd, bd, spec)
    assert y16.dtype == torch.float16
    # fp16 output = the correctly rounded fp32 result: equal to the fp32 launch's values rounded, one fp16 ulp at most where a sum lands
    # next to a rounding boundary (ties, accumulation order)
    r16 = y32.half().float()
    ulp = torch.finfo(torch.float16).eps * r16.abs().clamp(min=2.0 ** -14)
    diff = (y16.float() - r16).abs()
    assert bool((diff <= ulp).all()), float((diff / ulp).max())
    assert float((diff > 0).double().mean()) <= 1e-3
    gen = torch.Generator().manual_seed(7)
    dy = torch.randn(ref.shape, generator=gen).half().float()
    x64, w64, b64 = (t.double().requires_grad_(True) for t in (x, w, b))
    gx, gw, gb = torch.autograd.grad(_ref_conv(x64, w64, b64, s, p, tr), [x64, w64, b64], dy.double())
    dyd = _cl(dy.half())
    dx = MC.conv_dgrad(dyd, wd, spec, tuple(x.shape), out_dtype=torch.float32)
    assert _rel(dx, gx) <= 2e-5, _rel(dx, gx)
    dw, db = MC.conv_wgrad(xd, dyd, tuple(w.shape), spec)
    assert _rel(dw, gw) <= 4e-5, _rel(dw, gw)
    assert _rel(db, gb) <= 4e-5, _rel(db, gb)


@pytest.mark.parametrize("geom", [GEOMS[0], GEOMS[1], GEOMS[2], GEOMS[4], (2, 64, 64, 40, 40, 3, 1, 1, False)])
def test_fp16_small_integers_bit_exact(geom):
    """integers in [-2, 2]: every operand, product and partial sum is exact in fp16 x fp16 -> fp32, so forward, data and weight
    gradient must equal the fp64 result bit for bit (and the fp16 output wherever |y| <= 2048)"""
    L = _require_fp16()
    from liso_amd.utils import mfma_conv as MC

    B, Ci, Co, H, W, k, s, p, tr = geom
    g = torch.Generator().manual_seed(1)
    x = torch.randint(-2, 3, (B, Ci, H, W), generator=g).float()
    w = torch.randint(-2, 3, (Ci, Co, k, k) if tr else (Co, Ci, k, k), generator=g).float()
    b = torch.randint(-3, 4, (Co,), generator=g).float()
    spec = MC.ConvSpec(k, k, s, p, tr)
    xd = _cl(x.half())
    ref = _ref_conv(x, w, b, s, p, tr).float()
    y32, _ = MC.conv_forward(xd, w.cuda(), b.cuda(), spec, out_dtype=torch.float32)
    assert torch.equal(y32.cpu(), ref)
    y16, _ = MC.conv_forward(xd, w.cuda(), b.cuda(), spec)
    m = ref.abs() <= 2048
    assert torch.equal(y16.float().cpu()[m], ref[m])
    dy = torch.randint(-2, 3, tuple(ref.shape), generator=g).float()
    x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
    gx, gw = torch.autograd.grad(_ref_conv(x64, w64, None, s, p, tr), [x64, w64], dy.double())
    dyd = _cl(dy.half())
    dx = MC.conv_dgrad(dyd, w.cuda(), spec, tuple(x.shape), out_dtype=torch.float32)
    assert torch.equal(dx.cpu(), gx.float())
    dw, db = MC.conv_wgrad(xd, dyd, tuple(w.shape), spec)
    assert torch.equal(dw.cpu(), gw.float()) and torch.equal(db.cpu(), dy.sum(dim=(0, 2, 3)))


@pytest.mark.parametrize("integer", [False, True], ids=["random", "integer"])
def test_fp16_sparse_first_rpn_layer(integer, monkeypatch):
    """the sparse canvas kernels of the first RPN layer (3x3 / 2, 64 -> 64) with fp16 tensors against the dense fp16 kernels and fp64:
    forward at every pixel, data gradient at the occupied cells"""
    L = _require_fp16()
    from liso_amd.utils import mfma_conv as MC

    torch.manual_seed(4)
    B, H, W = 2, 128, 128
    occ = (torch.rand(B, 1, H, W) < 0.05).float()
    occ[:, :, 0, 0] = occ[:, :, H - 1, W - 1] = 1.0
    if integer:
        x = torch.randint(-2, 3, (B, 64, H, W)).float() * occ
        w = torch.randint(-2, 3, (64, 64, 3, 3)).float()
        g0 = torch.randint(-2, 3, (B, 64, H // 2, W // 2)).float()
    else:
        x = torch.randn(B, 64, H, W).half().float() * occ
        w = (torch.randn(64, 64, 3, 3) / 24.0).half().float()
        g0 = torch.randn(B, 64, H // 2, W // 2).half().float()
    conv = torch.nn.Conv2d(64, 64, 3, stride=2, padding=1, bias=False).cuda()
    bn = torch.nn.BatchNorm2d(64, eps=1e-3, momentum=0.01).cuda().train()
    with torch.no_grad():
        conv.weight.copy_(w)
    spec = MC.ConvSpec(3, 3, 2, 1)
    x64 = x.double().requires_grad_(True)
    ref = F.conv2d(x64, w.double(), None, stride=2, padding=1)
    gref, = torch.autograd.grad(ref, [x64], g0.double())
    res = []
    for sparse in ("0", "1"):
        monkeypatch.setenv("LISO_SPARSE_STEM", sparse)
        xd = _cl(x.half()).requires_grad_(True)
        y, _ = MC.fused_conv(xd, None, conv, out_bn=bn, spec=spec, occupancy=occ.cuda())  # (raw output; the BatchNorm is folded forward)
        assert y.dtype == torch.float16
        (y.float() * g0.cuda()).sum().backward()
        res.append((y.detach().float().cpu(), xd.grad.float().cpu()))
    m = occ.bool().expand_as(gref)
    for y, gx in res:
        if integer:
            assert torch.equal(y, ref.detach().float()) and torch.equal(gx[m], gref.float()[m])
        else:
            assert _rel(y, ref) <= 1e-3 and _rel(gx[m], gref[m]) <= 1e-3
    assert float(res[1][1][~m].abs().max()) == 0.0  # (the sparse data gradient writes occupied cells only)


@pytest.mark.parametrize("relu", [False, True])
def test_fp16_batchnorm_forward_backward(relu):
    L = _require_fp16()
    from liso_amd.networks.centerpoint.fused_bn import bn_act

    torch.manual_seed(2)
    x = (torch.randn(2, 64, 40, 48) * 2 + 0.5).half()
    bn = torch.nn.BatchNorm2d(64).cuda().train()
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5), bn.bias.uniform_(-0.3, 0.3)
    ref = torch.nn.BatchNorm2d(64).double().train()
    ref.load_state_dict({k: v.double() if v.is_floating_point() else v for k, v in bn.state_dict().items()})
    xd = _cl(x).requires_grad_(True)
    y = bn_act(xd, bn, relu=relu)
    assert y.dtype == torch.float16
    x64 = x.double().requires_grad_(True)
    y64 = ref(x64)
    if relu:
        y64 = torch.relu(y64)
    # fp16 output = correctly rounded: within half an fp16 ulp of fp64, plus the rounding of the fp32 statistics
    err = (y.float().cpu().double() - y64.detach()).abs()
    assert bool((err <= 2.0 ** -11 * y64.detach().abs() + 2e-5 * float(y64.detach().abs().max())).all()), float(err.max())
    gy = torch.randn(y64.shape).half()
    (y.float() * _cl(gy).float()).sum().backward()
    gx64, gw64, gb64 = torch.autograd.grad(y64, [x64, ref.weight, ref.bias], gy.double())
    assert _rel(xd.grad.float(), gx64) <= 2e-3, _rel(xd.grad.float(), gx64)
    assert _rel(bn.weight.grad, gw64) <= 1e-3 and _rel(bn.bias.grad, gb64) <= 1e-3
    assert _rel(bn.running_mean, ref.running_mean) <= 1e-4 and _rel(bn.running_var, ref.running_var) <= 1e-4


def test_fp16_pillar_canvas_forward_backward():
    """liso_pfn_forward_scatter / liso_pfn_backward with an fp16 canvas: the fp32 canvas rounded, and the same parameter gradients
    as from an fp32 canvas gradient carrying the same (fp16-representable) values"""
    L = _require_fp16()
    from liso_amd.networks.pcl_to_feature_grid.pcl_to_feature_grid import PointsPillarFeatureNetWrapper
    from liso_amd.utils.config import default_cfg

    cfg = default_cfg(grid=256, bev_range_m=100.0)
    torch.manual_seed(0)
    net = PointsPillarFeatureNetWrapper(cfg).to(DEV).train()
    g = torch.Generator().manual_seed(3)
    clouds = [(torch.rand(30000, 4, generator=g) * torch.tensor([100.0, 100, 3, 1]) - torch.tensor([50.0, 50, 1.5, 0])).to(DEV)
              for _ in range(2)]
    state = {k: v.clone() for k, v in net.state_dict().items()}
    out = {}
    for dtype in (torch.float32, torch.float16):
        net.load_state_dict(state)
        net.out_dtype = dtype
        net.zero_grad()
        bev, occ = net(clouds)
        assert bev.dtype == dtype
        gcan = torch.randn(bev.shape, generator=torch.Generator().manual_seed(9)).half().to(DEV).to(dtype)
        (bev.float() * gcan.float()).sum().backward()
        out[dtype] = (bev.detach().float(), occ.clone(), [p.grad.clone() for p in net.parameters() if p.grad is not None])
    b32, o32, g32 = out[torch.float32]
    b16, o16, g16 = out[torch.float16]
    assert torch.equal(o32, o16)
    assert torch.equal(b16, b32.half().float())
    for a, b in zip(g16, g32):
        assert _rel(a, b) <= 1e-5, _rel(a, b)


def _setup(grid, rng, B, n, dtype, seed=0, **kw):
    from liso_amd.datasets.synthetic import detector_batch
    from liso_amd.trainer import DetectorTrainer
    from liso_amd.utils.config import default_cfg

    torch.manual_seed(seed)
    tr = DetectorTrainer(default_cfg(grid=grid, bev_range_m=rng), DEV, compute_dtype=dtype, total_steps=20, **kw)
    pcls, targets = detector_batch(seed + 5, B, DEV, n_points=n, grid=grid, bev_range_m=rng)
    return tr, pcls, targets


def test_fp16_detector_logit_error_vs_exact_fp32_at_full_size():
    """120k points, 512^2, B = 1, train-mode BatchNorm, the seed of test_bf16_detector_logit_error_vs_exact_fp32_at_full_size: fp16 and
    bf16 raw logits against the exact fp32 path; fp16 must be well inside bf16's error on every head"""
    L = _require_fp16()
    from liso_amd.utils import mfma_conv as MC

    prev = MC.fp32_mode()
    raw, loss = {}, {}
    try:
        tr32, pcls, targets = _setup(512, 100.0, 1, 120000, torch.float32, seed=11)
        MC.set_fp32_mode("exact")
        sd = tr32.net.state_dict()
        for dtype in (torch.float32, torch.bfloat16, torch.float16):
            tr = tr32 if dtype == torch.float32 else _setup(512, 100.0, 1, 120000, dtype, seed=11)[0]
            tr.net.load_state_dict(sd)
            tr.model.train()
            with torch.no_grad():
                _, _, r, _ = tr.net(None, pcls, None, decode=False)
            raw[dtype] = {h: r[h].detach().double() for h in HEADS}
            loss[dtype] = float(tr.loss(pcls, targets)[0].detach())
            if tr is not tr32:
                del tr
    finally:
        MC.set_fp32_mode(prev)
    rep = {}
    for dtype in (torch.bfloat16, torch.float16):
        for h in HEADS:
            a, b = raw[dtype][h], raw[torch.float32][h]
            rep[(dtype, h)] = (float((a - b).abs().max() / b.abs().max()), float((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt()))
    print("vs exact fp32, per head (max / range, rms / rms):",
          {f"{str(d).split('.')[-1]}:{h}": (f"{v[0]:.2e}", f"{v[1]:.2e}") for (d, h), v in rep.items()},
          "loss", {str(d).split('.')[-1]: f"{abs(loss[d] - loss[torch.float32]) / abs(loss[torch.float32]):.2e}"
                   for d in (torch.bfloat16, torch.float16)})
    for h in HEADS:
        mx, rms = rep[(torch.float16, h)]
        bmx, brms = rep[(torch.bfloat16, h)]
        assert mx <= 2e-2 and rms <= 1.5e-2, (h, mx, rms)
        assert mx <= 0.5 * bmx and rms <= 0.5 * brms, (h, mx, bmx, rms, brms)


def test_fp16_eager_step_trains_and_is_reproducible():
    L = _require_fp16()
    tr, pcls, targets = _setup(256, 100.0, 2, 60000, torch.float16, seed=3)
    assert tr.loss_scaler is not None and tr.loss_scaler.dynamic
    sd = {k: v.clone() for k, v in tr.net.state_dict().items()}
    tr.model.train()
    total, _, _ = tr.loss(pcls, targets)
    tr._backward(total)  # (seeded with the default initial loss scale: it must not overflow on a fresh network)
    assert torch.isfinite(total)
    print("fp16 first backward: scale", tr.loss_scale_stats()["scale"], "max |scaled grad|", float(tr.optimizer.flat_grad.abs().max()))
    for n, p in tr.net.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and torch.isfinite(p.grad).all(), n
    tr.net.load_state_dict(sd)
    tr.optimizer.zero_grad()
    # two identical steps from the same state: bitwise identical
    runs = []
    for _ in range(2):
        t2, _, _ = _setup(256, 100.0, 2, 60000, torch.float16, seed=3)
        t2.net.load_state_dict(sd)
        l0 = float(t2.step(pcls, targets))
        runs.append((l0, torch.cat([p.detach().flatten() for p in t2.net.parameters()]).cpu()))
        del t2
    assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1])
    a = [float(tr.step(pcls, targets)) for _ in range(6)]
    st = tr.loss_scale_stats()
    print("fp16 eager losses", a, "loss scale", st)
    assert all(np.isfinite(a)) and a[-1] < a[0], a
    assert st["applied_steps"] + st["skipped_steps"] == 6 and st["applied_steps"] >= 5


def test_fp16_graph_step_equals_eager_and_two_graphs_equal_one():
    """the graph-captured fp16 step runs with the dynamic loss scale (a host sync would fail the capture) and equals the eager step;
    the two-graph step equals the one-graph step -- losses and parameters after 3 steps, bit for bit"""
    L = _require_fp16()
    from liso_amd.datasets.synthetic import detector_batch
    from liso_amd.trainer import DetectorTrainer
    from liso_amd.utils.config import default_cfg

    pcls, targets = detector_batch(44, 2, DEV, n_points=30000, grid=256, bev_range_m=50.0)
    out = []
    for use_graph, buckets in ((False, None), (True, 1), (True, 2)):
        torch.manual_seed(3)
        tr = DetectorTrainer(default_cfg(grid=256, bev_range_m=50.0), DEV, compute_dtype=torch.float16, total_steps=12,
                             use_graph=use_graph, grad_buckets=buckets)
        losses = [float(tr.step(pcls, targets)) for _ in range(3)]
        if use_graph:
            assert tr.n_grad_buckets == buckets
        out.append((losses, torch.cat([p.detach().flatten() for p in tr.net.parameters()]).cpu(), tr.loss_scale_stats()))
        del tr
    print("fp16 eager / graph / two graphs:", [(o[0], o[2]) for o in out])
    assert out[0][0] == out[1][0] == out[2][0], [o[0] for o in out]
    assert torch.equal(out[0][1], out[1][1]) and torch.equal(out[1][1], out[2][1])
    assert out[0][2] == out[1][2] == out[2][2]


def test_loss_scale_overflow_skips_the_step_and_backs_off_then_grows_back():
    """a scale that overflows the fp16 gradients: the step leaves parameters, both AdamW moments and the device step counter bitwise
    unchanged, halves the scale and counts one skipped step; after growth_interval clean steps the scale doubles again"""
    L = _require_fp16()
    tr, pcls, targets = _setup(256, 100.0, 2, 60000, torch.float16, seed=3)
    opt = tr.optimizer
    for _ in range(4):  # steps until one is applied: non-zero moments (a fresh network may back off first)
        tr.step(pcls, targets)
        st0 = tr.loss_scale_stats()
        if st0["applied_steps"] == 1:
            break
    assert st0["applied_steps"] == 1, st0
    skipped0 = st0["skipped_steps"]
    big = 2.0 ** 40
    tr.loss_scaler.set_scale(big)
    before = [t.clone() for t in (opt.flat_param, opt.flat_exp_avg, opt.flat_exp_avg_sq)]
    loss = tr.step(pcls, targets)
    assert torch.isfinite(loss)  # (the loss itself is unscaled fp32; its gradients overflowed)
    assert not torch.isfinite(opt.flat_grad).all()
    for a, b in zip(before, (opt.flat_param, opt.flat_exp_avg, opt.flat_exp_avg_sq)):
        assert torch.equal(a, b)
    st = tr.loss_scale_stats()
    assert st["scale"] == big / 2 and st["skipped_steps"] == skipped0 + 1 and st["applied_steps"] == 1 and st["growth_tracker"] == 0
    # back to a safe scale; growth after growth_interval clean steps
    tr.loss_scaler.set_scale(st0["scale"])
    tr.loss_scaler.growth_interval = 2
    tr.step(pcls, targets)
    assert tr.loss_scale_stats()["scale"] == st0["scale"]
    tr.step(pcls, targets)
    st2 = tr.loss_scale_stats()
    assert st2["scale"] == 2 * st0["scale"] and st2["applied_steps"] == 3 and st2["skipped_steps"] == skipped0 + 1
    assert not torch.equal(before[0], opt.flat_param)
    # a checkpoint carries the loss scale: a fresh trainer restored from it continues at the same scale / counters, not at init_scale
    sd = opt.state_dict()
    tr2, _, _ = _setup(256, 100.0, 2, 60000, torch.float16, seed=3)
    tr2.optimizer.load_state_dict(sd)
    assert tr2.loss_scale_stats() == tr.loss_scale_stats() and tr2.loss_scaler.growth_interval == 2


def test_fixed_loss_scale_and_loop_trainer_forwards_fp16():
    L = _require_fp16()
    from liso_amd.datasets.synthetic import slim_pair
    from liso_amd.trainer import LisoLoopTrainer
    from liso_amd.utils.config import apply_slim_simple_knn_training, default_cfg

    tr, pcls, targets = _setup(128, 50.0, 1, 20000, torch.float16, seed=1, loss_scale=256.0)
    assert not tr.loss_scaler.dynamic
    for _ in range(2):
        assert np.isfinite(float(tr.step(pcls, targets)))
    assert tr.loss_scale_stats()["scale"] == 256.0
    torch.manual_seed(0)
    lt = LisoLoopTrainer(apply_slim_simple_knn_training(default_cfg(grid=256, bev_range_m=50.0)), DEV, compute_dtype=torch.float16,
                         total_steps=10)
    assert lt.detector.net.model.pfn.out_dtype == torch.float16 and lt.detector.loss_scaler is not None
    pairs = [slim_pair(40 + i, DEV, n_points=20000, grid=256, bev_range_m=50.0) for i in range(2)]
    losses = [float(lt.step(*pairs[i % 2])) for i in range(2)]
    assert np.all(np.isfinite(losses)), losses


def test_config5_train_step_300k_points_1024_grid_fp16():
    """BASELINE configs[4] in its stated dtype: 300k 5-channel points, 1024^2 BEV, fp16 tensors with the dynamic loss scale: finite,
    loss within 5e-2 of the fp32 step's, two optimizer steps"""
    L = _require_fp16()
    from liso_amd.datasets.synthetic import detector_batch
    from liso_amd.trainer import DetectorTrainer
    from liso_amd.utils.config import default_cfg

    losses = {}
    for dtype in (torch.float16, torch.float32):
        torch.manual_seed(5)
        cfg = default_cfg(grid=1024, bev_range_m=100.0)
        cfg.data.num_point_channels = 5
        tr = DetectorTrainer(cfg, DEV, compute_dtype=dtype, total_steps=8)
        pcls, targets = detector_batch(9, 1, DEV, n_points=300000, grid=1024, bev_range_m=100.0)
        gen = torch.Generator().manual_seed(3)
        pcls = [torch.cat([p, (torch.randint(0, 10, (p.shape[0], 1), generator=gen).float() * 0.05).to(DEV)], dim=1) for p in pcls]
        tr.model.train()
        total, _, _ = tr.loss(pcls, targets)
        tr._backward(total)
        assert torch.isfinite(total)
        for n, p in tr.net.named_parameters():
            if p.requires_grad:
                assert p.grad is not None and torch.isfinite(p.grad).all(), n
        losses[dtype] = float(total)
        if dtype == torch.float16:
            l0, l1 = float(tr.step(pcls, targets)), float(tr.step(pcls, targets))
            assert np.isfinite(l0) and np.isfinite(l1)
            assert tr.loss_scale_stats()["applied_steps"] >= 1
        del tr
        torch.cuda.empty_cache()
    print("configs[4] losses", losses)
    assert abs(losses[torch.float16] - losses[torch.float32]) <= 5e-2 * abs(losses[torch.float32]), losses


def test_fp16_launches_under_guard_bands():
    """the fp16 canvas at the max_voxels cap, the fp16 sparse first layer beyond its cell-list capacity, fp16 convolutions on odd
    grids and one fp16 train step -- every wrapper-allocated buffer between canary bands that must come back untouched"""
    L = _require_fp16()
    from liso_amd.networks.pcl_to_feature_grid.pcl_to_feature_grid import PointsPillarFeatureNetWrapper
    from liso_amd.utils import mfma_conv as MC
    from liso_amd.utils.config import default_cfg

    cfg = default_cfg(grid=512, bev_range_m=100.0)
    torch.manual_seed(0)
    net = PointsPillarFeatureNetWrapper(cfg).to(DEV).train()
    net.out_dtype = torch.float16
    g = torch.Generator().manual_seed(3)
    uniform = torch.rand(200000, 4, generator=g) * torch.tensor([100.0, 100, 3, 1]) - torch.tensor([50.0, 50, 1.5, 0])
    with guarded() as gd:
        bev, occ = net([uniform.to(DEV), torch.zeros(0, 4, device=DEV)])
        gd.check()
        assert bev.dtype == torch.float16 and float(occ[0].sum()) == 40000.0 and float(occ[1].sum()) == 0
        bev.float().square().sum().backward()
        gd.check()
    B, H = 1, 512
    occ = (torch.rand(B, 1, H, H, device=DEV) < 0.3)  # more occupied cells than the sparse kernels' lists hold
    x = torch.where(occ, torch.randn(B, 64, H, H, device=DEV), torch.zeros((), device=DEV)).half().contiguous(memory_format=torch.channels_last)
    conv = torch.nn.Conv2d(64, 64, 3, stride=2, padding=1, bias=False).to(DEV)
    bn = torch.nn.BatchNorm2d(64).to(DEV).train()
    try:
        with guarded() as gd:
            y, _ = MC.fused_conv(x, None, conv, out_bn=bn, spec=MC.ConvSpec(3, 3, 2, 1), occupancy=occ.float())
            gd.check()
        assert torch.isfinite(y).all()
    finally:
        MC.reset_sparse_stem_overflow(DEV)
    with guarded() as gd:
        for (Ci, Co, Hh, Ww, k, s, p, tr) in [(64, 64, 37, 53, 3, 1, 1, False), (64, 128, 37, 53, 3, 2, 1, False),
                                             (128, 64, 19, 27, 2, 2, 0, True), (64, 3, 31, 33, 3, 1, 1, False)]:
            spec = MC.ConvSpec(k, k, s, p, tr)
            xi = torch.randn(2, Ci, Hh, Ww, device=DEV).half().contiguous(memory_format=torch.channels_last)
            w = torch.randn((Ci, Co, k, k) if tr else (Co, Ci, k, k), device=DEV) * 0.05
            y, _ = MC.conv_forward(xi, w, None, spec)
            gd.check()
            dy = torch.randn(y.shape, device=DEV).half().contiguous(memory_format=torch.channels_last)
            MC.conv_dgrad(dy, w, spec, tuple(xi.shape))
            MC.conv_wgrad(xi, dy, tuple(w.shape), spec)
            gd.check()
    trn, pcls, targets = _setup(128, 50.0, 2, 20000, torch.float16, seed=2)
    with guarded() as gd:
        assert np.isfinite(float(trn.step(pcls, targets)))
        gd.check()


def test_launching_entry_points_refuse_unknown_element_codes_with_real_buffers():
    """an element code outside 0..2 (InstanceNorm: outside 0..1), an unknown convolution mode or a misaligned loss-scale state returns
    LISO_EINVAL from the host side of the call, before any launch -- checked with valid device buffers of the right sizes"""
    L = _require_fp16()
    lib = L.lib()
    B, H, W, k, co, cap = 1, 64, 64, 3, 64, 256
    x = torch.zeros(B, H, W, 64, dtype=torch.float16, device=DEV)
    occ = torch.zeros(B, H, W, dtype=torch.float32, device=DEV)
    packed = torch.zeros(lib.liso_conv_packed_bytes(64, co, 9, L.CONV_F16), dtype=torch.uint8, device=DEV)
    y = torch.zeros(B, H // 2, W // 2, co, dtype=torch.float16, device=DEV)
    ws_bytes = lib.liso_sparse_conv_workspace_bytes(B, H, W, k, co, cap, 0)
    ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=DEV)
    flag = torch.zeros(4, dtype=torch.int32, device=DEV)
    st = L.stream_ptr()
    for code in (3, 7, -1):
        assert lib.liso_sparse_conv_forward(L.ptr(x), 64, code, L.ptr(occ), L.ptr(packed), None, B, H, W, k, co, cap, 0, L.ptr(y), None,
                                            None, L.ptr(flag), L.ptr(ws), ws_bytes, st) == -1
        assert lib.liso_sparse_conv_dgrad(L.ptr(y), co, code, L.ptr(occ), L.ptr(packed), B, H, W, k, co, cap, L.ptr(x), 64, L.ptr(flag),
                                          L.ptr(ws), ws_bytes, 0, st) == -1
    gamma = torch.ones(64, device=DEV)
    stats = torch.zeros(4 * 64, device=DEV)
    bn_ws = torch.zeros(lib.liso_in_workspace_bytes(1, 64), dtype=torch.uint8, device=DEV)
    assert lib.liso_in_relu_fwd(L.ptr(x), L.ELEM_F16, 1, H * W, 64, L.ptr(gamma), L.ptr(gamma), 1e-5, 1, L.ptr(x), L.ptr(stats),
                                L.ptr(bn_ws), bn_ws.numel(), st) == -1
    state = torch.zeros(16, dtype=torch.int32, device=DEV)
    g = torch.zeros(64, device=DEV)
    misaligned = ctypes.c_void_p(state.data_ptr() + 4)
    assert lib.liso_grad_nonfinite_f32(L.ptr(g), 64, misaligned, st) == -1
    assert lib.liso_loss_scale_update(misaligned, 2.0, 0.5, 10, st) == -1
    torch.cuda.synchronize()
    assert int(flag.sum()) == 0 and int(state.abs().sum()) == 0 and float(y.float().abs().sum()) == 0.0  # nothing ran
