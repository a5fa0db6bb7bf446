"""GPU: the weight-gradient slab reduction riding in the BatchNorm-backward finalize launch (liso_conv_wgrad_deferred +
liso_bn_relu_bwd_chained) against the separate launches (liso_conv_wgrad, liso_bn_relu_bwd).  Every block of the combined launch runs
the instructions of a block of the separate ones on the same data, so every comparison here is BITWISE: no tolerance anywhere."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

K_MAX_BLOCKS = 4096  # csrc/bn.hip: the dx coefficients sit behind kMaxBlocks x 2 x C partial sums in the BatchNorm workspace


def _bits(t):
    return t.detach().contiguous().reshape(-1).view(torch.uint8).cpu()


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _bn_stats(x, C):
    xf = x.float()
    mean, invstd = xf.mean(dim=(0, 2, 3)), (xf.var(dim=(0, 2, 3), unbiased=False) + 1e-3).rsqrt()
    gamma = torch.rand(C, device=x.device) + 0.5
    beta = torch.randn(C, device=x.device) * 0.1
    return gamma, torch.cat([gamma * invstd, beta - mean * gamma * invstd, mean, invstd]).contiguous()


def _bn_bwd(lib, L, g, x, gamma, stats, job):
    """liso_bn_relu_bwd (job None) / liso_bn_relu_bwd_chained on dense channels-last rows -> (dx, dgamma, dbeta, coef)"""
    B, C, H, W = x.shape
    xv, gv = x.permute(0, 2, 3, 1), g.permute(0, 2, 3, 1)
    assert xv.is_contiguous() and gv.is_contiguous()
    M = B * H * W
    nbytes = lib.liso_bn_workspace_bytes(C)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=x.device)
    dx = torch.empty_like(xv)
    gg, gb = torch.empty(C, device=x.device), torch.empty(C, device=x.device)
    code = L.elem_code(x.dtype)
    if job is None:
        L.check(lib.liso_bn_relu_bwd(L.ptr(gv), L.ptr(xv), code, M, C, L.ptr(gamma), L.ptr(stats), 1, 1, L.ptr(dx), L.ptr(gg), L.ptr(gb),
                                     L.ptr(ws), nbytes, L.stream_ptr()), "bn_relu_bwd")
    else:
        L.check(lib.liso_bn_relu_bwd_chained(L.ptr(gv), 0, L.ptr(xv), 0, code, M, C, L.ptr(gamma), L.ptr(stats), 1, 1, L.ptr(dx), 0, L.ptr(gg),
                                             L.ptr(gb), L.ptr(ws), nbytes, job.ride(), L.stream_ptr()), "bn_relu_bwd_chained")
    coef = ws.view(torch.float32)[K_MAX_BLOCKS * 2 * C:K_MAX_BLOCKS * 2 * C + 3 * C].clone()
    return dx, gg, gb, coef


# (ci, co, H = W of the input, stride, bias): the detector's 3x3 layer shapes + a small map (few splits)
LAYERS = [(64, 64, 256, 1, False), (128, 128, 128, 1, False), (256, 256, 64, 1, True), (64, 128, 256, 2, False), (64, 64, 16, 1, True),
          (128, 128, 32, 1, False)]


def test_combined_launch_equals_separate_launches_bitwise():
    """for every layer shape at B = 2 and B = 4: dw, dbias of the deferred route (slab kernel, then the reduction as blocks of the
    BatchNorm-backward finalize launch) and that launch's BatchNorm results (dgamma, dbeta, the three dx coefficients, dx) equal those
    of liso_conv_wgrad + liso_bn_relu_bwd bit for bit; the cases cover both instantiations of the reduction (> 16 and <= 16 splits)"""
    from liso_amd import _lib as L
    from liso_amd.utils import mfma_conv as MC

    lib = L.lib()
    dev = torch.device("cuda")
    seen = set()
    for B in (2, 4):
        for ci, co, hw, stride, bias in LAYERS:
            torch.manual_seed(ci + co + hw + B)
            spec = MC.ConvSpec(3, 3, stride=stride, padding=1)
            ho = (hw + 2 - 3) // stride + 1
            x = (torch.randn(B, hw, hw, ci, device=dev) * 0.5 + 0.1).to(torch.bfloat16).permute(0, 3, 1, 2)
            dy = torch.randn(B, ho, ho, co, device=dev).to(torch.bfloat16).permute(0, 3, 1, 2)
            g = torch.randn(B, hw, hw, ci, device=dev).to(torch.bfloat16).permute(0, 3, 1, 2)  # (stands for the data gradient)
            gamma, stats = _bn_stats(x, ci)
            sc, sh = stats[:ci], stats[ci:2 * ci]
            wshape = (co, ci, 3, 3)
            dw0, db0 = MC.conv_wgrad(x, dy, wshape, spec, sc, sh, in_relu=True, want_bias=bias)
            ref = _bn_bwd(lib, L, g, x, gamma, stats, None)
            dw1, db1, job = MC.conv_wgrad(x, dy, wshape, spec, sc, sh, in_relu=True, want_bias=bias, defer_reduce=True)
            assert job is not None and not job.done
            seen.add(job.job.splits > 16)
            got = _bn_bwd(lib, L, g, x, gamma, stats, job)
            torch.cuda.synchronize()
            tag = (B, ci, co, hw, stride, job.job.splits)
            assert _same(dw0, dw1), tag
            assert (db0 is None and db1 is None) or _same(db0, db1), tag
            for name, a, b in zip(("dx", "dgamma", "dbeta", "coef"), ref, got):
                assert _same(a, b), (tag, name)
            # and the plain reduction of a job (the route of every path without a finalize launch)
            dw2, db2, job2 = MC.conv_wgrad(x, dy, wshape, spec, sc, sh, in_relu=True, want_bias=bias, defer_reduce=True)
            job2.flush()
            assert _same(dw0, dw2) and ((db0 is None and db2 is None) or _same(db0, db2)), tag
    assert seen == {False, True}, f"the cases must cover the > 16 and the <= 16 splits reduction: {seen}"


def test_chained_entry_point_rejects_malformed_jobs():
    from liso_amd import _lib as L

    lib = L.lib()
    x = torch.zeros(1, 8, 8, 64, device="cuda", dtype=torch.bfloat16)
    f = torch.zeros(4 * 64, device="cuda")
    ws = torch.zeros(lib.liso_bn_workspace_bytes(64), dtype=torch.uint8, device="cuda")
    job = L.WgradReduceJob()  # all zero: no slab, no dw
    rc = lib.liso_bn_relu_bwd_chained(L.ptr(x), 0, L.ptr(x), 0, 1, 64, 64, L.ptr(f), L.ptr(f), 1, 1, L.ptr(x), 0, L.ptr(f), L.ptr(f), L.ptr(ws),
                                      ws.numel(), ctypes.byref(job), L.stream_ptr())
    assert rc != 0
    assert lib.liso_conv_wgrad_reduce(ctypes.byref(job), L.stream_ptr()) != 0
    assert lib.liso_conv_wgrad_reduce(None, L.stream_ptr()) != 0


def _layer(ci, co, groups, dev, bias=False, x_grad=True, param_grad=True, seed=0, hw=64, B=2):
    """a fused convolution behind a pending BatchNorm fold of `groups` channel groups -> (conv, x_raw, fold, dy)"""
    from liso_amd.utils import mfma_conv as MC

    torch.manual_seed(seed)
    conv = torch.nn.Conv2d(ci, co, 3, padding=1, bias=bias).to(dev)
    x_raw = (torch.randn(B, hw, hw, ci, device=dev) * 0.5 + 0.1).to(torch.bfloat16).permute(0, 3, 1, 2).requires_grad_(x_grad)
    fold = None
    if groups:
        grps, a = [], 0
        for C in groups:
            gamma, stats = _bn_stats(x_raw.detach()[:, a:a + C], C)
            beta = stats[C:2 * C] * 0  # (its value is inside `stats`; only the gradient matters here)
            grps.append({"stats": stats, "gamma": torch.nn.Parameter(gamma, requires_grad=param_grad),
                         "beta": torch.nn.Parameter(beta.clone(), requires_grad=param_grad)})
            a += C
        fold = MC.BnFold(grps, relu=True, training=True)
    dy = torch.randn(B, hw, hw, co, device=dev).to(torch.bfloat16).permute(0, 3, 1, 2)
    return conv, x_raw, fold, dy


def _backward_once(conv, x_raw, fold, dy):
    """-> [dw, dbias?, dx?, fold parameter gradients ...] of one _FusedConv backward"""
    from liso_amd.utils import mfma_conv as MC

    conv.weight.grad = None
    if conv.bias is not None:
        conv.bias.grad = None
    x_raw.grad = None
    for p in (fold.params() if fold is not None else []):
        p.grad = None
    y, _ = MC.fused_conv(x_raw, fold, conv)
    y.backward(dy)
    out = [conv.weight.grad.clone()]
    if conv.bias is not None:
        out.append(conv.bias.grad.clone())
    if x_raw.grad is not None:
        out.append(x_raw.grad.clone())
    out += [p.grad.clone() for p in (fold.params() if fold is not None else []) if p.grad is not None]
    return out


def _workspace_bytes(conv, x_raw, fold, dy):
    from liso_amd.utils import mfma_conv as MC

    sc, sh = fold.scale_shift()
    _, _, job = MC.conv_wgrad(x_raw.detach(), dy, tuple(conv.weight.shape), MC.ConvSpec.of(conv), sc, sh, in_relu=True, want_bias=False,
                              defer_reduce=True)
    n = job.ws.numel()
    job.flush()
    return n


def test_slabs_survive_until_they_are_reduced():
    """the deferred route keeps the workspace referenced until the launch that reduces it has been issued: with a free block of exactly
    the workspace's size waiting in the caching allocator (what the data gradient's output would otherwise be carved from), dw of the
    deferred route equals the plain route's"""
    from liso_amd.utils import mfma_conv as MC

    dev = torch.device("cuda")
    conv, x_raw, fold, dy = _layer(64, 64, [64], dev, hw=256)
    prev = MC.set_deferred_wgrad_reduce(False)
    try:
        ref = _backward_once(conv, x_raw, fold, dy)
        nbytes = _workspace_bytes(conv, x_raw, fold, dy)
        MC.set_deferred_wgrad_reduce(True)
        for _ in range(3):
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            t = torch.empty(nbytes, dtype=torch.uint8, device=dev)  # prime: one free block of exactly the workspace's size
            del t
            got = _backward_once(conv, x_raw, fold, dy)
            torch.cuda.synchronize()
            assert len(ref) == len(got) and all(_same(a, b) for a, b in zip(ref, got))
    finally:
        MC.set_deferred_wgrad_reduce(prev)


def test_slabs_survive_inside_a_captured_graph_replayed_twice():
    from liso_amd.utils import mfma_conv as MC

    dev = torch.device("cuda")
    conv, x_raw, fold, dy = _layer(64, 64, [64], dev, hw=256, seed=1)
    prev = MC.set_deferred_wgrad_reduce(False)
    try:
        ref = _backward_once(conv, x_raw, fold, dy)
        nbytes = _workspace_bytes(conv, x_raw, fold, dy)
        MC.set_deferred_wgrad_reduce(True)
        dw = torch.zeros_like(conv.weight)
        dx = torch.zeros_like(x_raw.detach())
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            _backward_once(conv, x_raw, fold, dy)  # warm-up off the capture
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            t = torch.empty(nbytes, dtype=torch.uint8, device=dev)  # (the graph's own pool: prime it the same way)
            del t
            got = _backward_once(conv, x_raw, fold, dy)
            dw.copy_(got[0])
            dx.copy_(got[1])
        for _ in range(2):
            dw.zero_()
            dx.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert _same(ref[0], dw) and _same(ref[1], dx)
    finally:
        MC.set_deferred_wgrad_reduce(prev)


@pytest.mark.parametrize("case", ["no_fold", "no_input_grad", "groups_cat", "groups_split", "bias", "single"])
def test_every_backward_path_yields_the_plain_paths_gradients(case):
    """`_FusedConv.backward` with the deferred reduction on == off, bit for bit, on every path: no fold (nothing to ride in), no input
    gradient wanted (no BatchNorm backward runs), several BatchNorm groups run as one call (<= 256 channels) and as one call per group
    (> 256 channels: the first group's finalize carries the reduction), a bias, and the plain single-fold layer"""
    from liso_amd.utils import mfma_conv as MC

    dev = torch.device("cuda")
    kw = {"no_fold": dict(ci=64, co=64, groups=None), "no_input_grad": dict(ci=64, co=64, groups=[64], x_grad=False, param_grad=False),
          "groups_cat": dict(ci=128, co=64, groups=[64, 64]), "groups_split": dict(ci=384, co=64, groups=[128, 128, 128]),
          "bias": dict(ci=64, co=128, groups=[64], bias=True), "single": dict(ci=128, co=128, groups=[128])}[case]
    conv, x_raw, fold, dy = _layer(dev=dev, seed=5, **kw)
    prev = MC.set_deferred_wgrad_reduce(False)
    try:
        ref = _backward_once(conv, x_raw, fold, dy)
        MC.set_deferred_wgrad_reduce(True)
        got = _backward_once(conv, x_raw, fold, dy)
        torch.cuda.synchronize()
    finally:
        MC.set_deferred_wgrad_reduce(prev)
    assert len(ref) == len(got)
    for i, (a, b) in enumerate(zip(ref, got)):
        assert _same(a, b), (case, i)


@pytest.mark.parametrize("use_graph", [False, True])
def test_detector_train_steps_are_bit_identical_with_and_without_the_fusion(use_graph):
    """DetectorTrainer, B = 2, bf16, three steps: losses and every parameter / buffer after the steps, deferred reduction on vs off"""
    from liso_amd.datasets.synthetic import detector_batch
    from liso_amd.trainer import DetectorTrainer
    from liso_amd.utils import mfma_conv as MC
    from liso_amd.utils.config import default_cfg

    dev = torch.device("cuda")
    pcls, targets = detector_batch(3, 2, dev, n_points=60000, grid=512, bev_range_m=100.0)
    runs = []
    prev = MC.set_deferred_wgrad_reduce(True)
    try:
        for on in (False, True):
            MC.set_deferred_wgrad_reduce(on)
            torch.manual_seed(0)
            tr = DetectorTrainer(default_cfg(grid=512, bev_range_m=100.0), dev, compute_dtype=torch.bfloat16, total_steps=8, use_graph=use_graph)
            losses = [_bits(tr.step(pcls, targets)) for _ in range(3)]
            torch.cuda.synchronize()
            runs.append((losses, {k: _bits(v) for k, v in tr.net.state_dict().items()}))
    finally:
        MC.set_deferred_wgrad_reduce(prev)
    assert all(torch.equal(a, b) for a, b in zip(runs[0][0], runs[1][0]))
    assert runs[0][1].keys() == runs[1][1].keys()
    for k in runs[0][1]:
        assert torch.equal(runs[0][1][k], runs[1][1][k]), k


def test_liso_loop_steps_are_bit_identical_with_and_without_the_fusion():
    """LisoLoopTrainer as the benchmark launches it (hipGraphs + pipeline), three steps: losses, mined boxes and the detector's state"""
    from liso_amd.datasets.synthetic import slim_pair
    from liso_amd.trainer import LisoLoopTrainer
    from liso_amd.utils import mfma_conv as MC
    from liso_amd.utils.config import apply_slim_simple_knn_training, default_cfg

    dev = torch.device("cuda")
    pairs = [slim_pair(40 + i, dev, n_points=20000, grid=256, bev_range_m=50.0) for i in range(3)]
    runs = []
    prev = MC.set_deferred_wgrad_reduce(True)
    try:
        for on in (False, True):
            MC.set_deferred_wgrad_reduce(on)
            torch.manual_seed(0)
            tr = LisoLoopTrainer(apply_slim_simple_knn_training(default_cfg(grid=256, bev_range_m=50.0)), dev, compute_dtype=torch.bfloat16,
                                 total_steps=10, use_graph=True, overlap=True)
            losses = [_bits(tr.step(*pairs[i % 3], upcoming=(pairs[(i + 1) % 3], pairs[(i + 2) % 3]))) for i in range(3)]
            torch.cuda.synchronize()
            runs.append((losses, int(tr.last_boxes.valid.sum()), {k: _bits(v) for k, v in tr.detector.net.state_dict().items()}))
    finally:
        MC.set_deferred_wgrad_reduce(prev)
    assert all(torch.equal(a, b) for a, b in zip(runs[0][0], runs[1][0]))
    assert runs[0][1] == runs[1][1]
    for k in runs[0][2]:
        assert torch.equal(runs[0][2][k], runs[1][2][k]), k
