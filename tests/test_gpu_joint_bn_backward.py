"""GPU: the joint BatchNorm backward of the detector step (mfma_conv.shared_fold, the grouped call of the deblocks' concatenation,
the merged statistics buffers) against the per-consumer, per-group form it replaces (mfma_conv.set_joint_bn_backward(False)).  The
joint form computes every sum in the order of the separate calls and adds two gradients as autograd's add does, so every comparison here
is BITWISE.  The network is the detector on a 64 x 64 grid, B = 2: three RPN blocks, three deblocks, the CenterHead."""
import pytest
import torch

pytestmark = pytest.mark.gpu

GRID, RANGE_M = 64, 40.0


def _bits(t):
    return t.detach().contiguous().reshape(-1).view(torch.uint8).cpu()


def _trainer(dtype, **kw):
    from liso_amd.trainer import DetectorTrainer
    from liso_amd.utils.config import default_cfg

    torch.manual_seed(0)
    return DetectorTrainer(default_cfg(grid=GRID, bev_range_m=RANGE_M), torch.device("cuda"), compute_dtype=dtype, total_steps=8, **kw)


def _batch():
    from liso_amd.datasets.synthetic import detector_batch

    return detector_batch(3, 2, torch.device("cuda"), n_points=8000, grid=GRID, bev_range_m=RANGE_M)


def _eager_pass(tr, pcls, targets, cut=False):
    """forward + loss + backward on a leaf canvas, eager launches -> (bits of the loss, of every parameter gradient and of the canvas
    gradient, number of BatchNorm-backward entry calls)"""
    from liso_amd import _lib as L
    from liso_amd.utils import mfma_conv as MC

    tr.model.train()
    for p in tr.net.parameters():
        p.grad = None
    with torch.no_grad():
        bev, occ = tr._pillars(pcls)
    bev = bev.detach().clone().requires_grad_(True)
    rpn = tr.net.model.rpn
    gc = MC.GradCut() if cut else None
    L.TIMER.reset()
    L.TIMER.enable("bn_bwd")
    try:
        rpn.grad_cut = gc
        try:
            total, _, _ = tr.loss(None, targets, canvas=(bev, occ.detach().clone()))
        finally:
            rpn.grad_cut = None
        total.backward()
        if gc is not None:
            gc.finish()
        torch.cuda.synchronize()
        calls = len(L.TIMER.events.get("bn_bwd", []))
    finally:
        L.TIMER.disable_all()
        L.TIMER.reset()
    grads = {k: _bits(p.grad) for k, p in tr.net.named_parameters() if p.grad is not None}
    return _bits(total), grads, _bits(bev.grad), calls


def _compare_eager(dtype, cut, calls_off, calls_on):
    from liso_amd.utils import mfma_conv as MC

    pcls, targets = _batch()
    runs = []
    prev = MC.set_joint_bn_backward(True)
    try:
        for on in (False, True):
            MC.set_joint_bn_backward(on)
            runs.append(_eager_pass(_trainer(dtype), pcls, targets, cut))
    finally:
        MC.set_joint_bn_backward(prev)
    (l0, g0, x0, c0), (l1, g1, x1, c1) = runs
    print(f"bn_bwd entry calls per step ({dtype}, grad_cut {cut}): {c0} -> {c1}")
    assert torch.equal(l0, l1), "loss"
    assert g0.keys() == g1.keys() and len(g0) > 0
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k
    assert torch.equal(x0, x1), "input gradient"
    assert (c0, c1) == (calls_off, calls_on)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_eager_step_is_bit_identical_and_runs_four_backward_calls_less(dtype):
    """loss, every parameter gradient and the input gradient, joint backward on vs off; the BatchNorm-backward entry calls (L.TIMER's
    `bn_bwd` events) drop from 23 to 19: one call instead of two at the outputs of blocks 0 and 1, one instead of three on the
    deblocks' 384-channel concatenation"""
    _compare_eager(dtype, False, 23, 19)


def test_grad_cut_keeps_the_per_consumer_backward_at_block_0():
    """with the backward pass cut behind block 0 (multi-rank trainers) that block's output keeps one backward per consumer -- its two
    gradients meet in the leaf, not in a node of this graph: 23 -> 20 calls, same bits"""
    _compare_eager(torch.bfloat16, True, 23, 20)


@pytest.mark.parametrize("buckets", [None, 2], ids=["one_graph", "grad_cut_two_graphs"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_captured_steps_are_bit_identical(dtype, buckets):
    """DetectorTrainer(use_graph=True) -- the trainer's capture helper, direct gradient writes into the flat buffer -- two steps:
    losses, the captured canvas gradient and every parameter / buffer after the steps, joint backward on vs off"""
    from liso_amd.utils import mfma_conv as MC

    pcls, targets = _batch()
    runs = []
    prev = MC.set_joint_bn_backward(True)
    try:
        for on in (False, True):
            MC.set_joint_bn_backward(on)
            tr = _trainer(dtype, use_graph=True, grad_buckets=buckets)
            losses = [_bits(tr.step(pcls, targets)) for _ in range(2)]
            torch.cuda.synchronize()
            runs.append((losses, _bits(tr._static_bev.grad), {k: _bits(v) for k, v in tr.net.state_dict().items()}))
    finally:
        MC.set_joint_bn_backward(prev)
    assert all(torch.equal(a, b) for a, b in zip(runs[0][0], runs[1][0])), "losses"
    assert torch.equal(runs[0][1], runs[1][1]), "input gradient"
    assert runs[0][2].keys() == runs[1][2].keys()
    for k in runs[0][2]:
        assert torch.equal(runs[0][2][k], runs[1][2][k]), k
