"""DetectorTrainer(use_graph=True) on panels and merged filters that the AdamW launch writes (liso_amd/utils/optimizer_packs.py,
include/liso_optim.h: liso_adamw_step_packed_f32) against the same trainer with mfma_conv.set_optimizer_packs(False), where every
captured step packs and merges for itself: losses and the whole state_dict (network and optimizer) bit for bit."""
import pytest
import torch

pytestmark = pytest.mark.gpu

GRID, RANGE_M = 64, 40.0


def _batch(dev):
    from liso_amd.datasets.synthetic import detector_batch

    return detector_batch(21, 2, dev, n_points=2000, grid=GRID, bev_range_m=RANGE_M)


def _run(dev, dtype, packs_on, batch, between=None, **kw):
    """four graph steps -> (losses, network state, optimizer state, the trainer's OptimizerPacks | None)"""
    from liso_amd.trainer import DetectorTrainer
    from liso_amd.utils import mfma_conv as MC
    from liso_amd.utils.config import default_cfg

    was = MC.set_optimizer_packs(packs_on)
    try:
        torch.manual_seed(3)
        tr = DetectorTrainer(default_cfg(grid=GRID, bev_range_m=RANGE_M), dev, compute_dtype=dtype, total_steps=12, use_graph=True, **kw)
        pcls, targets = batch
        losses = []
        for i in range(4):
            if i == 2 and between is not None:
                between(tr)
            losses.append(float(tr.step(pcls, targets)))
        torch.cuda.synchronize()
        net = {k: v.detach().cpu().clone() for k, v in tr.net.state_dict().items()}
        opt = tr.optimizer.state_dict()["state"]
        opt = {(i, k): (v.detach().cpu().clone() if torch.is_tensor(v) else v) for i, st in opt.items() for k, v in st.items()}
        return losses, net, opt, tr._opt_packs
    finally:
        MC.set_optimizer_packs(was)


def _assert_same(a, b):
    assert a[0] == b[0], (a[0], b[0])
    assert a[1].keys() == b[1].keys() and a[2].keys() == b[2].keys()
    for k in a[1]:
        assert torch.equal(a[1][k].view(torch.uint8) if a[1][k].is_floating_point() else a[1][k],
                           b[1][k].view(torch.uint8) if b[1][k].is_floating_point() else b[1][k]), k
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]) if torch.is_tensor(a[2][k]) else a[2][k] == b[2][k], k


def _edit_a_filter(tr):
    with torch.no_grad():  # (a block-1 filter with panels of its own, and a head filter that lives in a merged panel)
        next(tr.net.model.rpn.blocks[1].parameters()).mul_(1.25)
        seq = list(getattr(tr.net.model.center_head.tasks[0], next(iter(tr.net.model.center_head.tasks[0].heads))))
        seq[0].weight.add_(0.01)
        seq[3].bias.add_(0.5)


def _state_dict_round_trip(tr):
    net = {k: v.detach().clone() for k, v in tr.net.state_dict().items()}
    opt = tr.optimizer.state_dict()
    with torch.no_grad():
        for p in tr.net.parameters():
            p.zero_()
    tr.net.load_state_dict(net)
    tr.optimizer.load_state_dict(opt)


CASES = {"plain": {}, "two_buckets": {"grad_buckets": 2}, "in_place_edit": {"between": _edit_a_filter},
         "load_state_dict": {"between": _state_dict_round_trip}}


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_steps_on_optimizer_packs_equal_steps_that_pack_for_themselves(dtype, case):
    dev = torch.device("cuda:0")
    batch = _batch(dev)
    on = _run(dev, dtype, True, batch, **CASES[case])
    off = _run(dev, dtype, False, batch, **CASES[case])
    assert off[3] is None
    packs = on[3]
    # the table took over: every filter of the backbone and the head, both merged head convolutions, nothing left to pack in the graph
    assert packs is not None and packs.n_items > 20 and len(packs.merged) == 2 and not packs.leftover_jobs
    # the first replay finds the panels older than the restored warm-up state; afterwards only the edits between steps repack
    assert packs.repacks == (3 if CASES[case].get("between") else 2), packs.repacks
    _assert_same(on, off)
