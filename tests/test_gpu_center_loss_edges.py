"""The fused CenterPoint decode + loss kernels (liso_amd/csrc/detector_loss.hip: centerloss_partial / _final / _bwd) against
tests/center_loss_cases.py:loss_fp64 at the launch shapes, mask branches and saturated values the whole-step tests never reach.

Bounds (set before any run): every loss term and the total within 1e-5 * max(|ref|, 1e-3); every gradient, per head and per cell class
(selected centre / non-ignored non-centre / ignored), max |got - ref| <= 1e-5 * max |ref| over the class, and == 0 where the reference
is identically zero over a class.  An fp32 torch restatement on the CPU stays below 7e-7 per class.

Worst values observed on an MI355X over every case, layout and upstream gradient (bound 1e-5 each):
  loss terms, |got - ref| / max(|ref|, 1e-3):  probs 4.9e-8, rot 4.7e-8, dims 6.1e-8, pos 1.4e-7, reg 4.1e-8, total 5.3e-8
  gradients, max |got - ref| / max |ref| per class:
    pos    selected 1.4e-7                        (background, ignored: exact zeros)
    dims   selected 1.5e-7                        (background, ignored: exact zeros)
    rot    selected 1.4e-7, background 1.4e-7, ignored 1.0e-7
    probs  selected 2.7e-7, background 4.1e-7     (ignored: exact zeros)
  reference fixture through the kernel: losses <= 9.1e-8 (bound 1e-5); gradients pos 9.4e-8, dims 1.0e-7, rot 0, probs 2.4e-7 (bound 1e-4)

What each case is there to catch (checked once against deliberately wrong builds of the kernels, never committed): the backward's own
`max(sum w, 1)` -> M4 and M5; res_x and res_y swapped in the decode -> every geometry with res_x != res_y ((2, 48, 80) has
60 / 48 == 100 / 80 and cannot tell); a grid stride one short in the partial kernel -> every case of at least one full block, through
the forced centres at cell 0, the last cell and cell 512 * 256 - 1; (1 - gt)^2 for (1 - gt)^4 in the forward only -> every case with a
background cell.  n_blocks() caps the grid at 512 blocks and liso_centerloss_workspace_bytes() sizes the partial rows by the same
function, so the cap cannot outgrow the workspace without both changing -- read, not run."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import center_loss_cases as C

pytestmark = pytest.mark.gpu

KEY = "loss/supervised/centermaps/"
CASE_IDS = list(C.loss_cases())


@functools.lru_cache(maxsize=None)
def _case(cid):
    case = C.loss_case(**C.loss_cases()[cid])
    return case, C.loss_reference(case)


def _layout(t, how):
    """the same values as a logical [B,H,W,C] device tensor in another memory layout"""
    t = t.cuda()
    if how == "nchw":
        return t.permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1)
    return t.contiguous()


def _run(case, upstream=1.0, layout="contiguous"):
    """-> terms {name: float32 scalar on the host}, grads {head: [B,H,W,C] cpu, contiguous}, strides seen (input, gradient)"""
    from liso_amd.losses.fused_centerpoint import fused_centerpoint_loss

    dev = torch.device("cuda:0")
    if layout == "packed":  # the four maps as channel ranges of one [B,H,W,16] buffer
        B, H, W = case["geometry"]
        buf = torch.zeros(B, H, W, 16, device=dev)
        raw = {}
        for k, lo in (("pos", 0), ("dims", 4), ("rot", 8), ("probs", 12)):
            c = case["raw"][k].shape[-1]
            buf[..., lo:lo + c] = case["raw"][k].cuda()
            raw[k] = buf[..., lo:lo + c].detach().requires_grad_(True)
    else:
        raw = {k: _layout(case["raw"][k], layout).detach().requires_grad_(True) for k in C.HEADS}
    total, losses = fused_centerpoint_loss(
        cfg=C.case_cfg(case), raw_box_maps=raw, gt_maps={k: v.cuda() for k, v in case["gt"].items()},
        gt_center_mask=case["center_mask"].cuda(), ignore_region_is_true_mask=None if case["ignore"] is None else case["ignore"].cuda(),
        rotation_loss_weights_map=None if case["rot_w"] is None else case["rot_w"][..., None].cuda(),
        pillar_center_coors_m=case["centers"].cuda())
    grads = torch.autograd.grad(total, [raw[k] for k in C.HEADS], grad_outputs=torch.tensor(upstream, device=dev))
    strides = {k: (raw[k].stride(), g.stride()) for k, g in zip(C.HEADS, grads)}
    terms = {k: losses[KEY + k].cpu() for k in C.HEADS}
    terms.update(reg=losses["loss/regularization/rot_vec_on_unit_circle"].cpu(), total=total.detach().cpu())
    return terms, {k: g.contiguous().cpu() for k, g in zip(C.HEADS, grads)}, strides


def _check_against_reference(case, ref_terms, ref_grads, terms, grads, tag):
    for k in C.TERMS:
        got, ref = float(terms[k]), ref_terms[k]
        print(f"{tag} term {k}: got {got:.9g} ref {ref:.9g} err/scale {abs(got - ref) / max(abs(ref), 1e-3):.2e}")
    classes = C.cell_classes(case)
    errs = {h: C.class_errors(grads[h], ref_grads[h], classes) for h in C.HEADS}
    for h in C.HEADS:
        for cls, (err, ref) in errs[h].items():
            print(f"{tag} grad {h} / {cls}: max err {err:.3e} max ref {ref:.3e} ratio {err / ref if ref else 0.0:.2e}")
    for k in C.TERMS:
        assert np.isfinite(float(terms[k])), (tag, k)
        assert abs(float(terms[k]) - ref_terms[k]) <= 1e-5 * max(abs(ref_terms[k]), 1e-3), (tag, k, float(terms[k]), ref_terms[k])
    for h in C.HEADS:
        assert bool(torch.isfinite(grads[h]).all()), (tag, h)
        for cls, (err, ref) in errs[h].items():
            if ref == 0.0:
                assert bool((grads[h][classes[cls]] == 0).all()), (tag, h, cls)
            else:
                assert err <= 1e-5 * ref, (tag, h, cls, err, ref)


@pytest.mark.parametrize("cid", CASE_IDS)
def test_loss_and_gradients_match_fp64_per_term_and_per_cell_class(cid):
    case, (ref_terms, ref_grads) = _case(cid)
    terms, grads, strides = _run(case)
    _check_against_reference(case, ref_terms, ref_grads, terms, grads, cid)
    classes = C.cell_classes(case)
    sel = classes["selected"]
    if not bool(sel.any()):  # M2, M3, M6: no supervised L1 term at all, and only the regulariser reaches the rotation map
        for k in ("rot", "dims", "pos"):
            assert float(terms[k]) == 0.0, (k, float(terms[k]))
        assert bool((grads["pos"] == 0).all()) and bool((grads["dims"] == 0).all())
        only_reg = dict(case, sup_weight=0.0)
        _, reg_grads = C.loss_reference(only_reg)
        for cls, (err, ref) in C.class_errors(grads["rot"], reg_grads["rot"], classes).items():
            assert err <= 1e-5 * ref, ("rot carries more than the regulariser", cls, err, ref)
    if case["mask"] == "M6":
        assert float(terms["probs"]) == 0.0 and bool((grads["probs"] == 0).all())
    # off the selected cells pos and dims get exact zeros, ignored cells no probs gradient, and without the regulariser no rot either
    assert bool((grads["pos"][~sel] == 0).all()) and bool((grads["dims"][~sel] == 0).all())
    assert bool((grads["probs"][classes["ignored"]] == 0).all())
    if case["reg_weight"] == 0.0:
        assert bool((grads["rot"][~sel] == 0).all())
    for k, (s_in, s_grad) in strides.items():
        assert s_in == s_grad, (k, s_in, s_grad)


def test_two_calls_are_bit_identical():
    case, _ = _case("M1-1x129x129")
    a, b = _run(case), _run(case)
    for k in C.TERMS:
        assert torch.equal(a[0][k], b[0][k]), k
    for h in C.HEADS:
        assert torch.equal(a[1][h], b[1][h]), h


def test_memory_layouts_give_bit_identical_losses_and_gradients():
    """the arithmetic and the reduction order go by cell index, not by address: contiguous [B,H,W,C], NCHW storage viewed as [B,H,W,C],
    and the four maps as channel ranges of one [B,H,W,16] buffer; each gradient comes back with its input's strides"""
    case, (ref_terms, ref_grads) = _case("M1-2x48x80")
    runs = {how: _run(case, layout=how) for how in ("contiguous", "nchw", "packed")}
    B, H, W = case["geometry"]
    assert runs["nchw"][2]["pos"][0] == (3 * H * W, W, 1, H * W) and runs["packed"][2]["rot"][0] == (16 * H * W, 16 * W, 16, 1)
    for how, (terms, grads, strides) in runs.items():
        _check_against_reference(case, ref_terms, ref_grads, terms, grads, how)
        for k, (s_in, s_grad) in strides.items():
            assert s_in == s_grad, (how, k, s_in, s_grad)
        for k in C.TERMS:
            assert torch.equal(terms[k], runs["contiguous"][0][k]), (how, k)
        for h in C.HEADS:
            assert torch.equal(grads[h], runs["contiguous"][1][h]), (how, h)


def test_upstream_gradient_scales_the_backward_exactly():
    case, _ = _case("M1-3x5x7")
    one = _run(case, 1.0)[1]
    for s in (-1.0, 1.7, 65536.0):
        ref_terms, ref_grads = C.loss_reference(case, upstream=s)
        terms, grads, _ = _run(case, s)
        _check_against_reference(case, ref_terms, ref_grads, terms, grads, f"upstream {s}")
        if s == -1.0:
            for h in C.HEADS:
                assert torch.equal(grads[h], -one[h]), h
        if s == 65536.0:  # a power of two: no rounding anywhere changes
            for h in C.HEADS:
                assert torch.equal(grads[h], 65536.0 * one[h]), h


def test_reference_fixture_through_the_kernel(golden_dir):
    """tests/golden/detector_decode_loss.npz (16 x 16 at range 40, z prior -1.5 / -0.5, weights 1 and 0, rotation weights absent): the
    reference project's own four losses at 1e-5 and four raw-map gradients at 1e-4, the bounds of the CPU test of the same fixture"""
    from liso_amd.losses.fused_centerpoint import fused_centerpoint_loss
    from liso_amd.utils.config import default_cfg

    g = np.load(os.path.join(golden_dir, "detector_decode_loss.npz"))
    cfg = default_cfg(grid=64, bev_range_m=40.0)
    cfg.loss.supervised.supervised_on_clusters.weight = 1.0
    cfg.box_prediction.rotation_representation.regul_weight = 0.0
    raw = {k: torch.from_numpy(g["raw_" + k]).cuda().requires_grad_(True) for k in C.HEADS}
    total, losses = fused_centerpoint_loss(
        cfg=cfg, raw_box_maps=raw, gt_maps={k: torch.from_numpy(g["gt_" + k]).cuda() for k in C.HEADS},
        gt_center_mask=torch.from_numpy(g["center_mask"]).cuda(), ignore_region_is_true_mask=torch.from_numpy(g["ignore"]).cuda(),
        pillar_center_coors_m=torch.from_numpy(g["centers"]).cuda())
    grads = torch.autograd.grad(total, [raw[k] for k in C.HEADS])
    for k in C.HEADS:
        want = float(g["loss_" + k])
        print(f"fixture loss {k}: err {abs(float(losses[KEY + k]) - want) / abs(want):.2e}")
        assert abs(float(losses[KEY + k]) - want) <= 1e-5 * abs(want), (k, float(losses[KEY + k]), want)
    assert abs(float(total.detach()) - sum(float(g["loss_" + k]) for k in C.HEADS)) <= 1e-5 * abs(float(total.detach()))
    for k, got in zip(C.HEADS, grads):
        want = g["grad_" + k]
        err = np.abs(got.cpu().numpy() - want).max() / np.abs(want).max()
        print(f"fixture grad {k}: err {err:.2e}")
        assert err <= 1e-4, (k, err)
