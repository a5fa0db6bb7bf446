"""CPU anchors of tests/center_loss_cases.py: loss_fp64 against the project's torch-op path in fp64 and the reference project's loss
fixture, targets_fp64 against the torch formulation in fp64 and the reference's target fixture, and the conditions on the cases
themselves (kink margin, coverage of the classes, the cap on excluded cells) -- all without a GPU or a project kernel."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import center_loss_cases as C

KEY = "loss/supervised/centermaps/"
LOSS_IDS = list(C.loss_cases())
TARGET_IDS = list(C.target_cases())


@functools.lru_cache(maxsize=None)
def _loss_case(cid):
    return C.loss_case(**C.loss_cases()[cid])


@functools.lru_cache(maxsize=None)
def _target_ref(cid):
    c = C.target_cases()[cid]
    return c, C.targets_fp64(c["pos"], c["dims"], c["rot"], c["valid"], c["grid"], c["range"])


def _torch_op_path(case):
    from liso_amd.kabsch.output_modification import output_modification
    from liso_amd.losses.centerpoint_loss import centerpoint_loss, rotation_vec_on_unit_circle
    from liso_amd.networks.simple_net.simple_net_utils import allowed_activations

    cfg = C.case_cfg(case)
    raw = {k: case["raw"][k].double().requires_grad_(True) for k in C.HEADS}
    act = {k: allowed_activations[cfg.box_prediction.activations[k]](v) for k, v in raw.items()}
    dec = output_modification({k: v.clone() for k, v in act.items()}, cfg.box_prediction, cfg.data, "boxes", case["centers"].double())
    cen = case["center_mask"]
    ign = torch.zeros_like(cen) if case["ignore"] is None else case["ignore"]
    rot_w = torch.ones(cen.shape, dtype=torch.float64) if case["rot_w"] is None else case["rot_w"].double()
    losses = centerpoint_loss(loss_cfg=cfg.loss, raw_activated_pred_box_maps=act, decoded_pred_box_maps=dec,
                              gt_maps={k: v.double() for k, v in case["gt"].items()}, gt_center_mask=cen,
                              rotation_loss_weights_map=rot_w[..., None], box_prediction_cfg=cfg.box_prediction,
                              ignore_region_is_true_mask=ign)
    reg = rotation_vec_on_unit_circle(act)
    total = sum(losses.values()) * case["sup_weight"] + reg * case["reg_weight"]
    grads = torch.autograd.grad(total, [raw[k] for k in C.HEADS])
    terms = {k: float(losses[KEY + k].detach()) for k in C.HEADS}
    terms.update(reg=float(reg.detach()), total=float(total.detach()))
    return terms, dict(zip(C.HEADS, grads))


@pytest.mark.parametrize("cid", LOSS_IDS)
def test_loss_fp64_equals_the_torch_op_path_in_fp64(cid):
    case = _loss_case(cid)
    terms, grads = C.loss_reference(case)
    want_terms, want_grads = _torch_op_path(case)
    for k in C.TERMS:
        assert abs(terms[k] - want_terms[k]) <= 1e-12 * abs(want_terms[k]), (k, terms[k], want_terms[k])
    classes = C.cell_classes(case)
    for h in C.HEADS:
        for cls, (err, ref) in C.class_errors(grads[h], want_grads[h], classes).items():
            assert err <= 1e-12 * ref, (h, cls, err, ref)


@pytest.mark.parametrize("cid", LOSS_IDS)
def test_loss_cases_hold_their_conditions(cid):
    case = _loss_case(cid)
    B, H, W = case["geometry"]
    n = B * H * W
    cls = C.cell_classes(case)
    cen, mask = case["center_mask"], case["mask"]
    assert C.kink_margin(case) >= C.KINK_MARGIN
    assert (case["res"][0] != case["res"][1]) == (case["geometry"] not in ((1, 16, 16), (1, 129, 129), C.MAIN))  # (60 / 48 == 100 / 80)
    if mask in ("M0", "M1") and not case["edges"]:
        forced = [0, n - 1] + ([C.SECOND_TRIP_CELL] if n > C.SECOND_TRIP_CELL + 1 else [])
        assert all(bool(cls["selected"].reshape(-1)[i]) for i in forced)
        first = case["raw"]["pos"].reshape(n, 3)[0]
        assert float(first.abs().max()) <= 1.0
    if mask == "M1":
        assert int((cen & cls["ignored"]).sum()) >= 1 and int(cls["selected"].sum()) >= 2 and int((~cen & cls["ignored"]).sum()) >= 1
        assert float(case["rot_w"].min()) < 0.1 and float(case["rot_w"].max()) > 1.9 or n < 200
    want = {"M2": (0, 0), "M4": (3, 3), "M5": (1, 1)}.get(mask)
    if want:
        assert (int(cen.sum()), int(cls["selected"].sum())) == want
    if mask == "M3":
        assert int(cen.sum()) > 0 and int(cls["selected"].sum()) == 0 and int(cls["background"].sum()) > 0
    if mask == "M4":
        assert float(case["rot_w"][cen].abs().max()) == 0.0
    if mask == "M6":
        assert bool(case["ignore"].all()) and int(cen.sum()) > 0
    if case["edges"]:
        raw, gt = case["raw"], case["gt"]
        for name, m in cls.items():  # every planted value in every class
            for v in C.EDGE_LOGITS[:-1]:
                assert bool((raw["probs"][..., 0][m] == v).any()), (name, v)
            for v in C.EDGE_DIMS[:-1]:
                assert bool((raw["dims"][m] == v).any()), (name, v)
            for v in C.EDGE_POS[:-1]:
                assert bool((raw["pos"][m] == v).any()), (name, v)
            assert bool((raw["rot"][m] == 0).all(-1).any()) and bool((raw["rot"][m] == gt["rot"][m]).all(-1).any()), name
            assert bool((cen[m]).any()) == (name != "background")
        bg = gt["probs"][..., 0][~cen]
        assert bool((bg == 1.0).any()) and bool((bg == 0.0).any())


def test_loss_fp64_reproduces_the_reference_fixture(golden_dir):
    """tests/golden/detector_decode_loss.npz: the reference project's own decoded maps, four losses and four raw-map gradients, at the
    tolerances of tests/test_detector_cpu.py"""
    g = np.load(os.path.join(golden_dir, "detector_decode_loss.npz"))
    raw = {k: torch.from_numpy(g["raw_" + k]).double().requires_grad_(True) for k in C.HEADS}
    gt = {k: torch.from_numpy(g["gt_" + k]) for k in C.HEADS}
    out = C.loss_fp64(raw, gt, torch.from_numpy(g["center_mask"]), torch.from_numpy(g["ignore"]), None, torch.from_numpy(g["centers"]),
                      (40.0 / 16, 40.0 / 16), (-1.5, -0.5), 1.0, 0.0)
    for k in ("pos", "dims"):
        want = g["dec_" + k]
        assert np.abs(out["dec"][k].detach().numpy() - want).max() <= 1e-5 * np.abs(want).max(), k
    for k in C.HEADS:
        assert abs(float(out[k].detach()) - float(g["loss_" + k])) <= 1e-5 * abs(float(g["loss_" + k])), k
    grads = torch.autograd.grad(out["total"], [raw[k] for k in C.HEADS])
    for k, got in zip(C.HEADS, grads):
        want = g["grad_" + k]
        assert np.abs(got.numpy() - want).max() <= 1e-4 * np.abs(want).max(), k


@pytest.mark.parametrize("cid", [c for c in TARGET_IDS if c not in ("pad-zero", "pad-nan", "k0")])
def test_targets_fp64_equals_the_torch_formulation_in_fp64(cid):
    """(K = 0: the torch formulation cannot reduce over an empty axis; zero / NaN padding: it multiplies by the validity flag)"""
    from liso_amd.datasets.targets import render_center_targets_torch

    c, ref = _target_ref(cid)
    got = render_center_targets_torch(c["pos"].double(), c["dims"].double(), c["rot"].double(), c["valid"], c["grid"], c["range"])
    assert float((got["probs"] - ref["probs"]).abs().max()) <= 1e-12
    flagged = ref["winner_uncertain"] | ref["threshold_uncertain"]
    for k in ("dims", "pos", "rot"):
        assert float((got[k] - ref[k]).abs()[~flagged].max()) <= 1e-12 * max(float(ref[k].abs().max()), 1.0), k
    assert torch.equal(got["center_bool_mask"], ref["center_bool_mask"])


def test_targets_fp64_reproduces_the_reference_fixture(golden_dir):
    g = np.load(os.path.join(golden_dir, "targets_reference.npz"))
    for tag in ("a", "b", "c"):
        G, R = int(g[f"{tag}_grid_range"][0]), float(g[f"{tag}_grid_range"][1])
        pos, dims, rot = (torch.from_numpy(g[f"{tag}_box_{k}"]).float()[None] for k in ("pos", "dims", "rot"))
        ref = C.targets_fp64(pos, dims, rot, torch.ones(pos.shape[:2], dtype=torch.bool), (G, G), (R, R))
        for k in ("probs", "dims", "pos", "rot"):
            want = g[f"{tag}_{k}"]
            assert np.abs(ref[k][0].numpy() - want).max() <= 1e-4 * max(np.abs(want).max(), 1.0), (tag, k)
        assert np.array_equal(ref["center_bool_mask"][0].numpy(), g[f"{tag}_center_bool_mask"]), tag


@pytest.mark.parametrize("cid", TARGET_IDS)
def test_at_most_two_cells_of_a_target_case_are_excluded(cid):
    """the exclusion cap: a condition on the cases, met by the reference alone"""
    _, ref = _target_ref(cid)
    assert C.uncertain_count(ref) <= 2, (int(ref["winner_uncertain"].sum()), int(ref["threshold_uncertain"].sum()))


def test_target_cases_hold_their_conditions():
    cases = C.target_cases()
    for cid in ("border-64x64", "border-64x32"):
        c, ref = _target_ref(cid)
        assert torch.equal(ref["center_bool_mask"], C.border_expectation(c)), cid
        assert int(ref["center_bool_mask"].sum()) == 8
    c, ref = _target_ref("odd-33x57")
    assert float(C.cell_axis(33, 50.0)[16]) == 0.0 and float(C.cell_axis(57, 80.0)[28]) == 0.0
    assert not bool(c["valid"].all()) and bool(c["valid"].any(1).all())
    for cid in ("pad-zero", "pad-nan"):
        _, pad = _target_ref(cid)
        for k in ("probs", "dims", "pos", "rot", "center_bool_mask"):
            assert torch.equal(pad[k], ref[k]), (cid, k)
    assert bool(torch.isnan(cases["pad-nan"]["pos"]).any()) and bool((cases["pad-zero"]["dims"] == 0).all(-1).any())
    # duplicates: the cells the pair wins carry twice the attributes of the box, the heat of one
    c, ref = _target_ref("duplicate")
    single = [0, 1, 2, 3, 5]
    one = C.targets_fp64(c["pos"][:, single], c["dims"][:, single], c["rot"][:, single], c["valid"][:, single], c["grid"], c["range"])
    assert torch.equal(one["probs"], ref["probs"]) and torch.equal(one["center_bool_mask"], ref["center_bool_mask"])
    assert c["duplicate"] == (1, 4) and torch.equal(c["pos"][0, 1], c["pos"][0, 4])
    dup = c["dims"][0, 1].double()
    won = (ref["dims"][0] == 2.0 * dup).all(-1)
    assert int(won.sum()) >= 4 and bool((ref["probs"][0, ..., 0][won] > 0.01).all())
    # normalisation: the far box contributes nothing, the boxes beyond the edge reach 1.0 inside the grid off their centre
    c, ref = _target_ref("normalisation")
    keep = torch.ones(5, dtype=torch.bool)
    keep[c["far_box"]] = False
    without = C.targets_fp64(c["pos"][:, keep], c["dims"][:, keep], c["rot"][:, keep], c["valid"][:, keep], c["grid"], c["range"])
    assert torch.equal(without["probs"], ref["probs"]) and torch.equal(without["pos"], ref["pos"])
    for k in c["beyond_edge"]:
        alone = C.targets_fp64(c["pos"][:, k:k + 1], c["dims"][:, k:k + 1], c["rot"][:, k:k + 1], c["valid"][:, k:k + 1], c["grid"], c["range"])
        assert float(alone["probs"].max()) == 1.0 and not bool(alone["center_bool_mask"].any())
    alone = C.targets_fp64(c["pos"][:, 3:4], c["dims"][:, 3:4], c["rot"][:, 3:4], c["valid"][:, 3:4], c["grid"], c["range"])
    assert int((alone["probs"] > 0.01).sum()) == 1  # the 0.2 x 0.2 box lights its own cell only
    # near tie: along the column between the two boxes the heats differ by more than 1e-5 and by less than 1e-3 relative
    c, ref = _target_ref("near-tie")
    col = c["near_tie_col"]
    a, b = (C.targets_fp64(c["pos"][:, k:k + 1], c["dims"][:, k:k + 1], c["rot"][:, k:k + 1], c["valid"][:, k:k + 1], c["grid"], c["range"])
            ["probs"][0, :, col, 0] for k in (0, 1))
    lit = ref["probs"][0, :, col, 0] > 0.01
    gap = ((a - b) / a)[lit]
    assert int(lit.sum()) >= 5 and float(gap.min()) > 1e-4 and float(gap.max()) < 5e-4
    assert bool((ref["dims"][0, :, col, 2][lit] == 1.5).all())
