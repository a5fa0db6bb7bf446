"""CPU: tests/slim_decode_cases.py is what it says it is.

* The fp64 restatement equals the repository's torch formulation of the reference -- HeadDecoder.apply_output_modification +
  apply_flow_to_points on fp64 BEV maps (the port of head_decoder.py:67-408, 517-955), static_points_loss, NearestPointLoss / huber_delta --
  on every decode case (the default configuration, every legal forced-mode combination, both overwrite switches), values and gradients.
  The Kabsch fit between the two passes is a device kernel and not under test here: it is replaced by a function that records its arguments
  (pass 1: x, y, w) and returns the case's transform as a leaf, so the transform gradient is anchored too.
* The generators keep their promises: decision margins, planted classes, every value of every switch, the legal-mode enumeration.
* The fp32 copy of the restatement against the fp64 one, per quantity class: the numbers RECORDED in the cases module, from which the device
  bounds of tests/test_gpu_slim_decode_edges.py are taken (x 8).
"""
import itertools
import types

import pytest
import torch

from tests import slim_decode_cases as C

DECODE_IDS = list(C.decode_specs())
FOV_NAMES = {0: "none", 1: "ignore_out_fov", 2: "mask_close_fov"}


_slim_cfg = C.slim_cfg


def test_legal_mode_enumeration_matches_decode_meta():
    from liso_amd.slim.model.fused_decode import DecodeMeta

    plan = types.SimpleNamespace(shape=(1, 2, C.H, C.W), lin=torch.zeros(2, dtype=torch.int32))
    filled = torch.ones(1, C.H, C.W, dtype=torch.bool)
    accepted = []
    for st, dy, gr in itertools.product(("net", True, False), repeat=3):
        sp = dict(C.decode_specs()[DECODE_IDS[0]], modes=("net", st, dy, gr))
        try:
            DecodeMeta(_slim_cfg(sp), C.BEV_EXTENT, plan, filled, None, 0.4, torch.zeros(1, 2, 3))
            accepted.append((st, dy, gr))
        except AssertionError:
            assert not C.mode_legal(st, dy, gr), (st, dy, gr)
    assert accepted == C.LEGAL_MODES and len(accepted) == 13
    assert [sp["modes"][1:] for sp in C.decode_specs().values()][:13] == C.LEGAL_MODES


def test_every_value_of_every_switch_occurs():
    specs = list(C.decode_specs().values())
    for key, values in (("static_flow_zero", (False, True)), ("dynamic_flow_zero", (False, True)), ("overwrite_flow", (False, True)),
                        ("overwrite_logits", (False, True)), ("dyn_grad_scale", (0.0, 0.5, 1.0)), ("S", (1, 4)), ("N", (1, 255, 256, 257, 1000)),
                        ("pc_stride", (3, 4)), ("thr", (0.0, 0.4, 1.0, 1.5))):
        assert {sp[key] for sp in specs} == set(values), key
    assert {(sp["non_rigid"], sp["use_static_aggr"]) for sp in specs} == set(itertools.product((False, True), repeat=2))
    assert {sp["modes"][0] for sp in specs} == {"net", True, False}
    assert any(sp["dyn_grad_scale"] == 0.5 and not sp["dynamic_flow_zero"] for sp in specs)  # the scale reaches a live channel


@pytest.mark.parametrize("cid", DECODE_IDS)
def test_decode_case_holds_its_planted_rows_and_margins(cid):
    case = C.decode_case(cid)
    sp, cl = case["spec"], case["classes"]
    S, N = sp["S"], sp["N"]
    assert bool(C._margins_ok(case).all())
    lin = case["lin"].view(S, N)
    assert bool(((lin >= 0) == case["valid"]).all()) and bool((case["raw"][~case["valid"]] == 0).all())
    assert bool(cl["invalid"].any() and cl["unfilled"].any() and cl["filled"].any() and cl["tie"].any())
    if not sp.get("reduced"):
        assert bool((lin[:, 0] < 0).all() and (lin[:, N - 1] < 0).all() and (lin[:, N // 2] < 0).all())
        assert bool((cl["tie"] & cl["filled"]).any() and (cl["tie"] & cl["unfilled"]).any())
        assert len(torch.unique(lin[lin >= 0])) == S * C.H * C.W  # every pillar of every sample holds a point
    raw = case["raw"]
    assert bool((raw[..., 1][cl["tie"]] == raw[..., 3][cl["tie"]]).all())
    ref = C.decode_reference(cid)["out"]
    if sp["modes"][1:] == ("net", "net", "net") and sp["thr"] > 0:  # the tie survives the modes: `>=` calls it static
        rows = cl["tie"] & (cl["filled"] | torch.tensor(not sp["overwrite_logits"]))
        assert bool(rows.any()) and bool(ref["flags"][rows][:, 0].all())
        assert bool((ref["probs"][rows][:, 0] == ref["probs"][rows][:, 2]).all())
    if sp["thr"] == 0.0:
        assert bool(ref["flags"][case["valid"]][:, 1].all())
    if sp["thr"] > 1.0:
        assert not bool(ref["flags"][..., 1].any())
    if sp["thr"] == 1.0:  # dynamic forced ON: p_dyn == 1.0 == thr exactly at filled pillars, in both precisions
        assert bool((ref["probs"][cl["filled"]][:, 1] == 1.0).all()) and bool(ref["flags"][cl["filled"]][:, 1].all())
        assert not bool(ref["flags"][cl["unfilled"]][:, 1].any())
    assert bool((ref["flags"].sum(-1) == case["valid"].long()).all())  # exactly one flag per valid row, none at invalid rows


def _torch_formulation(case, monkeypatch):
    """the repository's port of the reference on fp64 BEV maps -> per-point predictions, pass-1 tensors, the leaves"""
    from liso_amd.slim.model.head_decoder import HeadDecoder
    from liso_amd.slim.slim_loss import static_aggregation as SA

    sp = case["spec"]
    S, N = sp["S"], sp["N"]
    net = case["net"].double().requires_grad_(True)
    T = case["T"].clone().requires_grad_(True)
    seen = {}

    def fit(x, y, w, valid, use_epsilon_on_weights=False):
        seen.update(x=x, y=y, w=w)
        return T, torch.zeros(S, dtype=torch.bool)

    monkeypatch.setattr(SA, "batched_weighted_pc_alignment", fit)
    dec = HeadDecoder(_slim_cfg(sp), "fw", C.BEV_EXTENT)
    dec.fused_decoding = False
    cell = case["lin"].view(S, N).clamp(min=0).long() % (C.H * C.W)
    coors = torch.stack([torch.div(cell, C.W, rounding_mode="floor"), cell % C.W], dim=-1).to(torch.int32)
    eye = torch.eye(4, dtype=torch.float64)[None].repeat(S, 1, 1)
    thr = torch.tensor(sp["thr"], dtype=torch.float32).double()
    modified = dec.apply_output_modification(
        net, thr, pc=case["pc"].double(), pointwise_voxel_coordinates_fs=coors, pointwise_valid_mask=case["valid"],
        filled_pillar_mask=case["filled"], inv_odom=eye, dynamic_flow_is_non_rigid_flow=sp["non_rigid"],
        overwrite_non_filled_pillars_with_default_flow=sp["overwrite_flow"],
        overwrite_non_filled_pillars_with_default_logits=sp["overwrite_logits"])[0]
    p = dec.apply_flow_to_points(modified_output_bev_img=modified, pointwise_voxel_coordinates_fs=coors, pointwise_valid_mask=case["valid"])
    out = {"dis_logit": p.disappearing_logit, "dis": p.disappearing, "logits": p.class_logits, "probs": p.class_probs, "staticness": p.staticness,
           "dynamicness": p.dynamicness, "groundness": p.groundness, "dyn_flow": p.dynamic_flow, "stat_flow": p.static_flow,
           "agg_flow": p.aggregated_flow, "saf_flow": p.static_aggr_flow, "x": seen["x"], "y": seen["y"], "w": seen["w"],
           "flags": torch.stack([p.is_static, p.is_dynamic, p.is_ground], dim=-1)}
    return out, net, T


@pytest.mark.parametrize("cid", DECODE_IDS)
def test_restatement_equals_the_torch_formulation_of_the_reference(cid, monkeypatch):
    from liso_amd.slim.slim_loss import slim_loss_adaptor as A

    A.set_fused_losses(False)
    try:
        case = C.decode_case(cid)
        sp = case["spec"]
        S, N = sp["S"], sp["N"]
        out, net, T = _torch_formulation(case, monkeypatch)
        ref = C.decode_reference(cid)
        assert torch.equal(out["flags"], ref["out"]["flags"])
        for k in C.OUT_CLASS:
            a, b = out[k].detach().double(), ref["out"][k]
            assert a.shape == b.shape, k
            # (the port rounds the rigid flow of the pillar centres to fp32, static_aggregation.py:88-99; the restatement keeps fp64)
            tol = 2e-7 if k in ("saf_flow", "agg_flow") else 1e-12
            assert float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max())), (k, float((a - b).abs().max()))
        up = case["upstream"]
        valid = case["valid"].reshape(-1)
        lin = case["lin"].long()[valid]

        def to_maps(graw):  # adjoint of the gather: the rows of a pillar add up
            return torch.zeros(S * C.H * C.W, 8, dtype=torch.float64).index_add_(0, lin, graw.reshape(-1, 8)[valid]).view(S, C.H, C.W, 8)

        (g1,) = torch.autograd.grad(sum((out[k] * up[k].double()).sum() for k in ("y", "w")), net, retain_graph=True)
        g2, gT = torch.autograd.grad(sum((out[k] * up[k].double()).sum() for k in C.FLOAT_OUTS), [net, T])
        for name, got, want in (("g1", g1, to_maps(ref["graw1"])), ("g2", g2, to_maps(ref["graw2"])), ("gT", gT, ref["gT"])):
            # that fp32 value multiplies the groundness gradient, and the transform's gradient passes the port's fp32 cast
            tol = 1e-6 if (sp["use_static_aggr"] and sp["non_rigid"]) or name == "gT" else 1e-11
            assert float((got - want).abs().max()) <= tol * max(1.0, float(want.abs().max())), float((got - want).abs().max())
        assert float(ref["graw2"].abs().max()) > 0
    finally:
        A.set_fused_losses(True)


@pytest.mark.parametrize("cid", list(C.static_specs()))
def test_static_loss_restatement_equals_static_points_loss(cid):
    from liso_amd.slim.slim_loss.slim_loss_adaptor import _masked_mean, static_points_loss

    case, ref = C.static_case(cid), C.static_reference(cid)
    flow, weight = case["flow"].double().requires_grad_(True), case["weight"].double().requires_grad_(True)
    mean = _masked_mean(static_points_loss(case["pc"][..., :3].double(), case["valid"], flow, weight, case["T"]), case["valid"])
    gf, gw = torch.autograd.grad(mean * case["g_mean"].double(), [flow, weight])
    if case["spec"].get("none_valid"):
        assert bool(torch.isnan(mean)) and bool(torch.isnan(ref["mean"]))
        assert bool((ref["gflow"] == 0).all()) and bool((ref["gweight"] == 0).all())
        return
    # (static_points_loss rounds the rigid flow of the point to fp32 before the residual, slim_loss_adaptor.py:43; the restatement keeps
    # fp64: 6e-8 of |est| ~ 1 on residuals of 0.1)
    assert abs(float(mean.detach()) - float(ref["mean"])) <= 1e-6 * abs(float(ref["mean"]))
    assert float((gf - ref["gflow"]).abs().max()) <= 1e-6 * float(ref["gflow"].abs().max())
    assert float((gw - ref["gweight"]).abs().max()) <= 1e-6 * float(ref["gweight"].abs().max())
    assert bool((ref["gflow"][~case["valid"]] == 0).all())
    if case["spec"].get("big"):  # either planted row alone carries far more than the bound of the mean
        with torch.no_grad():
            for row in case["planted_rows"]:
                s, i = divmod(row, case["spec"]["N"])
                fl = case["flow"].double().clone()
                fl[s, i] -= 50.0
                assert abs(float(C.static_loss_ref(case, fl, case["weight"].double())) / float(ref["mean"]) - 1.0) > 0.1
        assert case["spec"]["S"] * case["spec"]["N"] > C.BIG_ROW + 256


@pytest.mark.parametrize("cid", list(C.nploss_specs()))
def test_nearest_point_restatement_equals_nearest_point_loss(cid):
    from liso_amd.slim.slim_loss.knn_wrapper import NearestPointLoss, squared_sum
    from liso_amd.slim.slim_loss.slim_loss_adaptor import _masked_mean

    case, ref = C.nploss_case(cid), C.nploss_reference(cid)
    sp, valid = case["spec"], case["valid"]
    S, N, n_b = sp["S"], sp["N"], sp["n_b"]
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))  # noqa: E731
    lf = NearestPointLoss(bev_extent=[f32(v) for v in C.BEV_EXTENT], L1_delta=f32(sp["delta"]), drop_outliers__perc=0.0, fov_mode=FOV_NAMES[sp["fov_mode"]])
    flow = case["flow"].double().requires_grad_(True)
    q = case["pc"][..., :3].double() + flow
    nbr = case["nbr"]
    safe = torch.where((nbr >= 0) & (nbr < n_b), nbr, torch.zeros_like(nbr))
    nearest = torch.gather(case["cloud_b"][..., :3].double(), 1, safe[..., None].repeat(1, 1, 3))
    d2 = squared_sum(nearest - q, dim=-1)
    loss = lf(cloud_b__a=q, nearest_cloud_b__a=nearest, nearest_dist_sqr_b__a=d2)
    total = _masked_mean(loss, valid) * case["g_mean"].double()
    if sp["with_gd2"]:
        total = total + (torch.where(valid, d2, 0.0) * case["g_d2"].double()).sum()
    (gf,) = torch.autograd.grad(total, flow)
    if sp.get("none_valid"):
        assert bool(torch.isnan(ref["mean"])) and bool((ref["gflow"] == 0).all()) and not bool(valid.any())
        return
    assert abs(float(_masked_mean(loss, valid).detach()) - float(ref["mean"])) <= 1e-12 * abs(float(ref["mean"]))
    assert float((torch.where(valid, d2, 0.0) - ref["d2"]).abs().max()) <= 1e-12 * float(ref["d2"].max())
    assert float((gf - ref["gflow"]).abs().max()) <= 1e-12 * float(ref["gflow"].abs().max())
    # the planted classes
    assert bool(case["clear"][valid].all()) and S * N - int(valid.sum()) >= (0 if N == 1 else 3)
    w0 = valid & (ref["loss"] == 0) & (ref["d2"] > 0)
    if sp["fov_mode"] > 0 and N >= 255:
        assert bool(w0.any()) and bool((valid & (ref["loss"] > 0)).any())
        assert bool((valid & (case["min_fov_64"] < 0)).any())
    if sp["fov_mode"] == 2 and N >= 255:
        assert bool((valid & (case["min_fov_64"] > 0) & (case["d2_64"] >= case["min_fov_64"] ** 2)).any())
    if sp["delta"] > 0 and N >= 255:
        dd = f32(sp["delta"]) ** 2
        assert bool((valid & (ref["d2"] > 0) & (ref["d2"] < dd)).any()) and bool((valid & (ref["d2"] > dd)).any())
    if N >= 255 and not sp.get("big"):
        for i in case["planted"]["d2_zero"]:
            assert bool(valid[:, i].all()) and bool((ref["d2"][:, i] == 0).all()) and bool((ref["gflow"][:, i] == 0).all())
        for name, v in (("index_minus_one", -1), ("index_n_b", n_b)):
            i = case["planted"][name]
            assert bool((nbr[:, i] == v).all())
        assert n_b != N
    if sp["order"]:  # the index is in query order
        o = case["order"][torch.arange(S) % sp["clouds"]]
        assert torch.equal(case["index"], torch.gather(nbr, 1, o)) and (N == 1 or not torch.equal(case["index"], nbr))
        if sp["clouds"] == 2 and N > 1:
            assert not torch.equal(case["order"][0], case["order"][1])
    if sp.get("big"):
        with torch.no_grad():
            for row in C.BIG_PLANTED:  # each planted row alone carries far more than the bound of the mean
                keep = valid.clone()
                keep.view(-1)[row] = False
                assert bool(valid.view(-1)[row]) and abs(float(C._masked_mean(ref["loss"], keep, torch.float64)) / float(ref["mean"]) - 1.0) > 0.1


def test_knn_query_restatement_equals_the_nan_marked_sum():
    """knn_loss.py:44-58: padding rows of the cloud and of the flow are NaN before they are added; the queries go out in bucket order"""
    for cid in ("np-fov0-delta0-4x257-order-gd2", "np-fov0-delta0.1-1x256-identity-no_gd2"):
        case = C.nploss_case(cid)
        sp, v = case["spec"], case["valid"][..., None]
        nan = torch.full((), float("nan"))
        got = C.knn_queries_ref(case, case["flows"])
        for t, f in enumerate(case["flows"]):
            q = torch.where(v, case["pc"][..., :3], nan) + torch.where(v, f, nan)
            if case["order"] is not None:
                q = torch.stack([q[s].index_select(0, case["order"][s % sp["clouds"]]) for s in range(sp["S"])])
            assert torch.equal(torch.isnan(got[t]), torch.isnan(q)) and torch.equal(got[t].nan_to_num(), q.nan_to_num())


def test_extrema_cases_plant_their_extremes_past_one_sweep():
    for cid, (rows, stride, c, off) in C.extrema_specs().items():
        case = C.extrema_case(cid)
        x = case["buf"][off:off + rows * stride].view(rows, stride)
        assert torch.equal(case["ref"], torch.cat([x[:, :c].max(dim=0)[0], x[:, :c].min(dim=0)[0]]))
        if rows > C.BIG_ROW:
            assert bool((x[:, :c].argmax(dim=0) == rows - 1).all()) and bool((x[:, :c].argmin(dim=0) == C.BIG_ROW).all())


def test_fp32_restatement_error_per_quantity_class():
    """the numbers the device bounds come from.  Another host's libm may round an exp or a division the other way: twice the entry is allowed
    here; an entry of 0 means equal bits"""
    table = C.fp32_error_table()
    for k in sorted(table):
        print("%-22s fp32 vs fp64 %.3e   recorded %.1e   device bound %.1e" % (k, table[k], C.RECORDED[k], C.bound(k)))
    assert set(table) == set(C.RECORDED)
    for k, v in table.items():
        assert v <= 2.0 * C.RECORDED[k], (k, v, C.RECORDED[k])
        if C.RECORDED[k] > 0:
            assert v >= C.RECORDED[k] / 4.0, (k, v, "the recorded number no longer describes the cases")
