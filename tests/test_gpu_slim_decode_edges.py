"""The 14 kernels of liso_amd/csrc/slim_decode.hip (both decode passes with their backward, the static-points and nearest-point masked
means, the warped kNN queries, the channel extrema) and the per-row nearest-point loss of slim_loss.hip against the fp64 restatement of
tests/slim_decode_cases.py, per quantity and per row class (invalid / unfilled pillar / filled pillar / tie), never over a whole tensor.
Everything runs inside tests/guarded_alloc.guarded(): a write past an [S,N,...] output lands in a guard band.

Bounds (fixed before the first device run): max |got - ref| <= bound * max(|ref| over the row class, 1e-3), where bound = 8 x the error of the
fp32 restatement against the fp64 one for that quantity class and row class (slim_decode_cases.RECORDED, measured on the host by
tests/test_slim_decode_cases.py).  The factor 8 is for a device expf / sqrtf / division a few ulp off the host's and for FMA contraction
(slim_decode.hip is built with it).  A recorded error of 0 -- copies, constants, zeros, a single fp32 addition -- means equal bits.  The masked
means are non-negative fp32 terms summed in fp64 and get the relative bound of their class.  Flags are compared exactly on every row (the
generator keeps each decision 1e-4 clear of its threshold in fp64, or tied exactly); x, and the kNN queries of valid rows (fp32 pc + flow),
bit for bit; NaN at invalid query rows; exact zeros wherever the restatement is identically zero (invalid rows, dead channels, gradients behind
a forced or overwritten value).

Worst value observed on an MI355X over every case, as |got - ref| / max(|ref| over the class, 1e-3), with its bound in brackets (the host's
fp32 restatement gives the same figures but for grad_np, 2.6e-5 there: the device follows fp32 arithmetic, nothing more):
  out_copy     exact on every row class                      out_logit    filled, unfilled, tie 5.3e-8 (4.3e-7)
  out_prob     filled 9.1e-8 (6.6e-7), unfilled 8.6e-8 (5.6e-7), tie 7.4e-8 (5.8e-7)
  out_flow     filled 7.6e-8 (6.0e-7), unfilled 4.6e-8 (3.8e-7), tie 4.7e-5 (3.8e-4)
  grad1_logit  filled 4.4e-7 (3.5e-6), unfilled exact zeros, tie 2.4e-4 (1.9e-3)          grad1_flow   exact on every row class
  grad2_logit  filled 2.2e-7 (1.8e-6), unfilled 7.8e-8 (6.2e-7), tie 1.0e-4 (8.8e-4)
  grad2_flow   filled 5.7e-8 (4.6e-7), unfilled 2.4e-8 (1.9e-7), tie 5.9e-8 (4.7e-7)
  grad_trafo   1.2e-7 (1.0e-6)                               mean         static 7.9e-8 (6.4e-7), nearest-point 3.5e-7 (2.9e-6)
  np_row       1.1e-6 (8.8e-6)   grad_np  4.0e-5 (2.1e-4)    grad_static  8.1e-8 (6.5e-7)      invalid rows: exact zeros throughout
  (the tie figures are absolute errors of 1e-7 on values below the 1e-3 floor: 1 - p for p within 1e-5 of 1; grad_np is nn - (pc + flow) at
  |pc| = 30 and a distance of 0.03)
Flags, x, the kNN queries, the extrema, dist_sqr between the two nearest-point kernels and every repeated call: equal bits.  The whole file
takes 4 s.

What each planted class or shape is there to catch.  Each defect below was put, one at a time, into a local build of slim_decode.hip (value
changes only, no index that could leave a buffer; none committed) and this file run against it:
  x/y swap of ext_span / ext_lo in select()          -> saf_flow, agg_flow and the trafo gradient of every decode case (non-square extent)
  row/column swap (cell % w for cell / w)            -> the same outputs of every case with more than one pillar (5 x 7 grid)
  grid stride one short in the three reductions      -> the masked means of the "big" cases: row 131 071 is counted twice (the extrema are
                                                        idempotent and cannot see it); one long -> row 131 072 is lost: means and extrema
  p_static > p_ground for >=                         -> flags and agg_flow of the tie pillars wherever static and ground are both undecided
  p_dyn > thr for >=                                 -> the flags of thr1-dynamic_on (p_dyn == 1.0 == thr)
  live_logit ignored in either backward              -> exact-zero checks of every case with a forced or overwritten logit (22 tests)
  index[row] for index[qrow]                         -> every nearest-point case with a query order, against the restatement and the sibling
  order[0] for order[s % clouds]                     -> the S = 4, clouds = 2 nearest-point cases and their kNN queries
  dyn_grad_scale dropped                             -> grad2_flow of the cases with scale 0.5 and 0 and a live dynamic flow
  `filled` ignored in w                              -> w at unfilled pillars (out_prob/unfilled, exact zeros), 16 cases
  `filled` ignored in static2                        -> agg_flow at unfilled pillars of the five use_static_aggr cases
No wrong build left this file green.  The one divergence the file found in the kernels as they were: np_eval() let fminf / fmaxf swallow a NaN
squared distance when delta > 0 (a finite mean where torch and slim_loss.hip give NaN); it propagates now, and
test_nan_distance_on_a_valid_row_propagates_like_torch[...delta0.3...] fails against the earlier kernels.
"""
import ctypes
import functools
import types

import pytest
import torch

from tests import slim_decode_cases as C
from tests.guarded_alloc import guarded

pytestmark = pytest.mark.gpu

DECODE_IDS = list(C.decode_specs())
DEV = "cuda:0"


def _report(tag, res):
    """print every figure, then assert every bound"""
    for k in sorted(res):
        print("OBS %s %s %.3e bound %.3e" % (tag, k, res[k], C.bound(k)))
    for k, v in res.items():
        assert v <= C.bound(k), (tag, k, v, C.bound(k))


def _meta(case):
    from liso_amd.slim.model.fused_decode import DecodeMeta

    sp = case["spec"]
    plan = types.SimpleNamespace(shape=(sp["S"], sp["N"], C.H, C.W), lin=case["lin"].to(DEV))
    forced = any(m != "net" for m in sp["modes"][1:])
    extrema = (case["extrema"][0].to(DEV), case["extrema"][1].to(DEV)) if forced else None  # NULL where the kernels must not read it
    return DecodeMeta(C.slim_cfg(sp), C.BEV_EXTENT, plan, case["filled"].to(DEV), extrema, sp["thr"], case["pc"].to(DEV),
                      overwrite_flow=sp["overwrite_flow"], overwrite_logits=sp["overwrite_logits"], non_rigid=sp["non_rigid"])


def _run_decode(case, subset=None, pass1=("y", "w"), want_T=True):
    """both passes and their backward through fused_decode -> dict(out, graw1, graw2, gT) on the host.  Outputs outside `subset` / `pass1`
    get no upstream gradient: their pointers reach the backward kernels as NULL; want_T False: grad_saf_eff NULL"""
    from liso_amd.slim.model import fused_decode as FD

    with guarded() as g:
        meta = _meta(case)
        raw = case["raw"].to(DEV).requires_grad_(True)
        T = case["T"].to(DEV).requires_grad_(want_T)
        up = {k: v.to(DEV) for k, v in case["upstream"].items()}
        x, y, w = FD.decode_weights(raw, meta)
        o = FD.decode_points(raw, T, meta)
        p1 = {"y": y, "w": w}
        (g1,) = torch.autograd.grad(sum((p1[k] * up[k]).sum() for k in pass1), raw)
        names = C.FLOAT_OUTS if subset is None else subset
        res = torch.autograd.grad(sum((o[k] * up[k]).sum() for k in names), [raw, T] if want_T else [raw], allow_unused=True)
        g2, gT = res[0], (res[1] if want_T else None)
        n = g.check()
        assert n > 0
    out = {k: v.detach().cpu() for k, v in o.items()}
    out.update(x=x.cpu(), y=y.detach().cpu(), w=w.detach().cpu())
    return dict(out=out, graw1=g1.cpu(), graw2=g2.cpu(), gT=None if gT is None else gT.cpu())


def _check_decode_gradients(case, got, ref, tag):
    _report(tag, C.compare_decode(case, dict(got, out={}), ref))
    for k in ("graw1", "graw2"):
        assert bool(torch.isfinite(got[k]).all()), (tag, k)
        assert C.zeros_kept(got[k], ref[k]), (tag, k, "a gradient where the restatement has an exact zero")


@pytest.mark.parametrize("cid", DECODE_IDS)
def test_decode_passes_match_fp64_per_quantity_and_row_class(cid):
    case, ref = C.decode_case(cid), C.decode_reference(cid)
    got = _run_decode(case)
    sp, cl = case["spec"], case["classes"]
    S, N = sp["S"], sp["N"]
    assert torch.equal(got["out"]["flags"], ref["out"]["flags"]), (cid, int((got["out"]["flags"] != ref["out"]["flags"]).sum()))
    assert torch.equal(got["out"]["x"], torch.where(case["valid"][..., None], case["pc"][..., :3], torch.zeros(())))
    _report(cid, C.compare_decode(case, dict(out=got["out"]), ref))
    for k in C.OUT_CLASS:
        assert got["out"][k].shape == ref["out"][k].shape and bool(torch.isfinite(got["out"][k]).all()), k
        assert C.zeros_kept(got["out"][k], ref["out"][k]), (cid, k)
        assert bool((got["out"][k][cl["invalid"]] == 0).all()), (cid, k)
    for k in ("staticness", "dynamicness", "groundness"):  # the columns of probs, bit for bit
        assert torch.equal(got["out"][k], got["out"]["probs"][..., ("staticness", "dynamicness", "groundness").index(k)]), k
    _check_decode_gradients(case, got, ref, cid)
    assert bool((got["graw1"][cl["invalid"]] == 0).all()) and bool((got["graw2"][cl["invalid"]] == 0).all())
    assert got["gT"].shape == (S, 4, 4) and bool((got["gT"][:, 2:] == 0).all()) and bool((got["gT"][:, :, 2] == 0).all())
    assert C.zeros_kept(got["gT"], ref["gT"])


@pytest.mark.parametrize("prefix,subset,pass1", C.SUBSET_RUNS, ids=["%s-%s-%s" % (p, "+".join(s), "+".join(q)) for p, s, q in C.SUBSET_RUNS])
def test_backward_with_null_upstream_gradients_and_the_trafo_gradient(prefix, subset, pass1):
    """any subset of the 11 output gradients, grad_y or grad_w alone; the host-side reduction of grad_saf_eff onto T in
    _DecodePoints.backward against autograd through the restatement (saf_flow alone; use_static_aggr with agg_flow alone)"""
    cid = C.decode_id(prefix)
    case, ref = C.decode_case(cid), C.decode_reference(cid, subset, pass1)
    got = _run_decode(case, subset, pass1)
    _check_decode_gradients(case, got, ref, "%s/%s" % (prefix, "+".join(subset)))
    reaches_T = "saf_flow" in subset or (case["spec"]["use_static_aggr"] and "agg_flow" in subset)
    if reaches_T:
        assert float(ref["gT"].abs().max()) > 0 and C.zeros_kept(got["gT"], ref["gT"])
    else:
        assert got["gT"] is None and (ref["gT"] is None or not bool(ref["gT"].any()))
    # without a gradient for T the kernel gets grad_saf_eff == NULL and writes the same grad_raw
    again = _run_decode(case, subset, pass1, want_T=False)
    assert again["gT"] is None and torch.equal(again["graw2"], got["graw2"]) and torch.equal(again["graw1"], got["graw1"])


def test_forward_writes_only_the_outputs_it_is_asked_for():
    """inference: `want` leaves the other output pointers NULL; the values are those of the full call, bit for bit"""
    from liso_amd.slim.model import fused_decode as FD

    for prefix, want in (("mode03", ("agg_flow",)), ("mode00", ("stat_flow", "agg_flow", "saf_flow")), ("mode07", ("probs", "dis"))):
        case = C.decode_case(C.decode_id(prefix))
        with guarded() as g, torch.no_grad():
            meta = _meta(case)
            raw, T = case["raw"].to(DEV), case["T"].to(DEV)
            full = FD.decode_points(raw, T, meta)
            part = FD.decode_points(raw, T, meta, want=want)
            g.check()
        assert part["flags"] is None
        for k in C.FLOAT_OUTS:
            assert (part[k] is not None) == (k in want), k
            if k in want:
                assert torch.equal(part[k], full[k]), (prefix, k)


# ---- static-points loss ------------------------------------------------------------------------------------------------------------
def _run_static(case, need=("flow", "weight")):
    from liso_amd.slim.model import fused_decode as FD

    with guarded() as g:
        flow = case["flow"].to(DEV).requires_grad_("flow" in need)
        weight = case["weight"].to(DEV).requires_grad_("weight" in need)
        mean = FD.static_points_loss_mean(case["pc"].to(DEV), case["valid"].to(DEV), flow, weight, case["T"].to(DEV))
        grads = torch.autograd.grad(mean * case["g_mean"].to(DEV), [t for t in (flow, weight) if t.requires_grad])
        g.check()
    res = dict(mean=mean.detach().cpu())
    for k, v in zip([k for k in ("flow", "weight") if k in need], grads):
        res["g" + k] = v.cpu()
    return res


@pytest.mark.parametrize("cid", list(C.static_specs()))
def test_static_points_loss_mean_and_gradients(cid):
    case, ref = C.static_case(cid), C.static_reference(cid)
    got = _run_static(case)
    valid = case["valid"]
    if not bool(valid.any()):  # 0 / 0 as torch; nothing reaches the inputs
        assert bool(torch.isnan(got["mean"])) and not bool(got["gflow"].any()) and not bool(got["gweight"].any())
    else:
        print("static mean got %.9g ref %.9g" % (float(got["mean"]), float(ref["mean"])))
        _report(cid, C.compare_static(case, got, ref))
        assert bool(torch.isfinite(got["gflow"]).all() and torch.isfinite(got["gweight"]).all())
    assert not bool(got["gflow"][~valid].any()) and not bool(got["gweight"][~valid].any())
    # bit reproducible, and each gradient alone (the other pointer NULL) is the same
    again, only_f, only_w = _run_static(case), _run_static(case, ("flow",)), _run_static(case, ("weight",))
    for k in ("mean", "gflow", "gweight"):
        assert torch.equal(again[k], got[k]) or bool(torch.isnan(got[k]).all()), k
    assert torch.equal(only_f["gflow"], got["gflow"]) and torch.equal(only_w["gweight"], got["gweight"])


# ---- nearest-point loss --------------------------------------------------------------------------------------------------------------
def _np_cfg(sp):
    from liso_amd import _lib as L

    return L.SlimNpLossCfg(sp["S"], sp["clouds"], sp["N"], sp["n_b"], (ctypes.c_float * 4)(*C.BEV_EXTENT), sp["fov_mode"], sp["delta"])


def _run_nploss(case, with_gd2):
    from liso_amd.slim.model import fused_decode as FD

    with guarded() as g:
        flow = case["flow"].to(DEV).requires_grad_(True)
        order = None if case["order"] is None else case["order"].to(DEV).contiguous()
        mean, d2 = FD._NearestPointLossMean.apply(case["pc"].to(DEV), case["valid"].to(DEV), flow, case["cloud_b"].to(DEV),
                                                  case["index"].to(DEV).contiguous(), order, _np_cfg(case["spec"]))
        total = mean * case["g_mean"].to(DEV)
        if with_gd2:
            total = total + (d2 * case["g_d2"].to(DEV)).sum()
        (gf,) = torch.autograd.grad(total, flow)
        g.check()
    return dict(mean=mean.detach().cpu(), d2=d2.detach().cpu(), gflow=gf.cpu())


@functools.lru_cache(maxsize=None)
def _masked_np(cid):
    case = C.nploss_case(cid)
    return _run_nploss(case, case["spec"]["with_gd2"])


@pytest.mark.parametrize("cid", list(C.nploss_specs()))
def test_nearest_point_loss_mean_dist_sqr_and_gradient(cid):
    case, ref = C.nploss_case(cid), C.nploss_reference(cid)
    sp, valid = case["spec"], case["valid"]
    got = _masked_np(cid)
    if not bool(valid.any()):
        assert bool(torch.isnan(got["mean"])) and not bool(got["gflow"].any()) and not bool(got["d2"].any())
    else:
        print("np mean got %.9g ref %.9g" % (float(got["mean"]), float(ref["mean"])))
        _report(cid, C.compare_nploss(case, got, ref))
    assert bool(torch.isfinite(got["gflow"]).all()) and not bool(got["gflow"][~valid].any()) and not bool(got["d2"][~valid].any())
    assert C.zeros_kept(got["gflow"], ref["gflow"]) and C.zeros_kept(got["d2"], ref["d2"])  # a query on its neighbour: d2 == 0, no gradient
    again = _run_nploss(case, sp["with_gd2"])
    for k in ("mean", "d2", "gflow"):
        assert torch.equal(again[k], got[k]) or bool(torch.isnan(got[k]).all()), k
    # the other state of the optional grad_dist_sqr pointer
    other, ref_other = _run_nploss(case, not sp["with_gd2"]), C.nploss_reference(cid, not sp["with_gd2"])
    if bool(valid.any()):
        _report(cid + "/gd2-flipped", C.compare_nploss(case, dict(gflow=other["gflow"]), ref_other))
    assert torch.equal(other["d2"], got["d2"])


@pytest.mark.parametrize("cid", [c for c in C.nploss_specs() if "big" not in c])
def test_per_row_nearest_point_loss_is_the_same_arithmetic(cid):
    """liso_nearest_point_loss_{fwd,bwd}_f32 (slim_loss.hip): per-row losses in point order, NaN padding rows; against the same restatement,
    and dist_sqr bit for bit what the masked kernel wrote on the rows valid in both"""
    from liso_amd import _lib as L
    from liso_amd.slim.slim_loss.knn_wrapper import _NearestPointLossFused

    case, ref = C.nploss_case(cid), C.nploss_reference(cid)
    sp, valid = case["spec"], case["valid"]
    n_valid = int(valid.sum())
    with guarded() as g:
        cloud_a = torch.where(valid[..., None], case["pc"][..., :3], torch.full((), float("nan"))).contiguous().to(DEV)
        flow = case["flow"].to(DEV).requires_grad_(True)
        cfg = L.NpLossCfg(sp["S"], sp["N"], sp["n_b"], (ctypes.c_float * 4)(*C.BEV_EXTENT), sp["fov_mode"], sp["delta"])
        loss, d2 = _NearestPointLossFused.apply(cloud_a, flow, case["cloud_b"][..., :3].contiguous().to(DEV), case["nbr"].to(DEV), cfg)
        # the upstream gradients the masked mean hands down: g / count on the valid rows (+ grad_dist_sqr)
        gl = torch.where(valid.to(DEV), case["g_mean"].to(DEV) / max(n_valid, 1), torch.zeros((), device=DEV))
        gd = torch.where(valid, case["g_d2"], torch.zeros(())).to(DEV) if sp["with_gd2"] else None
        (gf,) = torch.autograd.grad([loss, d2] if gd is not None else [loss], flow, [gl, gd] if gd is not None else [gl])
        g.check()
    loss, d2, gf = loss.detach().cpu(), d2.detach().cpu(), gf.cpu()
    assert bool(torch.isnan(loss[~valid]).all()) and bool(torch.isfinite(loss[valid]).all()) and bool(torch.isfinite(gf).all())
    assert not bool(gf[~valid].any())
    if n_valid:
        z = torch.zeros(())
        res = C.compare_nploss(case, dict(d2=torch.where(valid, d2, z), loss=torch.where(valid, loss, z), gflow=gf), ref)
        _report(cid + "/per-row", res)
        assert torch.equal(d2[valid], _masked_np(cid)["d2"][valid])
        mean = (loss[valid].double().sum().float() / torch.tensor(float(n_valid))).item()  # the header's reduction, on the host
        assert abs(mean - float(_masked_np(cid)["mean"])) <= 2.0 ** -22 * abs(mean), (mean, float(_masked_np(cid)["mean"]))


@pytest.mark.parametrize("cid", ["np-fov0-delta0.3-4x257-order-gd2", "np-fov2-delta0-4x255-order-gd2"])
def test_nan_distance_on_a_valid_row_propagates_like_torch(cid):
    """one valid row with a NaN coordinate: the mean is NaN (torch's clamp / sqrt / NaN * 0 propagate; fminf / fmaxf alone would not, with
    delta > 0), as in the per-row kernel; that row gets a zero gradient, every other row the gradient it had"""
    base = C.nploss_case(cid)
    s, i = [int(v) for v in base["valid"].nonzero()[7]]
    case = dict(base, pc=base["pc"].clone())
    case["pc"][s, i, 1] = float("nan")
    ref = C.nploss_with_grads(case, torch.float64)
    got, clean = _run_nploss(case, True), _masked_np(cid)
    assert bool(torch.isnan(ref["mean"])) and bool(torch.isnan(got["mean"])) and bool(torch.isnan(got["d2"][s, i]))
    assert bool(torch.isfinite(got["gflow"]).all()) and not bool(got["gflow"][s, i].any())
    keep = torch.ones_like(base["valid"])
    keep[s, i] = False
    assert torch.equal(got["gflow"][keep], clean["gflow"][keep]) and torch.equal(got["d2"][keep], clean["d2"][keep])


# ---- kNN queries ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["np-fov0-delta0-4x257-order-gd2", "np-fov0-delta0.1-1x256-identity-no_gd2", "np-fov1-delta0.1-4x1-order",
                                 "np-fov1-delta0.3-1x1000-order-no_gd2"])
def test_knn_queries_are_fp32_pc_plus_flow_in_query_order(cid):
    from liso_amd import _lib as L

    case = C.nploss_case(cid)
    sp = case["spec"]
    S, N, types_n = sp["S"], sp["N"], len(case["flows"])
    ref = C.knn_queries_ref(case, case["flows"])
    with guarded() as g:
        pc, v8 = case["pc"].to(DEV), case["valid"].to(torch.uint8).to(DEV)
        fl = [f.contiguous().to(DEV) for f in case["flows"]]
        order = None if case["order"] is None else case["order"].to(DEV).contiguous()
        query = torch.empty((types_n, S, N, 3), dtype=torch.float32, device=DEV)
        ptrs = (ctypes.c_void_p * types_n)(*[f.data_ptr() for f in fl])
        L.check(L.lib().liso_slim_knn_queries(S, sp["clouds"], N, types_n, L.ptr(pc), pc.shape[-1], L.ptr(v8), ptrs,
                                              L.ptr(order) if order is not None else None, L.ptr(query), L.stream_ptr()), "slim_knn_queries")
        g.check()
    q = query.cpu()
    assert torch.equal(torch.isnan(q), torch.isnan(ref)) and torch.equal(q.nan_to_num(), ref.nan_to_num())
    assert bool(torch.isnan(ref).any()) and bool(torch.isnan(ref).all(dim=-1).eq(torch.isnan(ref).any(dim=-1)).all())


# ---- channel extrema -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", list(C.extrema_specs()))
def test_channel_extrema_small_shapes_and_two_sweeps(cid):
    from liso_amd.utils.graph_safety import channel_extrema

    case = C.extrema_case(cid)
    rows, stride, c, off = case["rows"], case["stride"], case["c"], case["off"]
    with guarded() as g:
        buf = case["buf"].to(DEV)
        x = buf[off:off + rows * stride].view(rows, stride)[:, :c]
        hi, lo = channel_extrema(x)
        hi2, lo2 = channel_extrema(x)
        g.check()
    got = torch.cat([hi, lo]).cpu()
    assert torch.equal(got, case["ref"]), (got, case["ref"])
    assert torch.equal(torch.cat([hi2, lo2]).cpu(), got)
