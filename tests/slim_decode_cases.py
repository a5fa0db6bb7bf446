"""Cases and the fp64 restatement for the per-point SLIM decoder and its point-wise losses (include/liso_slim_decode.h, and the
per-row nearest-point loss of include/liso_slim.h).  Importable without a GPU; tests/test_slim_decode_cases.py anchors the restatement
to the torch formulation of the reference (HeadDecoder, static_points_loss, NearestPointLoss) and checks what the generators promise;
tests/test_gpu_slim_decode_edges.py runs the kernels on the same cases.

The restatement (`decode_ref`, `static_loss_ref`, `nploss_ref`, `knn_queries_ref`, `extrema_ref`) is plain torch with autograd, written
from the header and the reference lines it cites; it never calls liso_amd/slim/model/fused_decode.py.  `dtype=torch.float32` evaluates the
same statements in fp32 (masked means: fp32 terms summed in fp64, fp32 sum / fp32 count, as the header states): the distance between the two
is what fp32 arithmetic alone costs per quantity class, RECORDED below, and the device bounds are 8 x those numbers.

Geometry of every small case: a 5 x 7 grid on the non-square, off-centre extent lo = (-10, -24), span = (20, 56) -- a row/column or x/y
swap moves every pillar centre.  N in {1, 255, 256, 257, 1000}, S in {1, 4}; S = 4 is 2 iterations x 2 clouds, so `order[s % clouds]` and
an index in query order matter.  pc_stride and cloud_b_stride are 3 or 4, n_b != n.

Decode cases: the 13 (static, dynamic, ground) logit-mode combinations DecodeMeta's assertions accept (LEGAL_MODES), with the
disappearing mode, static/dynamic_flow_zero, overwrite_flow, overwrite_logits, non_rigid x use_static_aggr and dyn_grad_scale in
{1, 0.5, 0} cycled across them (not crossed; every value of every switch occurs), + 3 threshold cases (0: all dynamic, 1.5: none, exactly 1.0
with the dynamic logit forced ON) + one 4 x 1 case = 17 decode cases.  Every case but the 4 x 1 one holds: invalid rows (first, last,
interior), valid rows in unfilled and in filled pillars, and "tie" pillars whose static and ground logits are bitwise equal with the dynamic
logit 12 below (p_static == p_ground exactly: `>=` must call them static).  Every other valid row keeps |p_dyn - thr| and
|p_static - p_ground| above MARGIN in fp64 unless the two sides are equal exactly in both precisions (equal logits; p_dyn == 1.0 == thr), so
flags are compared exactly and no row is excused.  (Two comparisons decide nothing and are not held to the margin: p_static against
p_ground on a row that is dynamic, and p_dyn >= 0 under the threshold 0.)

Reduction cases ("big"): 2 x 66 000 rows (> 512 * 256 = 131 072, the reach of one grid-stride sweep) with dominant terms at rows 131 071,
131 072 and the last row: a stride one short counts row 131 071 twice, a stride one long skips row 131 072, a missing second sweep loses the
tail -- each moves the mean far beyond the bound.  (The extrema are idempotent: a row visited twice is harmless there and invisible; the
minimum sits in row 131 072 and the maximum in the last row.)
"""
import functools
import itertools

import torch

H, W = 5, 7
EXT_LO, EXT_SPAN = (-10.0, -24.0), (20.0, 56.0)
BEV_EXTENT = (EXT_LO[0], EXT_LO[1], EXT_LO[0] + EXT_SPAN[0], EXT_LO[1] + EXT_SPAN[1])
MARGIN = 1e-4
FLOOR = 1e-3  # max(|ref| over the class, FLOOR) scales every bound
FLOAT_OUTS = ("dis_logit", "dis", "logits", "probs", "staticness", "dynamicness", "groundness", "dyn_flow", "stat_flow", "agg_flow", "saf_flow")
_CH_SCALE = torch.tensor([1.0, 1.5, 1.5, 1.0, 0.3, 0.3, 0.5, 0.5])

FACTOR = 8.0  # device expf / sqrtf / division within a few ulp of the host's, FMA contraction (slim_decode.hip is built with it)

# Worst |fp32 restatement - fp64 restatement| / max(|fp64| over the row class, FLOOR) over every case, per "quantity class/row class" (measured
# on the host by fp32_error_table(); tests/test_slim_decode_cases.py fails if a class leaves [entry / 4, 2 x entry] -- another host's libm -- ; rounded up to two digits).  0.0: copies,
# constants, zeros, or one fp32 operation on fp32 inputs that both sides round alike -- reproduced exactly or not at all.
# Quantity classes: out_copy (x, dis_logit, stat_flow, dyn_flow), out_logit (logits), out_prob (dis, probs, staticness, dynamicness, groundness,
# w), out_flow (y, agg_flow, saf_flow), grad{1,2}_{logit,flow} (pass, channels 0:4 / 4:8 of d / d raw), grad_trafo, mean (both masked means),
# np_row (per-row nearest-point loss, dist_sqr), grad_static (d mean / d flow, weight), grad_np (d / d flow).  The large entries are fp32's own:
# 1 - p where p is within 1e-5 of 1 ("tie" pillars under a forced mode), nn - (pc + flow) at |pc| = 30 and a distance of 0.03.
RECORDED = {
    "grad1_flow/filled": 0.0, "grad1_flow/invalid": 0.0, "grad1_flow/tie": 0.0, "grad1_flow/unfilled": 0.0, "grad1_logit/filled": 4.4e-7,
    "grad1_logit/invalid": 0.0, "grad1_logit/tie": 2.4e-4, "grad1_logit/unfilled": 0.0, "grad2_flow/filled": 5.8e-8, "grad2_flow/invalid": 0.0,
    "grad2_flow/tie": 5.9e-8, "grad2_flow/unfilled": 2.4e-8, "grad2_logit/filled": 2.3e-7, "grad2_logit/invalid": 0.0, "grad2_logit/tie": 1.1e-4,
    "grad2_logit/unfilled": 7.7e-8, "grad_np/invalid": 0.0, "grad_np/valid": 2.6e-5, "grad_static/invalid": 0.0, "grad_static/valid": 8.1e-8,
    "grad_trafo/all": 1.3e-7, "mean/np": 3.6e-7, "mean/static": 8.0e-8, "np_row/invalid": 0.0, "np_row/valid": 1.1e-6, "out_copy/filled": 0.0,
    "out_copy/invalid": 0.0, "out_copy/tie": 0.0, "out_copy/unfilled": 0.0, "out_flow/filled": 7.5e-8, "out_flow/invalid": 0.0,
    "out_flow/tie": 4.7e-5, "out_flow/unfilled": 4.7e-8, "out_logit/filled": 5.4e-8, "out_logit/invalid": 0.0, "out_logit/tie": 5.4e-8,
    "out_logit/unfilled": 5.3e-8, "out_prob/filled": 8.2e-8, "out_prob/invalid": 0.0, "out_prob/tie": 7.3e-8, "out_prob/unfilled": 7.0e-8,
}


def bound(key):
    return FACTOR * RECORDED[key]


def mode_legal(static, dynamic, ground):
    """the three assertions of DecodeMeta.__init__ (head_decoder.py:812-817, :827-829, :905-907)"""
    if static is True and not (dynamic is False and ground is False):
        return False
    if static is False and dynamic is False and ground is False:
        return False
    if ground is True and not (static is False and dynamic is False):
        return False
    return True


LEGAL_MODES = [m for m in itertools.product(("net", True, False), repeat=3) if mode_legal(*m)]
assert len(LEGAL_MODES) == 13
_TAG = {"net": "net", True: "on", False: "off"}


def decode_specs():
    """{case id: spec}; ids say what the case is for"""
    specs = {}
    ns = (255, 256, 257, 1000)
    for i, (st, dy, gr) in enumerate(LEGAL_MODES):
        nr, sa = ((0, 0), (0, 1), (1, 0), (1, 1))[i % 4]
        sp = dict(modes=(("net", True, False)[i % 3], st, dy, gr), static_flow_zero=bool(i % 2), dynamic_flow_zero=bool((i // 2) % 2),
                  overwrite_flow=i % 5 != 2, overwrite_logits=i % 4 != 1, non_rigid=bool(nr), use_static_aggr=bool(sa),
                  dyn_grad_scale=(1.0, 0.5, 0.0)[i % 3], S=4 if i % 2 == 0 else 1, N=ns[i % 4], thr=0.4, pc_stride=3 + i % 2, seed=100 + i)
        cid = "mode%02d-dis_%s-st_%s-dy_%s-gr_%s-sfz%d-dfz%d-owf%d-owl%d-nr%d-sa%d-dgs%g-%dx%d" % (
            i, _TAG[sp["modes"][0]], _TAG[st], _TAG[dy], _TAG[gr], sp["static_flow_zero"], sp["dynamic_flow_zero"], sp["overwrite_flow"],
            sp["overwrite_logits"], nr, sa, sp["dyn_grad_scale"], sp["S"], sp["N"])
        specs[cid] = sp
    base = dict(modes=(False, "net", "net", False), static_flow_zero=False, dynamic_flow_zero=False, overwrite_flow=True, overwrite_logits=True,
                non_rigid=False, use_static_aggr=False, dyn_grad_scale=1.0, pc_stride=4)
    specs["thr0-every_valid_row_dynamic-4x257"] = dict(base, S=4, N=257, thr=0.0, seed=201)
    specs["thr1.5-no_row_dynamic-1x255"] = dict(base, S=1, N=255, thr=1.5, seed=202)
    specs["thr1-dynamic_on_p_dyn_equals_thr-4x256"] = dict(base, modes=("net", "net", True, "net"), S=4, N=256, thr=1.0, seed=203)
    specs["rows-4x1-one_thread_per_sample"] = dict(base, S=4, N=1, thr=0.4, seed=204, reduced=True)
    return specs


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def logit_constants(modes, mx, mn):
    """artificial_logit_network_output (head_decoder.py:779-955) for the on / off modes, in the order of the reference: a forced channel is
    a constant map and enters the extrema of the channels decided after it.  mx, mn: [4] extrema of the raw logit maps (any float dtype)"""
    mx, mn = list(mx.unbind(0)), list(mn.unbind(0))
    c = [None] * 4
    if modes[0] != "net":
        c[0] = torch.zeros_like(mx[0]) + (0.0 if modes[0] is True else -100.0)
    if modes[1] != "net":
        c[1] = torch.maximum(mx[2], mx[3]) + (100.0 if modes[1] is True else -100.0)
        mx[1] = mn[1] = c[1]
    if modes[2] != "net":
        c[2] = torch.maximum(mx[1], mx[3]) + 100.0 if modes[2] is True else torch.minimum(mn[1], mn[3]) - 100.0
        mx[2] = mn[2] = c[2]
    if modes[3] != "net":
        c[3] = torch.maximum(mx[1], mx[2]) + 100.0 if modes[3] is True else torch.minimum(mn[1], mn[2]) - 100.0
    return c


def cell_centres(lin):
    """fp64 metric centre of the pillar of every row (bev_utils.py:24-40): x from the grid ROW over span[0], y from the COLUMN"""
    cell = lin.clamp(min=0).long() % (H * W)
    rr, cc = torch.div(cell, W, rounding_mode="floor"), cell % W
    cx = ((rr.double() + 0.5) / H) * EXT_SPAN[0] + EXT_LO[0]
    cy = ((cc.double() + 0.5) / W) * EXT_SPAN[1] + EXT_LO[1]
    return cx, cy


def decode_ref(case, raw, T, dtype=torch.float64):
    """both decode passes of one case -> {name: [S,N,...]}; raw [S,N,8] of `dtype` and T [S,4,4] float64 may require grad"""
    sp = case["spec"]
    modes = sp["modes"]
    S, N = sp["S"], sp["N"]
    valid, filled = case["valid"], case["filled_pt"]
    unf = ~filled
    consts = logit_constants(modes, case["extrema"][0].to(dtype), case["extrema"][1].to(dtype))
    logit = [raw[..., i] if modes[i] == "net" else consts[i].expand(S, N) for i in range(4)]
    zero2 = torch.zeros(S, N, 2, dtype=dtype)
    sf = zero2 if sp["static_flow_zero"] else raw[..., 4:6]
    df = zero2 if sp["dynamic_flow_zero"] else raw[..., 6:8]
    s = sp["dyn_grad_scale"]
    df = df * s - df.detach() * (s - 1.0)  # scale_gradient (:720-726): value unchanged, gradient times s
    if sp["overwrite_logits"]:  # defaults at unfilled pillars (:566-590)
        d = (-100.0, -100.0 if modes[1] is False else 0.0, 0.0 if modes[2] is True else -100.0, 0.0 if modes[3] is True else -100.0)
        logit = [torch.where(unf, torch.full((), d[i], dtype=dtype), logit[i]) for i in range(4)]
    if sp["overwrite_flow"]:
        sf, df = torch.where(unf[..., None], zero2, sf), torch.where(unf[..., None], zero2, df)
    cl = torch.stack(logit[1:], dim=-1)
    probs = torch.softmax(cl, dim=-1)
    thr = torch.tensor(sp["thr"], dtype=torch.float32).to(dtype)  # the device threshold is fp32
    is_dyn = probs[..., 1] >= thr
    is_static = (probs[..., 0] >= probs[..., 2]) & ~is_dyn
    is_ground = ~(is_static | is_dyn)
    cx, cy = (v.view(S, N) for v in cell_centres(case["lin"]))
    D = T - torch.eye(4, dtype=torch.float64)
    saf = torch.stack([D[:, None, 0, 0] * cx + D[:, None, 0, 1] * cy + D[:, None, 0, 3],
                       D[:, None, 1, 0] * cx + D[:, None, 1, 1] * cy + D[:, None, 1, 3]], dim=-1).to(dtype)  # (T - I)(cx, cy, 0, 1) in fp64
    static2 = torch.where(filled[..., None], saf, zero2) if sp["use_static_aggr"] else sf
    omg = 1.0 - probs[..., 2:3]
    dyn2 = df * omg
    if sp["non_rigid"]:
        dyn2 = static2 * omg + dyn2
    agg = torch.where(is_static[..., None], static2, dyn2)
    x = case["pc"][..., :3].to(dtype)
    z1 = torch.zeros(S, N, 1, dtype=dtype)
    f3 = lambda v: torch.cat([v, z1], dim=-1)  # noqa: E731
    out = {"x": x, "y": x + f3(sf), "w": probs[..., 0] * filled.to(dtype),
           "dis_logit": logit[0], "dis": torch.sigmoid(logit[0]), "logits": cl, "probs": probs, "staticness": probs[..., 0],
           "dynamicness": probs[..., 1], "groundness": probs[..., 2], "dyn_flow": f3(df), "stat_flow": f3(sf), "agg_flow": f3(agg),
           "saf_flow": f3(saf)}
    out = {k: torch.where(valid if v.dim() == 2 else valid[..., None], v, torch.zeros((), dtype=dtype)) for k, v in out.items()}
    out["flags"] = torch.stack([is_static, is_dyn, is_ground], dim=-1) & valid[..., None]
    return out


def decode_with_grads(case, dtype=torch.float64, subset=None, pass1=("y", "w")):
    """outputs + gradients under the case's random upstream gradients: `subset` of FLOAT_OUTS feeds pass 2 (None: all), `pass1` of (y, w)
    -> dict(out, graw1 [S,N,8], graw2 [S,N,8], gT [S,4,4] or None)"""
    raw = case["raw"].to(dtype).requires_grad_(True)
    T = case["T"].clone().requires_grad_(True)
    out = decode_ref(case, raw, T, dtype)
    up = case["upstream"]
    l1 = sum((out[k] * up[k].to(dtype)).sum() for k in pass1)
    # (y with static_flow_zero does not depend on raw at all)
    (g1,) = torch.autograd.grad(l1, raw, retain_graph=True) if torch.is_tensor(l1) and l1.requires_grad else (torch.zeros_like(raw),)
    names = FLOAT_OUTS if subset is None else subset
    l2 = sum((out[k] * up[k].to(dtype)).sum() for k in names)
    g2, gT = torch.autograd.grad(l2, [raw, T], allow_unused=True)
    return dict(out={k: v.detach() for k, v in out.items()}, graw1=g1, graw2=torch.zeros_like(raw) if g2 is None else g2, gT=gT)


def _masked_mean(terms, valid, dtype):
    t = torch.where(valid, terms, torch.zeros((), dtype=terms.dtype))
    if dtype == torch.float32:  # the header: fp32 terms, fp64 sum, fp32 sum / fp32 count
        return t.double().sum().float() / valid.sum().float()
    return t.sum() / valid.sum()


def static_loss_ref(case, flow, weight, dtype=torch.float64):
    """static_points_loss + masked mean (slim_loss_adaptor.py:55-91, :176-184): est = (T p)_xyz - p in fp64, then `dtype`"""
    p = case["pc"][..., :3].double()
    T = case["T"]
    moved = (p[:, :, None, :] * T[:, None, :3, :3]).sum(dim=-1) + T[:, None, :3, 3]
    est = (moved - p).to(dtype)
    rows = (weight[..., None] * (est - flow) ** 2).mean(dim=-1)
    return _masked_mean(rows, case["valid"], dtype)


def static_loss_with_grads(case, dtype=torch.float64):
    flow, weight = case["flow"].to(dtype).requires_grad_(True), case["weight"].to(dtype).requires_grad_(True)
    mean = static_loss_ref(case, flow, weight, dtype)
    gf, gw = torch.autograd.grad(mean * case["g_mean"].to(mean.dtype), [flow, weight])
    return dict(mean=mean.detach(), gflow=gf, gweight=gw)


def nploss_ref(case, flow, dtype=torch.float64):
    """knn_wrapper.py:58-135 + huber_delta (:11-49) + the masked mean, neighbours in POINT order (case["nbr"]); a neighbour index outside
    [0, n_b) reads row 0 of the sample's cloud, as the kernels do -> (mean, dist_sqr [S,N] with 0 at invalid rows, per-row loss)"""
    sp = case["spec"]
    q = case["pc"][..., :3].to(dtype) + flow
    nbr = case["nbr"]
    safe = torch.where((nbr >= 0) & (nbr < sp["n_b"]), nbr, torch.zeros_like(nbr))
    nn = torch.gather(case["cloud_b"][..., :3].to(dtype), 1, safe[..., None].expand(-1, -1, 3))
    d2 = ((nn - q) ** 2).sum(dim=-1)
    e = [torch.tensor(v, dtype=torch.float32).to(dtype) for v in BEV_EXTENT]
    min_fov = torch.minimum(torch.minimum(q[..., 0] - e[0], q[..., 1] - e[1]), torch.minimum(e[2] - q[..., 0], e[3] - q[..., 1]))
    w = torch.ones_like(d2)
    if sp["fov_mode"] == 1:
        w = (min_fov > 0).to(dtype)
    elif sp["fov_mode"] == 2:
        w = ((min_fov > 0) & (d2 < min_fov ** 2)).to(dtype)
    delta = torch.tensor(sp["delta"], dtype=torch.float32).to(dtype)
    if sp["delta"] == 0.0:
        nz = d2 != 0
        l = torch.where(nz, d2, torch.ones_like(d2)).sqrt() * nz.to(dtype)  # gradient-safe sqrt
    else:
        dd = delta * delta
        l = torch.clamp(d2, max=dd) / (2.0 * delta) + torch.clamp(d2, min=dd).sqrt() - delta
    loss = l * w
    valid = case["valid"]
    return _masked_mean(loss, valid, dtype), torch.where(valid, d2, torch.zeros((), dtype=dtype)), loss


def nploss_with_grads(case, dtype=torch.float64, with_gd2=None):
    flow = case["flow"].to(dtype).requires_grad_(True)
    mean, d2, loss = nploss_ref(case, flow, dtype)
    with_gd2 = case["spec"]["with_gd2"] if with_gd2 is None else with_gd2
    total = mean * case["g_mean"].to(mean.dtype)
    if with_gd2:
        total = total + (d2 * case["g_d2"].to(dtype)).sum()
    (gf,) = torch.autograd.grad(total, flow)
    return dict(mean=mean.detach(), d2=d2.detach(), loss=loss.detach(), gflow=gf)


def knn_queries_ref(case, flows):
    """knn_loss.py:44-58, knn_wrapper.py:170,186-190: query[t,s,j] = pc[s,o[j]] + flow_t[s,o[j]] in fp32, NaN at invalid rows,
    o = order[s % clouds] (identity without an order)"""
    sp = case["spec"]
    S, N = sp["S"], sp["N"]
    pc = case["pc"][..., :3]
    o = torch.arange(N)[None].expand(S, N) if case["order"] is None else case["order"][torch.arange(S) % sp["clouds"]]
    ok = torch.gather(case["valid"], 1, o)
    out = []
    for f in flows:
        q = torch.gather(pc + f, 1, o[..., None].expand(-1, -1, 3))
        out.append(torch.where(ok[..., None], q, torch.full((), float("nan"))))
    return torch.stack(out, dim=0)


def extrema_ref(x, c):
    """[max_0..max_{c-1} | min_0..min_{c-1}] over the rows of a [rows, stride] map"""
    return torch.cat([x[:, :c].amax(dim=0), x[:, :c].amin(dim=0)])


# ---- decode cases -----------------------------------------------------------------------------------------------------------------------
CELL_FILLED, CELL_UNFILLED, CELL_TIE_FILLED, CELL_TIE_UNFILLED = 0, 1, 2, 3


def _margins_ok(case):
    """per valid row: both decisions of the fp64 restatement are MARGIN clear, or tied exactly in a way fp32 ties too"""
    with torch.no_grad():
        out = decode_ref(case, case["raw"].double(), case["T"])
        out32 = decode_ref(case, case["raw"], case["T"], torch.float32)
    thr = float(torch.tensor(case["spec"]["thr"], dtype=torch.float32))
    p, p32 = out["probs"], out32["probs"].double()
    dyn_ok = ((p[..., 1] - thr).abs() > MARGIN) | ((p[..., 1] == thr) & (p32[..., 1] == thr))
    if thr <= 0.0:  # a probability is >= 0 in every precision
        dyn_ok = torch.ones_like(dyn_ok)
    sg_ok = ((p[..., 0] - p[..., 2]).abs() > MARGIN) | ((out["logits"][..., 0] == out["logits"][..., 2]) & (p32[..., 0] == p32[..., 2]))
    sg_ok = sg_ok | (p[..., 1] >= thr)  # a dynamic row is neither static nor ground, whatever p_static and p_ground are
    return (dyn_ok & sg_ok) | ~case["valid"]


@functools.lru_cache(maxsize=None)
def decode_case(cid):
    sp = dict(decode_specs()[cid])
    g = torch.Generator().manual_seed(sp["seed"])
    S, N, cells = sp["S"], sp["N"], H * W
    reduced = sp.get("reduced", False)
    cls = torch.zeros(S, cells, dtype=torch.int64)
    for s in range(S):
        perm = torch.randperm(cells, generator=g)
        cls[s, perm[:8]] = CELL_UNFILLED
        cls[s, perm[8:10]] = CELL_TIE_UNFILLED
        cls[s, perm[10:13]] = CELL_TIE_FILLED
    filled = ((cls == CELL_FILLED) | (cls == CELL_TIE_FILLED)).view(S, H, W)
    net = torch.randn(S, cells, 8, generator=g) * _CH_SCALE
    valid = torch.rand(S, N, generator=g) > 0.1
    valid[:, 0] = valid[:, N - 1] = valid[:, N // 2] = False
    cell = torch.zeros(S, N, dtype=torch.int64)
    for s in range(S):
        walk = torch.randperm(cells, generator=g)
        cell[s] = walk[(torch.cumsum(valid[s].long(), 0) - 1).clamp(min=0) % cells]  # the valid rows visit every cell in turn
    if reduced:  # 4 rows: invalid, tie in a filled pillar, unfilled, filled
        valid = torch.tensor([[False], [True], [True], [True]])
        for s, want in ((1, CELL_TIE_FILLED), (2, CELL_UNFILLED), (3, CELL_FILLED)):
            cell[s, 0] = int((cls[s] == want).nonzero()[0])
    lin = torch.where(valid, torch.arange(S)[:, None] * cells + cell, torch.full((), -1)).to(torch.int32).reshape(-1)
    cx, cy = (v.view(S, N) for v in cell_centres(lin))
    pc = torch.rand(S, N, sp["pc_stride"], generator=g) * 2.0 - 1.0
    pc[..., 0] = cx.float() + pc[..., 0] * 0.4 * EXT_SPAN[0] / H
    pc[..., 1] = cy.float() + pc[..., 1] * 0.4 * EXT_SPAN[1] / W
    T = torch.eye(4, dtype=torch.float64)[None].repeat(S, 1, 1)
    T[:, :3] += 0.05 * torch.randn(S, 3, 4, generator=g, dtype=torch.float64)  # every entry distinct: no symmetry hides a swap
    up = {k: torch.randn((S, N) + shape, generator=g) for k, shape in
          [("y", (3,)), ("w", ())] + [(k, (3,) if k in ("logits", "probs") or k.endswith("_flow") else ()) for k in FLOAT_OUTS]}
    case = dict(spec=sp, valid=valid, lin=lin, filled=filled, pc=pc.contiguous(), T=T, upstream=up, cell_class=cls)
    case["filled_pt"] = filled.view(S, cells).gather(1, cell) & valid
    for _ in range(50):
        tie = (cls == CELL_TIE_FILLED) | (cls == CELL_TIE_UNFILLED)
        net[..., 3] = torch.where(tie, net[..., 1], net[..., 3])
        net[..., 2] = torch.where(tie, net[..., 1] - 12.0, net[..., 2])
        case["net"] = net.view(S, H, W, 8).contiguous()
        case["raw"] = torch.where(valid[..., None], net.gather(1, cell[..., None].expand(-1, -1, 8)), torch.zeros(())).contiguous()
        case["extrema"] = (net[..., :4].amax(dim=(0, 1)), net[..., :4].amin(dim=(0, 1)))
        bad = ~_margins_ok(case)
        if not bool(bad.any()):
            break
        for s, c in {(int(s), int(cell[s, i])) for s, i in bad.nonzero().tolist()}:  # redraw the logits of the pillars that sit too close
            net[s, c, :4] = torch.randn(4, generator=g) * _CH_SCALE[:4]
    else:
        raise AssertionError("no margin-clear draw for " + cid)
    pt_cls = cls.gather(1, cell)
    tie_pt = ((pt_cls == CELL_TIE_FILLED) | (pt_cls == CELL_TIE_UNFILLED)) & valid
    case["classes"] = {"invalid": ~valid, "unfilled": valid & ~case["filled_pt"], "filled": valid & case["filled_pt"], "tie": tie_pt}
    return case


def slim_cfg(sp):
    """the SLIM configuration a decode spec stands for (DecodeMeta and HeadDecoder read it)"""
    from liso_amd.utils.config import default_cfg

    cfg = default_cfg(grid=32, bev_range_m=20.0).SLIM
    om = cfg.model.output_modification
    om.disappearing_logit, om.static_logit, om.dynamic_logit, om.ground_logit = sp["modes"]
    om.static_flow = "zero" if sp["static_flow_zero"] else "net"
    om.dynamic_flow = "zero" if sp["dynamic_flow_zero"] else "net"
    om.dynamic_flow_grad_scale = sp["dyn_grad_scale"]
    cfg.model.use_static_aggr_flow_for_aggr_flow = sp["use_static_aggr"]
    cfg.model.u_net.final_scale = 1
    return cfg


def decode_id(prefix):
    (cid,) = [c for c in decode_specs() if c.startswith(prefix + "-")]
    return cid


# Backward calls with only some upstream gradients (the others reach the kernels as NULL): (case, outputs feeding pass 2, outputs feeding
# pass 1).  The first three are the transform gradient through saf_flow alone and, with use_static_aggr, through agg_flow alone.
SUBSET_RUNS = [("mode00", ("saf_flow",), ("y",)), ("mode01", ("agg_flow",), ("w",)), ("mode03", ("agg_flow",), ("y", "w")),
               ("mode04", ("probs", "dyn_flow"), ("w",)), ("mode07", ("dis", "staticness", "agg_flow"), ("y",)),
               ("mode02", ("agg_flow", "groundness"), ("w",)), ("mode12", ("logits", "dis_logit", "stat_flow"), ("y", "w"))]


@functools.lru_cache(maxsize=None)
def decode_reference(cid, subset=None, pass1=("y", "w")):
    return decode_with_grads(decode_case(cid), torch.float64, subset, pass1)


# ---- loss cases ---------------------------------------------------------------------------------------------------------------------
BIG_N = 66000
BIG_ROW = 512 * 256  # first row of the second grid-stride sweep
# dominant terms: a stride one short visits row 131 071 twice, a stride one long never visits row 131 072, a missing second sweep loses the last row
BIG_PLANTED = (BIG_ROW - 1, BIG_ROW, 2 * BIG_N - 1)


def _valid_rows(S, N, g, p=0.1):
    valid = torch.rand(S, N, generator=g) > p
    if N >= 3:
        valid[:, 0] = valid[:, N - 1] = valid[:, N // 2] = False
    return valid


def static_specs():
    return {"static-4x257-stride4": dict(S=4, N=257, pc_stride=4, seed=301), "static-1x1000-stride3": dict(S=1, N=1000, pc_stride=3, seed=302),
            "static-1x256-stride3": dict(S=1, N=256, pc_stride=3, seed=303), "static-4x1-stride4": dict(S=4, N=1, pc_stride=4, seed=304),
            "static-1x255-no_valid_row": dict(S=1, N=255, pc_stride=3, seed=305, none_valid=True),
            "static-big-2x66000-terms_at_131071_131072_and_last": dict(S=2, N=BIG_N, pc_stride=3, seed=306, big=True)}


@functools.lru_cache(maxsize=None)
def static_case(cid):
    sp = dict(static_specs()[cid])
    g = torch.Generator().manual_seed(sp["seed"])
    S, N = sp["S"], sp["N"]
    pc = (torch.rand(S, N, sp["pc_stride"], generator=g) - 0.5) * torch.tensor([20.0, 56.0, 3.0, 1.0][:sp["pc_stride"]])
    T = torch.eye(4, dtype=torch.float64)[None].repeat(S, 1, 1)
    T[:, :3] += 0.02 * torch.randn(S, 3, 4, generator=g, dtype=torch.float64)
    valid = _valid_rows(S, N, g) if N > 1 else torch.tensor([[True], [False], [True], [True]])
    if sp.get("none_valid"):
        valid = torch.zeros(S, N, dtype=torch.bool)
    case = dict(spec=sp, pc=pc.contiguous(), T=T, valid=valid, weight=torch.rand(S, N, generator=g), g_mean=torch.randn((), generator=g) + 2.0)
    p = pc[..., :3].double()
    est = ((p[:, :, None, :] * T[:, None, :3, :3]).sum(-1) + T[:, None, :3, 3] - p).float()
    flow = est + 0.1 * torch.randn(S, N, 3, generator=g)
    if sp.get("big"):
        valid[:] = torch.rand(S, N, generator=g) > 0.02
        for row in BIG_PLANTED:
            s, i = divmod(row, N)
            valid[s, i] = True
            flow[s, i] += 50.0
            case["weight"][s, i] = 0.8
        case["planted_rows"] = BIG_PLANTED
    case["flow"] = flow.contiguous()
    return case


@functools.lru_cache(maxsize=None)
def static_reference(cid):
    return static_loss_with_grads(static_case(cid))


def nploss_specs():
    sp = {}
    n_of = {0: 257, 1: 1000, 2: 255}
    for k, (fov, delta) in enumerate(itertools.product((0, 1, 2), (0.0, 0.1, 0.3))):
        S = 4 if k % 2 == 0 else 1
        N = n_of[fov] if delta != 0.1 else 256
        sp["np-fov%d-delta%g-%dx%d-%s-%s" % (fov, delta, S, N, "order" if k % 3 != 1 else "identity", "gd2" if k % 2 == 0 else "no_gd2")] = dict(
            S=S, clouds=2 if S == 4 else 1, N=N, n_b=N + 13, fov_mode=fov, delta=delta, order=k % 3 != 1, with_gd2=k % 2 == 0,
            pc_stride=3 + k % 2, cb_stride=4 - k % 2, seed=400 + k)
    sp["np-fov1-delta0.1-4x1-order"] = dict(S=4, clouds=2, N=1, n_b=5, fov_mode=1, delta=0.1, order=True, with_gd2=True, pc_stride=3, cb_stride=4, seed=420)
    sp["np-fov2-delta0.3-4x256-no_valid_row"] = dict(S=4, clouds=2, N=256, n_b=100, fov_mode=2, delta=0.3, order=True, with_gd2=True, pc_stride=4,
                                                   cb_stride=3, seed=421, none_valid=True)
    for fov, delta, seed in ((0, 0.0, 430), (0, 0.3, 431)):
        sp["np-big-delta%g-2x66000-terms_at_131071_131072_and_last" % delta] = dict(S=2, clouds=2, N=BIG_N, n_b=1000, fov_mode=fov, delta=delta, order=False,
                                                                             with_gd2=False, pc_stride=3, cb_stride=3, seed=seed, big=True)
    return sp


NP_REL = 1e-3  # every decision of the nearest-point loss is this clear (relative) of its threshold on the rows that stay valid


@functools.lru_cache(maxsize=None)
def nploss_case(cid):
    sp = dict(nploss_specs()[cid])
    g = torch.Generator().manual_seed(sp["seed"])
    S, N, n_b, clouds = sp["S"], sp["N"], sp["n_b"], sp["clouds"]
    lo = torch.tensor([BEV_EXTENT[0] - 2.0, BEV_EXTENT[1] - 2.0, -1.5])
    hi = torch.tensor([BEV_EXTENT[2] + 2.0, BEV_EXTENT[3] + 2.0, 1.5])
    cb = torch.rand(S, n_b, sp["cb_stride"], generator=g)
    cb[..., :3] = lo + cb[..., :3] * (hi - lo)  # some reference points outside the field of view, some just inside its border
    nbr = torch.randint(0, n_b, (S, N), generator=g)
    valid = _valid_rows(S, N, g) if N > 1 else torch.tensor([[True], [False], [True], [True]])
    planted = {}
    if N >= 255 and not sp.get("big"):
        for name, i, v in (("index_minus_one", 5, -1), ("index_n_b", 9, n_b)):  # both read row 0
            nbr[:, i] = v
            valid[:, i] = True
            planted[name] = i
    safe = torch.where((nbr >= 0) & (nbr < n_b), nbr, torch.zeros_like(nbr))
    nn = torch.gather(cb[..., :3], 1, safe[..., None].expand(-1, -1, 3))
    dist = torch.tensor([0.03, 0.2, 1.0, 3.0])[torch.randint(0, 4, (S, N), generator=g)]
    if sp.get("big"):
        dist = torch.full((S, N), 0.2)
    direction = torch.nn.functional.normalize(torch.randn(S, N, 3, generator=g) * torch.tensor([1.0, 1.0, 0.2]), dim=-1)
    flow = 0.3 * torch.randn(S, N, 3, generator=g)
    pc = torch.rand(S, N, sp["pc_stride"], generator=g)
    pc[..., :3] = nn - direction * dist[..., None] - flow
    if N >= 255 and not sp.get("big"):
        for i in (17, 33, N - 2):  # queries exactly on their neighbour
            flow[:, i] = 0.0
            pc[:, i, :3] = nn[:, i]
            valid[:, i] = True
        planted["d2_zero"] = (17, 33, N - 2)
    if sp.get("big"):
        valid = torch.rand(S, N, generator=g) > 0.02
        for row in BIG_PLANTED:
            s, i = divmod(row, N)
            valid[s, i] = True
            pc[s, i, :3] = nn[s, i] - torch.tensor([3000.0, 4000.0, 0.0]) - flow[s, i]
    order = torch.stack([torch.randperm(N, generator=g) for _ in range(clouds)]) if sp["order"] else None
    case = dict(spec=sp, pc=pc.contiguous(), cloud_b=cb.contiguous(), nbr=nbr, flow=flow.contiguous(), order=order, planted=planted,
                g_mean=torch.randn((), generator=g) + 2.0, g_d2=torch.randn(S, N, generator=g),
                flows=[flow] + [0.3 * torch.randn(S, N, 3, generator=g) for _ in range(2)])
    # rows whose decisions are not clear of their thresholds in fp64 leave the valid set (drawn again would do the same)
    with torch.no_grad():
        q = pc[..., :3].double() + flow.double()
        d2 = ((nn.double() - q) ** 2).sum(-1)
        e = [float(torch.tensor(v, dtype=torch.float32)) for v in BEV_EXTENT]
        mf = torch.minimum(torch.minimum(q[..., 0] - e[0], q[..., 1] - e[1]), torch.minimum(e[2] - q[..., 0], e[3] - q[..., 1]))
        dd = float(torch.tensor(sp["delta"], dtype=torch.float32)) ** 2
        clear = (mf.abs() > NP_REL) & ((d2 - mf ** 2).abs() > NP_REL * torch.maximum(d2, mf ** 2))
        if dd > 0:
            clear &= (d2 - dd).abs() > NP_REL * dd
        clear &= (d2 == 0) | (d2 > 1e-6)
    valid = valid & clear
    if sp.get("none_valid"):
        valid = torch.zeros(S, N, dtype=torch.bool)
    case["valid"] = valid
    case["clear"] = clear
    case["d2_64"], case["min_fov_64"] = d2, mf
    # index in QUERY order: index[s, j] answers point order[s % clouds][j]
    if order is None:
        case["index"] = nbr.clone()
    else:
        case["index"] = torch.gather(nbr, 1, order[torch.arange(S) % clouds])
    return case


@functools.lru_cache(maxsize=None)
def nploss_reference(cid, with_gd2=None):
    return nploss_with_grads(nploss_case(cid), torch.float64, with_gd2)


def extrema_specs():
    """(rows, stride, channels, first channel): small odd shapes, the vector path (4 channels, stride % 4 == 0, 16-byte aligned), the scalar
    path, and two sweeps of the 512 x 256 grid with the maximum in the last row and the minimum in row 131 072"""
    return {"ext-1x8-c4": (1, 8, 4, 0), "ext-255x8-c4": (255, 8, 4, 0), "ext-257x5-c3": (257, 5, 3, 1), "ext-1000x4-c4": (1000, 4, 4, 0),
            "ext-256x8-c4-unaligned": (256, 8, 4, 1), "ext-big-132000x8-c4-vector": (2 * BIG_N, 8, 4, 0), "ext-big-132000x5-c3-scalar": (2 * BIG_N, 5, 3, 1)}


@functools.lru_cache(maxsize=None)
def extrema_case(cid):
    rows, stride, c, off = extrema_specs()[cid]
    g = torch.Generator().manual_seed(500 + rows + stride)
    buf = torch.randn(rows * stride + 8, generator=g)
    x = buf[off:off + rows * stride].view(rows, stride)
    if rows > BIG_ROW:
        x[rows - 1, :c] = 40.0 + torch.arange(c)
        x[BIG_ROW, :c] = -40.0 - torch.arange(c)
    return dict(buf=buf, off=off, rows=rows, stride=stride, c=c, ref=extrema_ref(x, c))


# ---- comparison -----------------------------------------------------------------------------------------------------------------------
OUT_CLASS = {"x": "out_copy", "dis_logit": "out_copy", "stat_flow": "out_copy", "dyn_flow": "out_copy", "logits": "out_logit", "dis": "out_prob",
             "probs": "out_prob", "staticness": "out_prob", "dynamicness": "out_prob", "groundness": "out_prob", "w": "out_prob", "y": "out_flow",
             "agg_flow": "out_flow", "saf_flow": "out_flow"}


def class_errors(got, ref, classes):
    """{row class: (max |got - ref|, max |ref|)} over the rows of each non-empty class; got, ref [S,N,...]"""
    res = {}
    d = (got.double() - ref.double()).abs()
    for name, m in classes.items():
        if bool(m.any()):
            res[name] = (float(d[m].max()), float(ref[m].abs().max()))
    return res


def rel_error(err, scale):
    return err / max(scale, FLOOR)


def _merge(res, qclass, got, ref, classes):
    for name, (e, s) in class_errors(got, ref, classes).items():
        key = qclass + "/" + name
        res[key] = max(res.get(key, 0.0), rel_error(e, s))


def _scalar(res, key, got, ref):
    res[key] = max(res.get(key, 0.0), rel_error(abs(float(got) - float(ref)), abs(float(ref))))


def compare_decode(case, got, ref):
    """{"quantity class/row class": worst relative error} of whatever `got` holds: out {name: tensor}, graw1, graw2, gT"""
    res, cl = {}, case["classes"]
    for k, v in got.get("out", {}).items():
        if k in OUT_CLASS:
            _merge(res, OUT_CLASS[k], v, ref["out"][k], cl)
    for p in ("1", "2"):
        if got.get("graw" + p) is not None:
            _merge(res, "grad%s_logit" % p, got["graw" + p][..., :4], ref["graw" + p][..., :4], cl)
            _merge(res, "grad%s_flow" % p, got["graw" + p][..., 4:], ref["graw" + p][..., 4:], cl)
    if got.get("gT") is not None:
        _merge(res, "grad_trafo", got["gT"], ref["gT"], {"all": torch.ones(got["gT"].shape[0], dtype=torch.bool)})
    return res


def loss_classes(case):
    return {"valid": case["valid"], "invalid": ~case["valid"]}


def compare_static(case, got, ref):
    res = {}
    if bool(case["valid"].any()):
        _scalar(res, "mean/static", got["mean"], ref["mean"])
    for k in ("gflow", "gweight"):
        if got.get(k) is not None:
            _merge(res, "grad_static", got[k], ref[k], loss_classes(case))
    return res


def compare_nploss(case, got, ref):
    res = {}
    if bool(case["valid"].any()) and got.get("mean") is not None:
        _scalar(res, "mean/np", got["mean"], ref["mean"])
    if got.get("d2") is not None:
        _merge(res, "np_row", got["d2"], ref["d2"], loss_classes(case))
    if got.get("loss") is not None:
        _merge(res, "np_row", got["loss"], ref["loss"], {"valid": case["valid"]})
    if got.get("gflow") is not None:
        _merge(res, "grad_np", got["gflow"], ref["gflow"], loss_classes(case))
    return res


def zeros_kept(got, ref):
    """wherever the fp64 restatement is exactly zero (invalid rows, dead channels, gradients behind a forced or overwritten value), so is `got`"""
    return bool((got[ref == 0] == 0).all())


def fp32_error_table():
    """the fp32 restatement against the fp64 one over every case -> {key: worst relative error}; flags must agree exactly"""
    worst = {}

    def fold(res):
        for k, v in res.items():
            worst[k] = max(worst.get(k, 0.0), v)

    for cid in decode_specs():
        case, ref = decode_case(cid), decode_reference(cid)
        got = decode_with_grads(case, torch.float32)
        assert torch.equal(got["out"]["flags"], ref["out"]["flags"]), cid
        fold(compare_decode(case, got, ref))
    for prefix, subset, pass1 in SUBSET_RUNS:
        case = decode_case(decode_id(prefix))
        got = decode_with_grads(case, torch.float32, subset, pass1)
        fold(compare_decode(case, dict(got, out={}), decode_reference(decode_id(prefix), subset, pass1)))
    for cid in static_specs():
        case = static_case(cid)
        fold(compare_static(case, static_loss_with_grads(case, torch.float32), static_reference(cid)))
    for cid in nploss_specs():
        case = nploss_case(cid)
        fold(compare_nploss(case, nploss_with_grads(case, torch.float32), nploss_reference(cid)))
    return worst
