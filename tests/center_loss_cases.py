"""Cases and fp64 references of the detector's loss and target kernels (liso_amd/csrc/detector_loss.hip); nothing here needs a GPU or
calls a project kernel.  tests/test_center_loss_cases.py anchors the two references on the CPU (the project's torch-op path in fp64,
the reference project's fixtures); tests/test_gpu_center_loss_edges.py and tests/test_gpu_target_render_edges.py hold the kernels to
them.

loss_fp64      activations, decode, the four CenterPoint terms and the unit-circle regulariser as elementary fp64 torch operations,
               differentiable by autograd, over the STORED fp32 inputs.
targets_fp64   the target renderer in fp64 from the fp32 boxes, plus the two per-cell flags that say where fp32 may legitimately
               pick another winner ("winner uncertain") or land on the other side of the occupancy threshold ("threshold uncertain").

Conditions the case builders guarantee, asserted on the CPU (no kernel output enters any of them):
  * every selected centre keeps |prediction - target| >= 1e-4 in pos and dims: the L1 kinks lie a hundred fp32 roundings of a 50 m
    coordinate away, so sgn() is the same in fp32 and fp64 (planted exact equalities of the rotation vector involve no arithmetic);
  * the first centre of a case holds raw pos and dims in [-1, 1]: the gradient bound is relative to a class's largest reference value,
    and `1 - tanh^2` of a saturated cell is all cancellation -- a class of one or three centres needs one well-conditioned member;
  * cell 0, the last cell and (where it exists) cell 512 * 256 - 1 are selected centres, so a cell that a wrong grid stride counts twice
    or never weighs 1 / #centres of three loss terms, not 1 / #cells of one;
  * per target case at most 2 cells are flagged uncertain."""
import math

import numpy as np
import torch
import torch.nn.functional as F

HEADS = ("pos", "dims", "rot", "probs")
TERMS = ("probs", "rot", "dims", "pos", "reg", "total")
KINK_MARGIN = 1e-4


def f32(v):
    """the value an fp32 ABI field receives"""
    return float(np.float32(v))


def centres_f32(h, w, rng):
    """[H,W,2] cell centres ((i + 0.5) / n) * range - range / 2, fp64 arithmetic rounded to fp32 (what the kernels are handed / do)"""
    ys = ((torch.arange(h, dtype=torch.float64) + 0.5) / h) * rng[0] - 0.5 * rng[0]
    xs = ((torch.arange(w, dtype=torch.float64) + 0.5) / w) * rng[1] - 0.5 * rng[1]
    return torch.stack(torch.meshgrid(ys, xs, indexing="ij"), -1).float()


# ---- loss ----------------------------------------------------------------------------------------------------------------------------------
def loss_fp64(raw, gt, center_mask, ignore_mask, rot_weights, centers, res, z_prior, sup_weight, rot_reg_weight):
    """raw / gt: dicts of [B,H,W,3|3|2|1] (raw in fp64 and, for gradients, requiring grad); center_mask / ignore_mask [B,H,W] bool,
    rot_weights [B,H,W] -- None: nothing ignored / weights of one; centers [H,W,2]; res = range / (H, W).
    -> dict of the five terms, the total and the decoded maps"""
    pos, dims, rot, logit = (raw[k].double() for k in HEADS)
    g = {k: gt[k].double() for k in HEADS}
    cen = center_mask.bool()
    ign = torch.zeros_like(cen) if ignore_mask is None else ignore_mask.bool()
    w = torch.ones(cen.shape, dtype=torch.float64) if rot_weights is None else rot_weights.double().reshape(cen.shape)
    tp = torch.tanh(pos)
    sp = F.softplus(dims, beta=1.0, threshold=20.0)
    c = centers.double()
    dec = torch.stack([c[None, ..., 0] + 0.5 * res[0] * tp[..., 0], c[None, ..., 1] + 0.5 * res[1] * tp[..., 1],
                       z_prior[0] + 0.5 * (tp[..., 2] + 1.0) * (z_prior[1] - z_prior[0])], -1)
    num_pos = max(float(cen.sum()), 1.0)
    sel = cen & ~ign
    x = logit[..., 0]
    pp, pn = torch.sigmoid(x), torch.sigmoid(-x)
    om = 1.0 - g["probs"][..., 0]
    f_pos = 0.5 * pn ** 2 * F.logsigmoid(x)
    f_neg = 0.5 * pp ** 2 * om ** 4 * F.logsigmoid(-x)
    l_probs = -(f_pos[sel].sum() + f_neg[~cen & ~ign].sum()) / num_pos
    wc = w.clamp(min=0.1)[sel]
    l_rot = 10.0 * (wc[:, None] * (rot[sel] - g["rot"][sel]).abs()).sum() / max(float(wc.sum()), 1.0)
    n_el = max(3.0 * float(sel.sum()), 1.0)
    l_dims = (sp[sel] - g["dims"][sel]).abs().sum() / n_el / num_pos
    l_pos = (dec[sel] - g["pos"][sel]).abs().sum() / n_el / num_pos
    l_reg = ((torch.linalg.vector_norm(rot, dim=-1) - 1.0) ** 2).mean()  # (vector_norm: subgradient 0 at a zero vector)
    total = sup_weight * (l_probs + l_rot + l_dims + l_pos) + rot_reg_weight * l_reg
    return {"probs": l_probs, "rot": l_rot, "dims": l_dims, "pos": l_pos, "reg": l_reg, "total": total,
            "dec": {"pos": dec, "dims": sp, "rot": rot, "probs": logit}}


def loss_reference(case, upstream=1.0):
    """terms (floats) and raw-map gradients (fp64 [B,H,W,C]) of `upstream * total` for a case of loss_case()"""
    raw = {k: case["raw"][k].double().requires_grad_(True) for k in HEADS}
    out = loss_fp64(raw, case["gt"], case["center_mask"], case["ignore"], case["rot_w"], case["centers"], case["res"], case["z_prior"],
                    case["sup_weight"], case["reg_weight"])
    grads = torch.autograd.grad(out["total"] * upstream, [raw[k] for k in HEADS])
    return {k: float(out[k].detach()) for k in TERMS}, dict(zip(HEADS, grads))


def cell_classes(case):
    """the three classes a gradient is compared in: selected centre, non-ignored non-centre, ignored"""
    cen = case["center_mask"]
    ign = torch.zeros_like(cen) if case["ignore"] is None else case["ignore"]
    return {"selected": cen & ~ign, "background": ~cen & ~ign, "ignored": ign}


def class_errors(got, ref, classes):
    """{class: (max |got - ref|, max |ref|)} over the cells of each non-empty class; inf where got is not finite"""
    out = {}
    for name, m in classes.items():
        if not bool(m.any()):
            continue
        a, b = got.double()[m], ref.double()[m]
        d = (a - b).abs()
        d = torch.where(torch.isfinite(a), d, torch.full_like(d, float("inf")))
        out[name] = (float(d.max()), float(b.abs().max()))
    return out


GEOMETRIES = [(3, 5, 7), (1, 16, 16), (1, 257, 1), (2, 48, 80), (1, 129, 129), (3, 256, 192)]
MASKS = ("M0", "M1", "M2", "M3", "M4", "M5", "M6")
MAIN = (2, 48, 80)
SECOND_TRIP_CELL = 512 * 256 - 1  # the last cell of the first trip of a 512-block launch
EDGE_LOGITS = (40.0, -40.0, 88.0, -88.0, 104.0, -104.0, None)
EDGE_DIMS = (20.0, 20.5, 25.0, -60.0, -104.0, None)
EDGE_POS = (0.0, 12.0, -12.0, None)


def bev_range(h, w):
    return (60.0, 100.0) if h != w else (50.0, 50.0)


def loss_case(geometry, mask="M1", edges=False, reg_weight=None):
    """CPU tensors of one loss case.  mask: M0 .. M6 of MASKS; edges: plant the saturating values at every 7th cell from cell 3 on"""
    B, H, W = geometry
    n = B * H * W
    g = torch.Generator().manual_seed(1000 * MASKS.index(mask) + 7 * n + (500 if edges else 0))
    rng = bev_range(H, W)
    res = (f32(rng[0] / H), f32(rng[1] / W))
    z_prior = (-1.5, -0.5) if mask in ("M0", "M2") else (-2.25, 0.5)
    centers = centres_f32(H, W, rng)
    raw = {"pos": 3.0 * torch.randn(B, H, W, 3, generator=g), "dims": 3.0 * torch.randn(B, H, W, 3, generator=g),
           "rot": 3.0 * torch.randn(B, H, W, 2, generator=g), "probs": 3.0 * torch.randn(B, H, W, 1, generator=g)}
    # ---- masks
    perm = [int(v) for v in torch.randperm(n, generator=g)]
    forced = [0, n - 1] + ([SECOND_TRIP_CELL] if n > SECOND_TRIP_CELL + 1 else [])
    count = {"M2": 0, "M4": 3, "M5": 1}.get(mask, min(max(3, round(0.04 * n)), 200))
    cells = (forced + [p for p in perm if p not in forced])[:count]
    cen = torch.zeros(n, dtype=torch.bool)
    cen[cells] = True
    ign = torch.rand(n, generator=g) < 0.1
    rot_w = 2.0 * torch.rand(n, generator=g)
    if mask == "M1" and not edges:
        ign[cells] = False
        ign[cells[3::4]] = True      # ignored centres: they count in num_pos and nowhere else
    elif mask == "M3":
        ign[cells] = True
    elif mask in ("M4", "M5"):
        ign[cells] = False
        if mask == "M4":
            rot_w[cells] = 0.0
    elif mask == "M6":
        ign[:] = True
    # ---- targets
    ang = 2.0 * math.pi * torch.rand(n, generator=g)
    gt_rot = torch.stack([torch.sin(ang), torch.cos(ang)], -1)
    gt_dims = 0.5 + 4.5 * torch.rand(n, 3, generator=g)
    off = (0.5 + 2.5 * torch.rand(n, 2, generator=g)) * torch.where(torch.rand(n, 2, generator=g) < 0.5, -1.0, 1.0)
    side = torch.rand(n, generator=g) < 0.5
    dz = 0.25 + 0.75 * torch.rand(n, generator=g)
    gt_z = torch.where(side, z_prior[1] + dz, z_prior[0] - dz)
    gt_pos = torch.cat([centers.reshape(1, H * W, 2).expand(B, -1, -1).reshape(n, 2) + off, gt_z[:, None]], -1)
    gt_probs = torch.rand(n, generator=g)
    flat = {k: v.reshape(n, -1) for k, v in raw.items()}
    if edges:
        planted = list(range(3, n, 7))
        for k, i in enumerate(planted):
            cls = k % 3  # 0 selected centre, 1 non-ignored non-centre, 2 ignored (every other one a centre)
            cen[i] = cls == 0 or (cls == 2 and k % 2 == 0)
            ign[i] = cls == 2
            if EDGE_LOGITS[k % 7] is not None:
                flat["probs"][i, 0] = EDGE_LOGITS[k % 7]
            for ch in range(3):
                if EDGE_DIMS[(k + ch) % 6] is not None:
                    flat["dims"][i, ch] = EDGE_DIMS[(k + ch) % 6]
                if EDGE_POS[(k + ch) % 4] is not None:
                    flat["pos"][i, ch] = EDGE_POS[(k + ch) % 4]
            if k % 4 == 0:
                flat["rot"][i] = 0.0
            elif k % 4 == 1:
                flat["rot"][i] = gt_rot[i]
            if not cen[i]:
                gt_probs[i] = float(k % 2)
        cells = [i for i in cells if bool(cen[i]) and not bool(ign[i])] or [planted[0]]
    gt_probs[cen] = 1.0
    if cells and not edges:  # one well-conditioned selected centre (module docstring)
        flat["pos"][cells[0]] = torch.tensor([0.3, -0.6, 0.9])
        flat["dims"][cells[0]] = torch.tensor([0.8, -0.4, 0.1])
    case = dict(geometry=geometry, mask=mask, edges=edges, raw={k: v.reshape(B, H, W, -1).contiguous() for k, v in flat.items()},
                gt={"pos": gt_pos.reshape(B, H, W, 3), "dims": gt_dims.reshape(B, H, W, 3), "rot": gt_rot.reshape(B, H, W, 2),
                    "probs": gt_probs.reshape(B, H, W, 1)},
                center_mask=cen.reshape(B, H, W), ignore=None if mask == "M0" else ign.reshape(B, H, W),
                rot_w=None if mask == "M0" else rot_w.reshape(B, H, W), centers=centers, range=rng, res=res, z_prior=z_prior,
                sup_weight=1.0 if mask == "M0" else 0.75,
                reg_weight=f32(reg_weight if reg_weight is not None else (0.0001 if mask == "M0" else 0.5)))
    return case


def loss_cases():
    """{id: keyword arguments of loss_case()} -- every case of the GPU test"""
    out = {}
    for geo in GEOMETRIES:
        for m in ("M0", "M1"):
            out["%s-%dx%dx%d" % ((m,) + geo)] = dict(geometry=geo, mask=m)
    for m in MASKS[2:]:
        out["%s-%dx%dx%d" % ((m,) + MAIN)] = dict(geometry=MAIN, mask=m)
    out["M1-noreg"] = dict(geometry=MAIN, mask="M1", reg_weight=0.0)
    out["edges"] = dict(geometry=MAIN, mask="M1", edges=True)
    return out


def kink_margin(case):
    """smallest |prediction - target| of pos and dims over the selected centres, in fp64 (inf without any)"""
    raw = {k: case["raw"][k].double() for k in HEADS}
    out = loss_fp64(raw, case["gt"], case["center_mask"], case["ignore"], case["rot_w"], case["centers"], case["res"], case["z_prior"],
                    case["sup_weight"], case["reg_weight"])
    sel = cell_classes(case)["selected"]
    if not bool(sel.any()):
        return float("inf")
    return min(float((out["dec"][k][sel] - case["gt"][k].double()[sel]).abs().min()) for k in ("pos", "dims"))


def case_cfg(case):
    """the project's configuration of a loss case (range, z prior, weights)"""
    from liso_amd.utils.config import default_cfg

    cfg = default_cfg(grid=64, bev_range_m=case["range"][0])
    cfg.data.bev_range_m = tuple(case["range"])
    cfg.box_prediction.position_representation.box_z_pos_prior_min = case["z_prior"][0]
    cfg.box_prediction.position_representation.box_z_pos_prior_max = case["z_prior"][1]
    cfg.loss.supervised.supervised_on_clusters.weight = case["sup_weight"]
    cfg.box_prediction.rotation_representation.regul_weight = case["reg_weight"]
    return cfg


# ---- targets -------------------------------------------------------------------------------------------------------------------------------
def cell_axis(n, rng):
    """cell centres along one axis: ((i + 0.5) / n) * range - range / 2 in fp64, rounded to fp32 as the kernel does"""
    return ((((torch.arange(n, dtype=torch.float64) + 0.5) / n) * rng - 0.5 * rng).float()).double()


def targets_fp64(box_pos, box_dims, box_rot, box_valid, grid, rng):
    """box_pos / box_dims [B,K,3], box_rot [B,K,1] fp32, box_valid [B,K] bool, grid (H, W), rng (range_x, range_y).
    -> probs [B,H,W,1], dims / pos [..3], rot [..2] = (sin, cos) in fp64, center_bool_mask [B,H,W], winner_uncertain and
    threshold_uncertain [B,H,W] bool, candidates: {(b, y, x): list of [8] attribute rows, one per near-tied heat} of the flagged cells.
    Winner uncertain: the two largest distinct heats of a cell that may carry attributes (probs > 0.01 - 1e-6) lie within 1e-5
    relative -- below the threshold every attribute is zero whoever wins, so those cells stay in the comparison."""
    B, K = box_valid.shape
    H, W = grid
    cy, cx = cell_axis(H, rng[0]), cell_axis(W, rng[1])  # (the kernel's names: "x" runs along the rows)
    probs = torch.zeros(B, H, W, dtype=torch.float64)
    attr = torch.zeros(B, H, W, 8, dtype=torch.float64)
    cmask = torch.zeros(B, H, W, dtype=torch.bool)
    win_unc = torch.zeros(B, H, W, dtype=torch.bool)
    candidates = {}
    for b in range(B):
        keep = box_valid[b].bool()  # invalid slots leave before any arithmetic
        if not bool(keep.any()):
            continue
        P, D, R = box_pos[b][keep].double(), box_dims[b][keep].double(), box_rot[b][keep].double().reshape(-1)
        c, s = torch.cos(R)[:, None, None], torch.sin(R)[:, None, None]
        dx, dy = cy[None, :, None] - P[:, 0, None, None], cx[None, None, :] - P[:, 1, None, None]
        u, v = dx * c + dy * s, -dx * s + dy * c
        heat = torch.exp(-(u * u / (0.15 * D[:, 0, None, None]) + v * v / (0.15 * D[:, 1, None, None])) / 2.0)
        heat = heat / heat.amax(dim=(1, 2), keepdim=True).clamp(min=1e-5)
        best = heat.amax(0)
        probs[b] = best
        rows = torch.cat([D, P, torch.sin(R)[:, None], torch.cos(R)[:, None]], -1)  # [k, 8]
        wins = (heat == best[None]).double()
        occ = best > 0.01
        attr[b] = torch.einsum("khw,kc->hwc", wins, rows) * occ[..., None]
        second = torch.where(heat < best[None], heat, torch.full_like(heat, -1.0)).amax(0)
        win_unc[b] = (second >= best * (1.0 - 1e-5)) & (best > 0.01 - 1e-6)
        for y, x in win_unc[b].nonzero().tolist():
            near = heat[:, y, x] >= best[y, x] * (1.0 - 1e-5)
            candidates[(b, y, x)] = [rows[near & (heat[:, y, x] == hv)].sum(0) for hv in heat[near, y, x].unique()]
        fy = torch.floor((P[:, 0] + 0.5 * rng[0]) * (H / rng[0]))
        fx = torch.floor((P[:, 1] + 0.5 * rng[1]) * (W / rng[1]))
        inside = (fy >= 0) & (fy < H) & (fx >= 0) & (fx < W)
        cmask[b, fy[inside].long(), fx[inside].long()] = True
    thr_unc = (probs - 0.01).abs() < 1e-6
    return {"probs": probs[..., None], "dims": attr[..., 0:3], "pos": attr[..., 3:6], "rot": attr[..., 6:8], "center_bool_mask": cmask,
            "winner_uncertain": win_unc, "threshold_uncertain": thr_unc, "candidates": candidates}


def _random_boxes(B, K, rng, seed, valid_share=0.75):
    g = torch.Generator().manual_seed(seed)
    r = torch.tensor(rng)
    pos = torch.cat([(torch.rand(B, K, 2, generator=g) * 0.9 - 0.45) * r, torch.rand(B, K, 1, generator=g) - 1.5], -1)
    dims = torch.stack([torch.rand(B, K, generator=g) * 3 + 2.5, torch.rand(B, K, generator=g) + 1.4, torch.rand(B, K, generator=g) + 1.2], -1)
    rot = (torch.rand(B, K, 1, generator=g) * 2 - 1) * 3.1
    valid = torch.rand(B, K, generator=g) < valid_share
    return pos, dims, rot, valid


BORDER_VALUES = (-32.0, 0.0, 3.0, 31.999998, 32.0, -32.000004, -33.5)  # on a 64 m axis; halved (exactly) on a 32 m axis


def _border_case(grid, rng, seed):
    """one box per border value and axis; the other coordinate is inside the grid.  Which cell, if any, each box marks follows from
    floor((v + range / 2) * n / range) with every factor exactly representable"""
    g = torch.Generator().manual_seed(seed)
    pos = []
    for axis in (0, 1):
        for i, v in enumerate(BORDER_VALUES):
            p = [0.0, 0.0, -1.0]
            p[axis] = float(np.float32(v)) * (rng[axis] / 64.0)
            p[1 - axis] = (5.25 - 1.5 * i) * (rng[1 - axis] / 64.0)
            pos.append(p)
    K = len(pos)
    pos = torch.tensor(pos, dtype=torch.float32)[None]
    dims = torch.stack([torch.rand(1, K, generator=g) * 3 + 2.5, torch.rand(1, K, generator=g) + 1.4, torch.rand(1, K, generator=g) + 1.2], -1)
    rot = (torch.rand(1, K, 1, generator=g) * 2 - 1) * 3.1
    return dict(pos=pos, dims=dims, rot=rot, valid=torch.ones(1, K, dtype=torch.bool), grid=grid, range=rng)


def border_expectation(case):
    """the centre cells of _border_case() worked out by hand: -r/2 -> cell 0, 0 -> n/2, 3 (scaled) -> n/2 + 3 n/64, the largest fp32
    below r/2 -> n - 1; r/2, the fp32 below -r/2 and -r/2 - 1.5 (scaled) -> outside"""
    H, W = case["grid"]
    want = torch.zeros(1, H, W, dtype=torch.bool)
    for axis, n in ((0, H), (1, W)):
        for i, cell in enumerate((0, n // 2, n // 2 + 3 * n // 64, n - 1, None, None, None)):
            if cell is None:
                continue
            other_n, other_r = (W, case["range"][1]) if axis == 0 else (H, case["range"][0])
            other = math.floor(((5.25 - 1.5 * i) * (other_r / 64.0) + other_r / 2) * other_n / other_r)
            want[(0, cell, other) if axis == 0 else (0, other, cell)] = True
    return want


def target_cases():
    """{id: dict(pos, dims, rot, valid, grid, range [, same_as])} of CPU fp32 tensors; `same_as` names the case whose outputs a padded
    variant must reproduce bit for bit"""
    out = {}

    def add(name, pos, dims, rot, valid, grid, rng, **kw):
        out[name] = dict(pos=pos.float(), dims=dims.float(), rot=rot.float(), valid=valid, grid=grid, range=rng, **kw)

    for name, B, K, grid, rng, seed in (("nonsquare-48x80", 2, 15, (48, 80), (60.0, 100.0), 215), ("odd-33x57", 3, 40, (33, 57), (50.0, 80.0), 340),
                                        ("small-5x7", 2, 7, (5, 7), (20.0, 28.0), 207), ("k300", 2, 300, (32, 32), (100.0, 100.0), 2300)):
        add(name, *_random_boxes(B, K, rng, seed), grid, rng)
    p, d, r, v = _random_boxes(2, 1, (60.0, 100.0), 11, valid_share=2.0)
    add("k1", p, d, r, v, (48, 80), (60.0, 100.0))
    add("k0", torch.zeros(2, 0, 3), torch.zeros(2, 0, 3), torch.zeros(2, 0, 1), torch.zeros(2, 0, dtype=torch.bool), (16, 24), (40.0, 60.0))
    p, d, r, v = _random_boxes(2, 6, (50.0, 80.0), 12)
    add("all-invalid", p, d, r, torch.zeros_like(v), (33, 57), (50.0, 80.0))
    # padded slots: the odd grid's boxes with invalid slots overwritten by zeros / NaN -- nothing may change
    base = out["odd-33x57"]
    for name, fill in (("pad-zero", 0.0), ("pad-nan", float("nan"))):
        inv = ~base["valid"]
        add(name, torch.where(inv[..., None], torch.full_like(base["pos"], fill), base["pos"]),
            torch.where(inv[..., None], torch.full_like(base["dims"], fill), base["dims"]),
            torch.where(inv[..., None], torch.full_like(base["rot"], fill), base["rot"]), base["valid"], base["grid"], base["range"],
            same_as="odd-33x57")
    out["border-64x64"] = _border_case((64, 64), (64.0, 64.0), 21)
    out["border-64x32"] = _border_case((64, 32), (32.0, 64.0), 22)
    # two identical valid boxes (slots 1 and 4) among others: the cells they win carry doubled attributes, unchanged probs
    p, d, r, v = _random_boxes(1, 6, (60.0, 100.0), 13, valid_share=2.0)
    p[0, 4], d[0, 4], r[0, 4] = p[0, 1], d[0, 1], r[0, 1]
    add("duplicate", p, d, r, v, (48, 80), (60.0, 100.0), duplicate=(1, 4))
    # normalisation, on 1.5 m cells (grid 40 x 60, range 60 x 90): 1 m beyond either edge (the in-grid maximum is off the centre), ten
    # ranges away (the maximum underflows: the 1e-5 clamp, every heat 0), 0.2 x 0.2 inside one cell, length 30
    pos = torch.tensor([[[31.0, 4.0, -1.0], [-7.0, -46.0, -1.2], [600.0, -900.0, -1.0], [3.3, -11.2, -0.8], [-12.0, 20.0, -1.1]]])
    dims = torch.tensor([[[4.0, 1.8, 1.5], [3.5, 1.6, 1.4], [4.0, 2.0, 1.5], [0.2, 0.2, 1.0], [30.0, 2.5, 3.0]]])
    rot = torch.tensor([[[0.4], [-1.1], [0.3], [0.7], [2.0]]])
    add("normalisation", pos, dims, rot, torch.ones(1, 5, dtype=torch.bool), (40, 60), (60.0, 90.0), far_box=2, beyond_edge=(0, 1))
    # rotations 0, float(pi / 2), +/- float(pi), 50
    rots = [0.0, float(np.float32(math.pi / 2)), float(np.float32(math.pi)), -float(np.float32(math.pi)), 50.0]
    p, d, _, _ = _random_boxes(1, 5, (60.0, 100.0), 14)
    add("rotations", p, d, torch.tensor(rots)[None, :, None], torch.ones(1, 5, dtype=torch.bool), (48, 80), (60.0, 100.0))
    # two boxes of one footprint 2.0001 m apart around a column of cell centres (1 m cells): along it their heats differ by 3e-4
    # relative -- well outside "uncertain", well inside a sloppy `h >= best * 0.999f` tie test; their z, height and nothing else differ
    pos = torch.tensor([[[3.5, -0.5, -1.0], [3.5, 1.5001, -0.4]]])
    dims = torch.tensor([[[12.0, 2.0, 1.5], [12.0, 2.0, 2.5]]])
    add("near-tie", pos, dims, torch.zeros(1, 2, 1), torch.ones(1, 2, dtype=torch.bool), (64, 64), (64.0, 64.0), near_tie_col=32)
    return out


def uncertain_count(ref):
    return int(ref["winner_uncertain"].sum()) + int((ref["threshold_uncertain"] & ~ref["winner_uncertain"]).sum())
