"""The cases, references and bounds of tests/norm_cases.py mean something, shown without a GPU: the case tables cover every (path,
dtype) pair and every geometry of the GPU test (tests/test_gpu_norm_fp64.py); the inputs have the structure the references need to
tell kernels apart; and every wrong kernel of the sensitivity list moves an output of every case it can affect by more than ten of
that case's bounds."""
import pytest
import torch

from tests import norm_cases as NC

TEN = 10.0


def _id(case):
    return "-".join(str(v) for v in case)


# ---- the tables ---------------------------------------------------------------------------------------------------------------------------
def test_case_tables_cover_every_path_dtype_and_geometry():
    dts = set(NC.DTYPES)
    assert {c[0] for c in NC.FWD_CASES} == dts and {c[0] for c in NC.EVAL_FWD_CASES} == dts
    assert {c[0] for c in NC.IN_FWD_CASES} == {"fp32", "bf16"} == {c[0] for c in NC.IN_BWD_SUM_CASES}  # (InstanceNorm: fp32 / bf16 only)
    for dt in dts:
        assert {(r, t) for d, _, _, r, t in NC.BWD_CASES if d == dt} == {(0, 0), (0, 1), (1, 0), (1, 1)}, dt
        assert {c[3] for c in NC.FWD_CASES if c[0] == dt} == {0, 1}
    for table in (NC.BWD_CASES, NC.FWD_CASES):
        assert {c[1] for c in table if c[0] == "fp32"} >= {4, 24, 96, 200, 256}
        for dt in ("bf16", "fp16"):
            assert {c[1] for c in table if c[0] == dt} >= {8, 96, 200, 256}
        assert {c[2] for c in table} == {1, 3, 37, 128, 129, 261, 8064, 8065, 32769, 65541, 70001}
        assert len({_id(c) for c in table}) == len(table)
    # eval-mode backward with ReLU in fp32 and bf16 (and fp16)
    assert {d for d, _, _, r, t in NC.BWD_CASES if r == 1 and t == 0} == dts


def test_geometries_take_the_paths_they_are_named_for():
    G = NC.Geo
    for dt, c in (("fp32", 4), ("bf16", 8), ("fp16", 8)):
        g = G(3, c, dt)
        assert (g.cg, g.rl, g.nblk) == (1, 256, 1) and g.m < g.rl  # one lane per row, fewer rows than row lanes
        assert G(1, c, dt).last_n == 1
    assert G(37, 24, "fp32").idle_lanes == 4 and G(37, 96, "bf16").idle_lanes == 4 and G(261, 200, "fp16").idle_lanes == 6
    assert G(261, 96, "fp32").idle_lanes == 16 and G(129, 200, "fp32").idle_lanes == 6
    assert (G(37, 24, "fp32").nblk, G(37, 24, "fp32").last_n) == (1, 37)
    assert (G(128, 96, "fp32").nblk, G(128, 96, "fp32").last_n) == (1, 128)
    assert (G(129, 200, "fp32").nblk, G(129, 200, "fp32").last_n) == (2, 1)
    assert (G(261, 256, "fp32").nblk, G(261, 256, "fp32").last_n) == (3, 5)
    for dt in NC.DTYPES:
        g = G(8064, 256, dt)
        assert (g.nblk, g.last_n, g.cw) == (63, 128, 256)  # whole-C finalize
        for c in (96, 256):
            g = G(8065, c, dt)
            assert (g.nblk, g.last_n, g.cw) == (64, 1, 32)  # 32-channel segment finalize
        assert G(8065, 200, dt).cw == 200 and G(8065, 24 if dt == "fp32" else 8, dt).cw != 32
    g = G(32769, 256, "fp32")
    assert (g.rpb, g.nblk, g.last_n, g.groups_of_rows, g.second_trip) == (129, 255, 3, 8193, True)
    for dt in ("bf16", "fp16"):
        g = G(65541, 256, dt)
        assert (g.rpb, g.nblk, g.last_n, g.second_trip) == (257, 256, 6, True) and g.groups_of_rows == 8193
    for dt in ("fp32", "bf16"):
        g = G(70001, 64, dt)
        assert (g.rpb, g.nblk, g.last_n) == (274, 256, 131)
    assert max(G(m, c, dt).rpb for dt, c, m, *_ in NC.BWD_CASES) > 128 and max(G(m, c, dt).rpb for dt, c, m, _ in NC.FWD_CASES) > 128
    # the largest tensor is about 33 MB
    assert max(m * c * (4 if dt == "fp32" else 2) for dt, c, m, *_ in NC.BWD_CASES + NC.FWD_CASES) <= 34 * 2 ** 20


# ---- the inputs ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", list(NC.DTYPES))
def test_inputs_have_offsets_block_structure_and_exact_zeros(dt):
    m, c = 8065, 96
    geo = NC.Geo(m, c, dt)
    case = NC.make_bwd_case(dt, c, m, 1, 1, 5)
    x, dy, st = case["x"][0], case["dy"][0], case["stats"][0].double().view(4, c)
    assert x.dtype == NC.DTYPES[dt] == dy.dtype and case["stats"].dtype == torch.float32
    mean, var = NC.direct_stats(x)
    ratio = (mean.abs() / var.sqrt())
    keep = torch.tensor([ch not in NC.zero_channels(c) for ch in range(c)])
    for k, (lo, hi) in enumerate(((0.0, 0.2), (4.0, 6.0), (40.0, 60.0))):  # |mean| / std of 0, 5 and 50
        sel = keep & (torch.arange(c) % 3 == k)
        assert sel.any() and bool(((ratio[sel] >= lo) & (ratio[sel] <= hi)).all()), (k, ratio[sel])
    assert (mean > 0).any() and (mean < 0).any()
    bm = NC.block_moments(x, geo)
    spread = (bm["mean"].max(0).values - bm["mean"].min(0).values) / var.sqrt()
    assert float(spread.min()) > 1.0  # block means differ by more than a standard deviation
    # the last block (ONE row here: ramp end + its own noise) lies about a standard deviation from the global mean
    assert float(((bm["mean"][-1] - mean).abs() / var.sqrt()).median()) > 0.7
    # sum(dz) / m and sum(dz xhat) / m are O(1) parts of dx, of both signs
    r = NC.bwd_reference(x, dy, case["gamma"], case["stats"][0], 1, 1, geo)
    # (a zero channel with a negative offset is off everywhere: B = C = 0 there)
    assert float((r["B"].abs() > 0.1).double().mean()) > 0.9 and (r["B"] > 0).any() and (r["B"] < 0).any()
    assert float(r["C"].abs().median()) > 0.1 and (r["C"] > 0).any() and (r["C"] < 0).any()
    assert (case["gamma"] < 0).any() and (case["gamma"] > 0).any()
    # exact zeros of the ReLU input: decided the same way by one fp32 fmaf and by fp64
    z = x.double() * st[0] + st[1]
    rows, zc = NC.planted_rows(m), NC.zero_channels(c)
    assert len(zc) >= 1 and {0, m - 1} <= set(rows)
    assert bool((z[rows][:, zc] == 0).all()) and bool((st[1][zc] == 0).all())
    z32 = torch.addcmul(st[1].float(), x.float(), st[0].float())  # (not fused on every host: the sign can only be compared where |z| is not tiny)
    big = z.abs() > 1e-4
    assert bool(((z32.double() > 0) == (z > 0))[big].all())
    assert 0.02 < float((z > 0).double().mean()) < 0.98


def test_zero_channels_and_rows_exist_at_every_size():
    for c in (4, 8, 24, 96, 200, 256):
        assert NC.zero_channels(c) and max(NC.zero_channels(c)) < c
    for m in (1, 3, 37, 70001):
        assert {0, m - 1} <= set(NC.planted_rows(m)) and max(NC.planted_rows(m)) < m


# ---- the references -----------------------------------------------------------------------------------------------------------------------
def test_backward_reference_is_the_derivative_of_the_forward_formula():
    """autograd of the elementary fp64 forward (not of a library BatchNorm) gives the reference's dx, grad_gamma and grad_beta"""
    m, c, dt = 37, 24, "fp32"
    geo = NC.Geo(m, c, dt)
    for training in (1, 0):
        case = NC.make_bwd_case(dt, c, m, 1, training, 9)
        st = case["stats"][0].double().view(4, c)
        x = case["x"][0].double().requires_grad_(True)
        gamma = case["gamma"].double().requires_grad_(True)
        beta = torch.zeros(c, dtype=torch.float64, requires_grad=True)
        if training:  # statistics that ARE functions of x; the mask and xhat use the same numbers as the reference
            mean = x.sum(0) / m
            inv = 1.0 / torch.sqrt(((x - mean) ** 2).sum(0) / m + NC.EPS)
            stats = torch.stack([case["gamma"].double() * inv, st[1], mean, inv]).detach()
        else:
            mean, inv, stats = st[2], st[3], st
        y = gamma * (x - mean) * inv + beta
        on = (case["x"][0].double() * stats[0] + stats[1]) > 0
        (y * on * case["dy"][0].double()).sum().backward()
        r = NC.bwd_reference(case["x"][0], case["dy"][0], case["gamma"], stats.reshape(-1), training, 1, geo)
        assert float((r["dx"] - x.grad).abs().max()) < 1e-12 * float(x.grad.abs().max())
        assert float((r["grad_gamma"] - gamma.grad).abs().max()) < 1e-12 * float(gamma.grad.abs().max())
        assert float((r["grad_beta"] - beta.grad).abs().max()) < 1e-12 * float(beta.grad.abs().max())


@pytest.mark.parametrize("case", [c for c in NC.FWD_CASES if c[2] <= 8065], ids=_id)
def test_block_merge_restates_the_direct_statistics(case):
    dt, c, m, _ = case
    geo = NC.Geo(m, c, dt)
    x = NC.make_x(m, c, dt, NC.case_seed(*case))[0]
    mean, var = NC.direct_stats(x)
    bmean, m2 = NC.merge_blocks(NC.block_moments(x, geo), geo)
    scale = float(x.double().abs().max())
    assert float((bmean - mean).abs().max()) <= 1e-12 * scale and float((m2 / m - var).abs().max()) <= 1e-10 * scale * scale
    if m == 1:
        assert float(var.abs().max()) == 0.0


def test_spacing_and_apply_allowance():
    v = torch.tensor([1.0, 1.5, 2.0, 0.75, 3e-6, 0.0], dtype=torch.float64)
    assert NC.spacing(v, "fp32").tolist()[:4] == [2.0 ** -23, 2.0 ** -23, 2.0 ** -22, 2.0 ** -24]
    assert NC.spacing(v, "bf16").tolist()[:3] == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6]
    assert NC.spacing(v, "fp16").tolist() == [2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 2.0 ** -11, 2.0 ** -24, 2.0 ** -24]
    for dt in ("bf16", "fp16"):  # rounding to T is within the allowance, a truncating store is not
        z = torch.linspace(0.1, 9.0, 4001, dtype=torch.float64)
        assert bool(((NC.round_to(z.float(), dt).double() - z).abs() <= NC.apply_allowance(z, dt)).all())
        trunc = torch.floor(z / NC.spacing(z, dt)) * NC.spacing(z, dt)
        assert bool(((trunc - z).abs() > NC.apply_allowance(z, dt)).any())


# ---- sensitivity: a wrong kernel is more than ten bounds away ----------------------------------------------------------------------------
@pytest.mark.parametrize("case", NC.BWD_CASES, ids=_id)
def test_wrong_backward_kernels_are_ten_bounds_away(case):
    dt, c, m, relu, training = case
    geo = NC.Geo(m, c, dt)
    d = NC.make_bwd_case(dt, c, m, relu, training, NC.case_seed(*case))
    args = (d["x"][0], d["dy"][0], d["gamma"], d["stats"][0], training, relu, geo)
    ref = NC.bwd_reference(*args)
    bnd = NC.bwd_bounds(ref, geo, training)
    assert all(bool(torch.isfinite(b).all()) and bool((b >= 0).all()) for b in bnd.values())
    variants = NC.bwd_variants(*case)
    assert variants  # every case can tell at least one wrong kernel
    assert ("drop_last" in variants) == (geo.nblk > 1) and ("mask_ge" in variants) == bool(relu)
    for v in variants:
        ratio = NC.worst_ratio(ref, NC.bwd_reference(*args, variant=v), bnd)
        assert ratio > TEN, (v, ratio)
    # a note on the case's entry replaces "m_plus_1" by "m_padded" exactly where the arithmetic rules it out for ANY input:
    # |dx(m + 1) - dx| = |A| |B + xhat C| / (m + 1) <= |A| (mean|dz| + |xhat| mean|dz xhat|) / (m + 1), and the bound holds
    # SAFETY |A| (n_t + rl + 1) u (mean|dz| + |xhat| mean|dz xhat|) from the sums' errors alone
    if training:
        assert (case in NC.BWD_NOTES) == (1.0 / (m + 1) < TEN * NC.SAFETY * (geo.k + 1) * NC.U)
        assert ("m_padded" in variants) == (case in NC.BWD_NOTES) == ("m_plus_1" not in variants)
    else:
        assert case not in NC.BWD_NOTES and "eval_as_training" in variants


@pytest.mark.parametrize("case", NC.IN_BWD_SUM_CASES, ids=_id)
def test_wrong_instance_norm_backward_is_ten_bounds_away(case):
    dt, c, m, relu = case
    geo = NC.Geo(m, c, dt)
    d = NC.make_bwd_case(dt, c, m, relu, 1, NC.case_seed(*case), groups=NC.GROUPS)
    ref, bnd = NC.in_bwd_sum_reference(d, relu, geo)
    means = torch.stack([NC.direct_stats(d["x"][k])[0] for k in range(NC.GROUPS)])
    assert float((means[1:] - means[:-1]).abs().min()) > 0.1  # every sample has its own offset in every channel
    # a sample's statistics or partial sums taken from its neighbour
    swapped = dict(d, stats=d["stats"].roll(1, 0).contiguous())
    other, _ = NC.in_bwd_sum_reference(swapped, relu, geo)
    assert NC.worst_ratio(ref, other, bnd) > TEN
    for v in ("drop_last", "mask_ge", "m_plus_1"):
        dx, gg, gb = [], 0.0, 0.0
        for k in range(NC.GROUPS):
            r = NC.bwd_reference(d["x"][k], d["dy"][k], d["gamma"], d["stats"][k], 1, relu, geo, variant=v)
            dx.append(r["dx"]); gg = gg + r["grad_gamma"]; gb = gb + r["grad_beta"]
        assert NC.worst_ratio(ref, dict(dx=torch.stack(dx), grad_gamma=gg, grad_beta=gb), bnd) > TEN, v


def _fwd_sensitivity(x, gamma, beta, rm, rv, geo, variants):
    ref = NC.fwd_stats_reference(x, gamma, beta, rm, rv, geo)
    bnd = NC.fwd_stats_bounds(x, ref, gamma, rm, rv, geo)
    assert all(bool(torch.isfinite(b).all()) and bool((b >= 0).all()) for b in bnd.values())
    # the variance's bound is relative to the variance (through invstd), not to mean^2
    assert float((bnd["invstd"] / ref["invstd"]).max()) < 2e-3
    for v in variants:
        ratio = NC.worst_ratio(ref, NC.fwd_stats_reference(x, gamma, beta, rm, rv, geo, variant=v), bnd)
        assert ratio > TEN, (v, ratio)
    return ref, bnd


@pytest.mark.parametrize("case", NC.FWD_CASES, ids=_id)
def test_wrong_forward_merges_are_ten_bounds_away(case):
    dt, c, m, _ = case
    geo = NC.Geo(m, c, dt)
    seed = NC.case_seed(*case)
    gamma, beta, rm, rv = NC.make_params(c, seed)
    variants = NC.fwd_variants(*case)
    assert bool(variants) == (geo.nblk > 1)
    # the one note of this table: "last_count_rpb" cannot show exactly where the last block is whole
    assert (case in NC.FWD_NOTES) == (geo.nblk > 1 and geo.last_n == geo.rpb) == (geo.nblk > 1 and "last_count_rpb" not in variants)
    ref, bnd = _fwd_sensitivity(NC.make_x(m, c, dt, seed)[0], gamma, beta, rm, rv, geo, variants)
    if m == 1:
        assert torch.equal(ref["running_mean"], rm.double()) and torch.equal(ref["running_var"], rv.double())
        assert float(bnd["running_mean"].max()) == 0.0 == float(bnd["running_var"].max())


@pytest.mark.parametrize("case", NC.IN_FWD_CASES, ids=_id)
def test_wrong_instance_norm_forward_is_ten_bounds_away(case):
    dt, c, m, _ = case
    geo = NC.Geo(m, c, dt)
    seed = NC.case_seed(*case)
    gamma, beta, _, _ = NC.make_params(c, seed)
    x = NC.make_x(m, c, dt, seed, groups=NC.GROUPS)
    refs = []
    for k in range(NC.GROUPS):
        ref, bnd = _fwd_sensitivity(x[k], gamma, beta, None, None, geo, NC.fwd_variants(dt, c, m))
        refs.append((ref, bnd))
    for k in range(NC.GROUPS):  # a sample read at its neighbour's partials or statistics address
        assert NC.worst_ratio(refs[k][0], refs[(k + 1) % NC.GROUPS][0], refs[k][1]) > TEN


def test_eval_statistics_bounds_and_conv_finalize_reference():
    gamma, beta, rm, rv = NC.make_params(256, 3)
    ref = NC.eval_stats_reference(gamma, beta, rm, rv)
    bnd = NC.eval_stats_bounds(ref, gamma, rm)
    assert torch.equal(ref["mean"], rm.double()) and float((bnd["scale"] / ref["scale"].abs()).max()) < 1e-6
    for rows in NC.CONV_ROWS:
        for co in NC.CONV_CO:
            for with_shift in (False, True):
                part, shift, n, co_pad = NC.conv_partials(rows, co, rows + co, with_shift)
                assert part.shape == (1, rows, 2, co_pad) and co_pad % 64 == 0 and 0 <= co_pad - co < 64 and n[0] >= rows
                out, b = NC.conv_finalize_reference(part[0], co, n[0], shift, gamma[:co], beta[:co], rm[:co], rv[:co])
                assert all(bool(torch.isfinite(v).all()) for v in list(out.values()) + list(b.values()))
                assert float((b["mean"] / out["mean"].abs().clamp(min=1e-3)).max()) < 1e-5
                # a finalize that loses the last row of the walk, or reads the pad columns, is far outside
                less, _ = NC.conv_finalize_reference(part[0][:-1], co, n[0], shift, gamma[:co], beta[:co], rm[:co], rv[:co]) if rows > 1 else (None, None)
                if less is not None:
                    assert NC.worst_ratio(out, less, b) > TEN
    part, shift, n, _ = NC.conv_partials(65, 8, 1, True, single=True)
    assert n == [1]
    out, b = NC.conv_finalize_reference(part[0], 8, 1, shift, gamma[:8], beta[:8], rm[:8], rv[:8])
    assert float(out["var"].abs().max()) < 1e-6 and bool(torch.isfinite(out["running_var"]).all())


def test_a_non_finite_output_never_passes():
    """NaN and infinities in any output, under a positive or a zero bound, score inf; `within` refuses them too"""
    dt, c, m = "bf16", 8, 3
    geo = NC.Geo(m, c, dt)
    d = NC.make_bwd_case(dt, c, m, 1, 1, 4)
    ref = NC.bwd_reference(d["x"][0], d["dy"][0], d["gamma"], d["stats"][0], 1, 1, geo)
    bnd = NC.bwd_bounds(ref, geo, 1)
    good = {k: ref[k].clone() for k in bnd}
    assert NC.worst_ratio(ref, good, bnd) == 0.0
    for name in bnd:
        for bad in (float("nan"), float("inf"), -float("inf")):
            got = {k: v.clone() for k, v in good.items()}
            got[name].view(-1)[got[name].numel() // 2] = bad
            assert NC.worst_ratio(ref, got, bnd) > 1.0, (name, bad)
            assert NC.worst_ratio(ref, got, {name: bnd[name]}) == float("inf")
            got[name].fill_(bad)
            assert NC.worst_ratio(ref, got, bnd) == float("inf")
    zero = {"dx": torch.zeros_like(bnd["dx"])}  # a zero bound: equal passes, NaN does not
    assert NC.worst_ratio(ref, good, zero) == 0.0
    got = {"dx": good["dx"].clone()}
    got["dx"][1, 2] = float("nan")
    assert NC.worst_ratio(ref, got, zero) == float("inf")
    z = torch.linspace(-2.0, 2.0, 64, dtype=torch.float64)
    y = NC.round_to(z.float(), dt)
    assert NC.within(y, z, NC.apply_allowance(z, dt)) == (True, 0)
    for bad in (float("nan"), float("inf")):
        y2 = y.clone()
        y2[7] = bad
        assert NC.within(y2, z, NC.apply_allowance(z, dt)) == (False, 1)


def test_residual_reference():
    a, b = torch.tensor([[[1.0, -2.0, 0.5, -0.25]]]), torch.tensor([[[0.5, 1.0, -3.0, 0.25]]])
    sc, sh = torch.tensor([[2.0, 2.0, 2.0, 2.0]]), torch.tensor([[0.0, 1.0, 0.0, 0.0]])
    assert NC.residual_reference(a, None, None, 0, b, None, None, 0).tolist() == [[[1.5, 0.0, 0.0, 0.0]]]
    assert NC.residual_reference(a, sc, sh, 0, b, None, None, 0).tolist() == [[[2.5, 0.0, 0.0, 0.0]]]
    assert NC.residual_reference(a, sc, sh, 1, b, None, None, 0).tolist() == [[[2.5, 1.0, 0.0, 0.25]]]
    assert NC.residual_reference(a, sc, sh, 1, b, sc, sh, 1).tolist() == [[[3.0, 3.0, 1.0, 0.5]]]
