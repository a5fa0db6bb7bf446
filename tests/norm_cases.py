"""Cases, fp64 references and derived error bounds of the normalisation tests (tests/test_gpu_norm_fp64.py); nothing here needs a GPU.
tests/test_norm_cases.py proves on the CPU that the inputs are structured enough and the bounds tight enough: a reference that drops
the last block, miscounts its rows, divides by a wrong m, masks with `>=` or keeps the training coefficients in eval mode is off by
more than ten bounds.

References are elementary sums and products of torch fp64 tensors (any device) over the STORED, rounded inputs.  Bounds come from
the kernels' summation structure (liso_amd/csrc/bn.hip, chain_bodies.h, conv_mfma.hip) and the magnitudes of the case, never from a
kernel's output: u = 2^-24, first-order in u, one overall factor SAFETY = 2 for the dropped higher orders.

Geometry of bn.hip (geom(), stream_grid(), finalize_segment()): a 256-thread block has cg = C / V column groups (V = 4 fp32, 8 in the
16-bit types) and rl = 256 / cg row lanes; a block owns rows_per_block = max(ceil(M / 256), 128) rows, of which a thread adds
n_t = ceil(rows_per_block / rl) sequentially in fp32; one thread per channel then adds the rl LDS values in fp32; blocks are merged in
fp64."""
import numpy as np
import torch

U = 2.0 ** -24
SAFETY = 2.0
EPS, MOMENTUM = float(np.float32(1e-3)), float(np.float32(0.1))  # the ABI takes fp32: the references use the values it receives
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
VEC = {"fp32": 4, "bf16": 8, "fp16": 8}
FORMAT = {"fp32": (24, -126), "bf16": (8, -126), "fp16": (11, -14)}  # significant bits, smallest normal exponent
# the store of a 16-bit result, relative to the value and absolute (fp16 subnormals): half a spacing, before SAFETY
STORE = {"fp32": (0.0, 0.0), "bf16": (2.0 ** -9, 0.0), "fp16": (2.0 ** -12, 2.0 ** -25)}


class Geo:
    """the launch geometry of bn.hip for M rows of C channels"""

    def __init__(self, m, c, dt):
        v = VEC[dt]
        assert c % v == 0 and 0 < c <= 256 and m > 0
        self.m, self.c, self.dt = m, c, dt
        self.cg = c // v
        self.rl = 256 // self.cg
        self.rpb = max(-(-m // 256), 128)
        self.nblk = -(-m // self.rpb)
        assert self.nblk <= 4096
        self.last_n = m - (self.nblk - 1) * self.rpb
        self.n_t = -(-self.rpb // self.rl)
        self.k = self.n_t + self.rl  # fp32 additions behind one channel's block sum
        self.groups_of_rows = -(-m // self.rl)
        self.grid = min(self.groups_of_rows, 8192)
        self.second_trip = self.groups_of_rows > 8192
        self.idle_lanes = 256 - self.rl * self.cg
        self.cw = 32 if (c % 32 == 0 and c > 32 and self.nblk >= 64) else c


def spacing(v, dt):
    """distance between neighbouring values of the format at |v|"""
    p, emin = FORMAT[dt]
    _, e = torch.frexp(v.abs().double().clamp(min=2.0 ** emin))  # |v| = f * 2^e, f in [0.5, 1)
    return torch.exp2((e - 1 - (p - 1)).double())


def round_to(v, dt):
    return v.to(DTYPES[dt])


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
def zero_channels(c):
    """channels whose statistics get shift = 0 and whose planted rows hold x = 0: the ReLU input is exactly zero there"""
    return [ch for ch in range(c) if ch % 7 == 1]


def planted_rows(m):
    return sorted({0, m // 2, m - 1} | set(range(5, m, 13)))


def make_x(m, c, dt, seed, groups=1):
    """[groups, m, c] in the element type: per channel noise of std s_c + a ramp of amplitude 2 s_c along the rows + an offset of
    0 / 5 / 50 total stds (both signs); every group (InstanceNorm sample) gets another offset; exact zeros in zero_channels(c)"""
    g = torch.Generator().manual_seed(seed)
    ch = torch.arange(c)
    s = 0.25 * torch.exp2((ch % 4).double())
    ratio = torch.tensor([0.0, 5.0, 50.0], dtype=torch.float64)[ch % 3] * torch.where(ch % 2 == 0, 1.0, -1.0).double()
    ramp = torch.linspace(-1.0, 1.0, m, dtype=torch.float64)[:, None]
    x = torch.empty(groups, m, c, dtype=torch.float64)
    for k in range(groups):
        x[k] = s * (torch.randn(m, c, generator=g, dtype=torch.float64) + 2.0 * ramp + 1.5 * ratio + 0.8 * k)
    rows, z = torch.tensor(planted_rows(m)), torch.tensor(zero_channels(c))
    x[:, rows[:, None], z[None, :]] = 0.0
    return round_to(x, dt)


def make_params(c, seed):
    g = torch.Generator().manual_seed(seed + 1000)
    ch = torch.arange(c)
    gamma = (0.5 + torch.rand(c, generator=g)) * torch.where(ch % 5 == 0, -1.0, 1.0)
    beta = (0.1 + 0.3 * torch.randn(c, generator=g).abs()) * torch.where(ch % 4 == 3, -1.0, 1.0)  # (a single row's ReLU input is beta)
    rm = torch.randn(c, generator=g)
    rv = 0.5 + 1.5 * torch.rand(c, generator=g)
    return gamma.float(), beta.float(), rm.float(), rv.float()


def direct_stats(x):
    """fp64 mean and biased variance per channel of [m, c] (two passes)"""
    X = x.double()
    mean = X.sum(0) / X.shape[0]
    d = X - mean
    return mean, (d * d).sum(0) / X.shape[0]


def make_bwd_case(dt, c, m, relu, training, seed, groups=1):
    """x, dy in the element type; gamma and stats = scale | shift | mean | invstd in fp32, shift = 0 in zero_channels(c).
    dy = a_c + b_c * xhat + noise with |a_c| in [1, 1.5], |b_c| in [0.5, 1] and every sign pair"""
    x = make_x(m, c, dt, seed, groups)
    gamma, beta, _, _ = make_params(c, seed)
    g = torch.Generator().manual_seed(seed + 2000)
    ch = torch.arange(c)
    a = (1.0 + 0.5 * torch.rand(c, generator=g, dtype=torch.float64)) * torch.where(ch % 2 == 0, 1.0, -1.0)
    b = (0.5 + 0.5 * torch.rand(c, generator=g, dtype=torch.float64)) * torch.where((ch // 2) % 2 == 0, 1.0, -1.0)
    stats, dy = [], []
    for k in range(groups):
        mean, var = direct_stats(x[k])
        if not training:  # eval mode normalises with running statistics, not the batch's
            mean, var = mean + 0.1 * var.sqrt() + 0.01, var * 1.3 + 0.01
        inv = 1.0 / torch.sqrt(var + EPS)
        st = torch.stack([gamma.double() * inv, beta.double() - mean * gamma.double() * inv, mean, inv]).float()
        st[1, zero_channels(c)] = 0.0
        xh = (x[k].double() - st[2].double()) * st[3].double()
        dy.append(round_to(a + b * xh + 0.3 * torch.randn(m, c, generator=g, dtype=torch.float64), dt))
        stats.append(st.reshape(-1))
    return dict(x=x.contiguous(), dy=torch.stack(dy).contiguous(), gamma=gamma, stats=torch.stack(stats).contiguous())


# ---- backward: dx = A (dz - B - xhat C), grad_beta = sum dz, grad_gamma = sum dz xhat ---------------------------------------------
def bwd_reference(x, dy, gamma, stats, training, relu, geo, variant=None):
    """fp64 reference of liso_bn_relu_bwd on [m, c]; `variant` names one of the wrong kernels of the sensitivity checks"""
    X, G, c, m = x.double(), dy.double(), x.shape[1], x.shape[0]
    sc, sh, mu, inv = stats.double().view(4, c)
    if relu:
        z = X * sc + sh  # (fp32 operands: the product is exact in fp64 and the sum keeps the sign of the exact value, as one fmaf does)
        dz = torch.where((z >= 0) if variant == "mask_ge" else (z > 0), G, torch.zeros_like(G))
    else:
        dz = G
    xh = (X - mu) * inv
    t = dz * xh
    kept = (geo.nblk - 1) * geo.rpb if variant == "drop_last" else m
    a, b = dz[:kept].sum(0), t[:kept].sum(0)
    div = {"m_plus_1": m + 1, "m_padded": geo.nblk * geo.rpb}.get(variant, m)
    if training or variant == "eval_as_training":
        B, C = a / div, b / div
    else:
        B, C = torch.zeros_like(a), torch.zeros_like(b)
    A = gamma.double().to(X.device) * inv
    return dict(dx=A * (dz - B - xh * C), grad_gamma=b, grad_beta=a, A=A, B=B, C=C, dz=dz, xh=xh, abs_a=dz.abs().sum(0), abs_b=t.abs().sum(0))


def bwd_bounds(r, geo, training):
    """bounds of |kernel - reference| for the outputs of bwd_reference (per channel / per element), SAFETY included"""
    k, m = geo.k, geo.m
    # bn_bwd_reduce_body `a[n][j] += dz` (n_t - 1 adds), `sa += s_a[..]` (rl adds), bn_bwd_finalize_segment `(float)a` (1)
    da = (k + 1) * U * r["abs_a"]
    # the same adds as fmaf, + `xh = (vx - mu) * is` (2 roundings carried by every term) + the cast (1) + the fmaf's own rounding (1)
    db = (k + 4) * U * r["abs_b"]
    # coef B = (float)(a / m), C = (float)(b / m): the sums' errors over m (the casts are the `+ 1` above); 0 in eval mode
    dB, dC = (da / m, db / m) if training else (torch.zeros_like(da), torch.zeros_like(db))
    A, xh = r["A"].abs(), r["xh"].abs()
    # bn_bwd_dx_body `A * (dz - B - (vx - mu) * is * C)`: vx - mu, * is, * C, dz - B, - (..), A * (..): 6 roundings of terms no larger
    # than |dz| + |B| + |xhat C|; then the coefficient errors; `coef[ch] = gamma[ch] * stats[3c + ch]` rounds A once: u |dx|
    dx = A * (6 * U * (r["dz"].abs() + r["B"].abs() + (r["xh"] * r["C"]).abs()) + dB + xh * dC) + U * r["dx"].abs()
    rel, ab = STORE[geo.dt]
    dx = dx + rel * r["dx"].abs() + ab  # Vec<T>::store rounds to T
    return dict(dx=SAFETY * dx, grad_gamma=SAFETY * db, grad_beta=SAFETY * da)


def in_bwd_sum_reference(case, relu, geo):
    """liso_in_relu_bwd_sum: per-sample backward (training coefficients), parameter gradients rounded to fp32 per sample
    (in_bwd_finalize_sum_kernel `sum_a += (double)(float)a`, inside each sample's bound) and summed, the sum rounded once more"""
    dx, bdx, gg, gb, bgg, bgb = [], [], 0.0, 0.0, 0.0, 0.0
    for k in range(case["x"].shape[0]):
        r = bwd_reference(case["x"][k], case["dy"][k], case["gamma"], case["stats"][k], 1, relu, geo)
        b = bwd_bounds(r, geo, 1)
        dx.append(r["dx"]); bdx.append(b["dx"])
        gg, gb, bgg, bgb = gg + r["grad_gamma"], gb + r["grad_beta"], bgg + b["grad_gamma"], bgb + b["grad_beta"]
    ref = dict(dx=torch.stack(dx), grad_gamma=gg, grad_beta=gb)
    bnd = dict(dx=torch.stack(bdx), grad_gamma=bgg + SAFETY * U * gg.abs(), grad_beta=bgb + SAFETY * U * gb.abs())  # `(float)sum_a`
    return ref, bnd


# ---- forward statistics -------------------------------------------------------------------------------------------------------------------
def block_moments(x, geo):
    """per block b and channel, in fp64: n_b, K_b = first row, a = sum(x - K), |.| sum, b2 = sum (x - K)^2, mean_b, M2_b"""
    X, m, c = x.double(), geo.m, geo.c
    pad = geo.nblk * geo.rpb - m
    if pad:  # copies of the last block's first row add nothing to its shifted sums
        X = torch.cat([X, X[(geo.nblk - 1) * geo.rpb].expand(pad, c)])
    X = X.view(geo.nblk, geo.rpb, c)
    n = torch.full((geo.nblk, 1), float(geo.rpb), dtype=torch.float64, device=X.device)
    n[-1] = geo.last_n
    K = X[:, 0]
    d = X - K[:, None]
    a, abs1, b2 = d.sum(1), d.abs().sum(1), (d * d).sum(1)
    return dict(n=n, K=K, a=a, abs1=abs1, b2=b2, mean=K + a / n, m2=b2 - a * a / n)


def merge_blocks(bm, geo, variant=None):
    """bn_finalize_kernel in fp64: mean = sum n_b mean_b / m, M2 = sum (M2_b + n_b (mean_b - mean)^2)"""
    n, mean_b, m2_b = bm["n"].clone(), bm["mean"], bm["m2"]
    if variant == "last_count_rpb":
        n[-1] = geo.rpb
    if variant == "drop_last":
        n, mean_b, m2_b = n[:-1], mean_b[:-1], m2_b[:-1]
    mean = (n * mean_b).sum(0) / geo.m
    return mean, (m2_b + n * (mean_b - mean) ** 2).sum(0)


def finish_stats(mean, var, var_unbiased, gamma, beta, rm, rv, count):
    """scale | shift | mean | invstd and the running statistics' update (skipped for a single row, as bn_finalize_kernel does)"""
    g, b = gamma.double().to(mean.device), beta.double().to(mean.device)
    inv = 1.0 / torch.sqrt(var + EPS)
    out = dict(scale=g * inv, shift=b - mean * g * inv, mean=mean, invstd=inv, var=var)
    if rm is not None:
        r, v = rm.double().to(mean.device), rv.double().to(mean.device)
        out["running_mean"] = (1.0 - MOMENTUM) * r + MOMENTUM * mean if count > 1 else r
        out["running_var"] = (1.0 - MOMENTUM) * v + MOMENTUM * var_unbiased if count > 1 else v
    return out


def fwd_stats_reference(x, gamma, beta, rm, rv, geo, variant=None):
    """training-mode statistics of liso_bn_relu_fwd / one sample of liso_in_relu_fwd (rm = rv = None) on [m, c]"""
    m = geo.m
    if variant is None:
        mean, var = direct_stats(x)
        m2 = var * m
    else:
        mean, m2 = merge_blocks(block_moments(x, geo), geo, variant)
    return finish_stats(mean, m2 / m, m2 / max(m - 1, 1), gamma, beta, rm, rv, m)


def fwd_stats_bounds(x, ref, gamma, rm, rv, geo):
    """bounds for the outputs of fwd_stats_reference, SAFETY included"""
    bm, k, m = block_moments(x, geo), geo.k, geo.m
    n = bm["n"]
    # bn_stats_kernel `d = v - K` (1), `s1[j] += d` (n_t - 1), `a += s_1[..]` (rl)
    da = (k + 1) * U * bm["abs1"]
    # `p[tid] = kk + a / n`: the quotient and the sum round once each
    dmean_b = da / n + U * (bm["a"] / n).abs() + U * bm["mean"].abs()
    # `s2 = fmaf(d, d, s2)`: d carries its rounding twice (2) + the adds; `b2 - a * a / n`: a's error twice over, product and
    # quotient (2), the difference (1)
    dm2_b = (k + 2) * U * bm["b2"] + (2 * bm["a"].abs() * da + 2 * U * bm["a"] ** 2) / n + U * bm["m2"].abs()
    # bn_finalize_kernel: fp64 merge of the fp32 partials (its own roundings are 2^-29 u), `(float)mean`
    dmean64 = (n * dmean_b).sum(0) / m
    # `d = v - mean; acc += q2 + n_b * d * d`: both the block mean and the merged mean are perturbed
    mean, var = ref["mean"], ref["var"]
    dm2 = dm2_b.sum(0) + (2 * n * (bm["mean"] - mean).abs() * (dmean_b + dmean64)).sum(0)
    dinv64 = 0.5 * ref["invstd"] * (dm2 / m) / (var + EPS)  # d/dvar of (var + eps)^-1/2
    g = gamma.double().abs().to(mean.device)
    out = dict(mean=dmean64 + U * mean.abs(),                                      # `(float)mean`
               invstd=dinv64 + U * ref["invstd"],                                  # `(float)invstd`
               scale=g * dinv64 + U * ref["scale"].abs(),                          # `(float)(gamma * invstd)`
               shift=g * (ref["invstd"] * dmean64 + mean.abs() * dinv64) + U * ref["shift"].abs())  # `(float)(beta - mean * gamma * invstd)`
    if rm is not None and m > 1:
        # `(1.f - momentum) * running + momentum * (float)v`: 1.f - momentum and its product (2), momentum * v (1), the sum (1)
        keep_m, keep_v = (1.0 - MOMENTUM) * rm.double().abs().to(mean.device), (1.0 - MOMENTUM) * rv.double().abs().to(mean.device)
        var_u = var * m / (m - 1)
        out["running_mean"] = MOMENTUM * out["mean"] + 2 * U * keep_m + U * MOMENTUM * mean.abs() + U * ref["running_mean"].abs()
        out["running_var"] = MOMENTUM * (dm2 / (m - 1) + U * var_u) + 2 * U * keep_v + U * MOMENTUM * var_u + U * ref["running_var"].abs()
    elif rm is not None:
        out["running_mean"], out["running_var"] = torch.zeros_like(mean), torch.zeros_like(mean)  # left bit-identical
    return {k_: SAFETY * v for k_, v in out.items()}


def eval_stats_reference(gamma, beta, rm, rv):
    return finish_stats(rm.double(), rv.double(), None, gamma, beta, None, None, 0)


def eval_stats_bounds(ref, gamma, rm):
    """bn_eval_stats_kernel, all fp32: `1.f / sqrtf(running_var + eps)`: the sum (half of it under the root), the root, the quotient"""
    dinv = 2.5 * U * ref["invstd"]
    g = gamma.double().abs()
    return dict(mean=torch.zeros_like(dinv), invstd=SAFETY * dinv,
                scale=SAFETY * (g * dinv + U * ref["scale"].abs()),  # `gamma * invstd`
                # `beta - running_mean * gamma * invstd`: two products, the difference
                shift=SAFETY * (rm.double().abs() * g * dinv + 2 * U * (ref["mean"] * ref["scale"]).abs() + U * ref["shift"].abs()))


# ---- apply: y = round_T(relu?(fmaf(x, scale, shift))) from the fp32 statistics the call returned -------------------------------------------
def apply_reference(x, stats32, relu):
    c = x.shape[-1]
    sc, sh = stats32.double().view(4, c)[:2]
    z = x.double() * sc + sh
    return z.clamp(min=0.0) if relu else z


def apply_allowance(z, dt):
    """one fp32 spacing (bn_apply_kernel rounds the exact value once, the fp64 reference once more) + half a spacing of a 16-bit T"""
    return spacing(z, "fp32") + (0.5 * spacing(z, dt) if dt != "fp32" else 0.0)


# ---- convolution-side finalize: partial sums [rows][2][co_pad] -> statistics ---------------------------------------------------------------
CONV_ROWS = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 1345)
CONV_CO = (1, 3, 8, 64, 200)


def conv_partials(rows, co, seed, with_shift, samples=1, single=False):
    """per sample: `rows` blocks of known count, mean and variance per channel -> S1 = sum (y - shift), S2 = sum (y - shift)^2 in fp64,
    cast to fp32 [samples, rows, 2, co_pad]; co_pad - co columns of a pattern no channel may read.  single: one element in all (n = 1)"""
    g = torch.Generator().manual_seed(seed)
    co_pad = -(-co // 64) * 64
    ch = torch.arange(co)
    s = 0.25 * torch.exp2((ch % 4).double())
    centre = s * torch.tensor([0.0, 5.0, 50.0], dtype=torch.float64)[ch % 3] * torch.where(ch % 2 == 0, 1.0, -1.0)
    shift = (centre + 0.3 * s).float() if with_shift else None
    k0 = shift.double() if with_shift else torch.zeros(co, dtype=torch.float64)
    cnt = torch.randint(1, 200, (1, rows, 1), generator=g).double().expand(samples, rows, 1)  # (every sample has the same n)
    if single:
        cnt = torch.zeros(samples, rows, 1, dtype=torch.float64)
        cnt[:, rows // 2] = 1.0
    mu = centre + s * (torch.randn(samples, rows, co, generator=g, dtype=torch.float64) + torch.arange(samples).double()[:, None, None])
    var = (s * s) * (0.5 + torch.rand(samples, rows, co, generator=g, dtype=torch.float64)) * (cnt > 1)
    part = torch.full((samples, rows, 2, co_pad), 1.0e30, dtype=torch.float64)
    part[:, :, 0, :co] = cnt * (mu - k0)
    part[:, :, 1, :co] = cnt * (var + (mu - k0) ** 2)
    return part.float().contiguous(), shift, [int(v) for v in cnt.sum((1, 2))], co_pad


def conv_finalize_reference(part32, co, n, shift, gamma, beta, rm, rv, momentum=MOMENTUM):
    """mean = shift + S1 / n, var = max(S2 / n - (S1 / n)^2, 0) on the same fp32 partials, for one sample [rows, 2, co_pad]"""
    P = part32.double()
    s1, s2 = P[:, 0, :co].sum(0), P[:, 1, :co].sum(0)
    m1 = s1 / n
    var = (s2 / n - m1 * m1).clamp(min=0.0)
    mean = m1 + (shift.double().to(P.device) if shift is not None else 0.0)
    one, zero = torch.ones(co, dtype=torch.float64), torch.zeros(co, dtype=torch.float64)
    out = finish_stats(mean, var, None, gamma if gamma is not None else one, beta if beta is not None else zero, None, None, n)
    rows = P.shape[0]
    e = 2.0 ** -53
    # conv_bn_finalize_kernel: `acc += (double)v` and the two-level tree (rows additions in fp64); `q2 / n - m1 * m1` (3 roundings of
    # terms no larger than S2 / n + m1^2); `k + m1`
    dvar = e * ((rows + 3) * (P[:, 1, :co].abs().sum(0) / n + m1 * m1))
    dmean64 = e * (rows + 2) * (P[:, 0, :co].abs().sum(0) / n + mean.abs())
    dinv64 = 0.5 * out["invstd"] * dvar / (var + EPS) + e * out["invstd"]
    g = (gamma if gamma is not None else one).double().abs().to(P.device)
    bnd = dict(mean=dmean64 + U * mean.abs(), invstd=dinv64 + U * out["invstd"], scale=g * dinv64 + U * out["scale"].abs(),
               shift=g * (out["invstd"] * dmean64 + mean.abs() * dinv64) + U * out["shift"].abs())  # the four `(float)` casts
    if rm is not None:
        unb = var * n / (n - 1) if n > 1 else var  # (n = 1: the biased value, as the kernel keeps it)
        out["running_mean"] = (1.0 - momentum) * rm.double() + momentum * mean
        out["running_var"] = (1.0 - momentum) * rv.double() + momentum * unb
        # `(float)((1.0 - momentum) * running + momentum * v)`: fp64 arithmetic, one cast
        bnd["running_mean"] = momentum * dmean64 + U * out["running_mean"].abs()
        bnd["running_var"] = momentum * dvar * (n / max(n - 1, 1)) + U * out["running_var"].abs()
    return out, {k_: SAFETY * v for k_, v in bnd.items()}


# ---- residual tail: out = relu(fa(a) + fb(b)) ------------------------------------------------------------------------------------------------
def residual_reference(a, a_scale, a_shift, a_relu, b, b_scale, b_shift, b_relu):
    """[batch, pixels, c] fp32; scale / shift [batch, c] or None.  Each branch is one fmaf (one rounding of the exact value), then the
    sum rounds: the fp64 value of the same formula with the branches rounded to fp32 is within one fp32 spacing of the result"""
    def branch(v, sc, sh, relu):
        v = v.double()
        if sc is None:
            return v
        v = v * sc.double()[:, None, :] + sh.double()[:, None, :]
        v = v.float().double()  # (fp32 operands: the fp64 product is exact, the fp64 sum then the fp32 rounding differ from one fmaf
        return v.clamp(min=0.0) if relu else v  # only at a double-rounding tie: inside the spacing allowed)

    return (branch(a, a_scale, a_shift, a_relu) + branch(b, b_scale, b_shift, b_relu)).clamp(min=0.0)


# ---- case tables ---------------------------------------------------------------------------------------------------------------------------
# (dtype, C, M, relu, training); every M of the geometry table, paired with a C that takes the path named there
BWD_CASES = [
    ("fp32", 4, 1, 1, 1), ("fp32", 4, 3, 1, 0), ("fp32", 24, 37, 1, 1), ("fp32", 96, 128, 0, 1), ("fp32", 200, 129, 1, 1),
    ("fp32", 256, 261, 1, 1), ("fp32", 96, 261, 0, 0), ("fp32", 200, 261, 1, 0), ("fp32", 256, 8064, 1, 1), ("fp32", 96, 8065, 1, 1),
    ("fp32", 256, 8065, 0, 1), ("fp32", 256, 32769, 1, 1), ("fp32", 64, 70001, 1, 1),
    ("bf16", 8, 1, 1, 1), ("bf16", 8, 3, 0, 1), ("bf16", 96, 37, 1, 1), ("bf16", 200, 128, 1, 0), ("bf16", 256, 129, 1, 1),
    ("bf16", 96, 261, 0, 0), ("bf16", 200, 8064, 1, 1), ("bf16", 256, 8065, 1, 1), ("bf16", 96, 8065, 0, 1), ("bf16", 256, 65541, 1, 1),
    ("bf16", 64, 70001, 1, 1),
    ("fp16", 8, 37, 1, 1), ("fp16", 96, 129, 0, 1), ("fp16", 200, 261, 1, 0), ("fp16", 256, 261, 0, 0), ("fp16", 256, 8065, 1, 1),
    ("fp16", 256, 65541, 1, 1),
]
IN_BWD_SUM_CASES = [("fp32", 96, 261, 1), ("bf16", 200, 261, 1)]  # (dtype, C, M, relu), groups = 3
# (dtype, C, M, relu); training mode
FWD_CASES = [
    ("fp32", 4, 1, 1), ("fp32", 4, 3, 0), ("fp32", 24, 37, 1), ("fp32", 96, 128, 1), ("fp32", 200, 129, 0), ("fp32", 256, 261, 1),
    ("fp32", 256, 8064, 1), ("fp32", 96, 8065, 1), ("fp32", 256, 8065, 0), ("fp32", 256, 32769, 1), ("fp32", 64, 70001, 1),
    ("bf16", 8, 1, 1), ("bf16", 8, 3, 1), ("bf16", 96, 37, 0), ("bf16", 200, 129, 1), ("bf16", 256, 261, 1), ("bf16", 96, 8065, 1),
    ("bf16", 256, 8064, 0), ("bf16", 256, 65541, 1), ("bf16", 64, 70001, 1),
    ("fp16", 8, 37, 1), ("fp16", 200, 261, 0), ("fp16", 96, 129, 1), ("fp16", 256, 8065, 1), ("fp16", 256, 65541, 1),
]
EVAL_FWD_CASES = [("fp32", 96, 261, 1), ("fp32", 4, 3, 0), ("bf16", 200, 129, 1), ("fp16", 256, 37, 1)]
IN_FWD_CASES = [("fp32", 96, 261, 1), ("fp32", 24, 8065, 0), ("bf16", 200, 261, 1), ("bf16", 8, 129, 1)]  # groups = 3
GROUPS = 3

# Sensitivity (tests/test_norm_cases.py): every wrong kernel a case can tell must move one of its outputs by more than ten bounds.
# Rules that follow from a case's own flags:
#   single block  -> no "drop_last" / "last_count_rpb" (the issue's exemption: block variants on single-block cases)
#   relu = 0      -> no "mask_ge" (the issue's exemption: without a mask no planted zero takes part)
#   training = 0  -> B = C = 0 whatever m is, so "m_plus_1" is the reference itself; "eval_as_training" is required instead
#   training = 1  -> "eval_as_training" is the reference itself
# Everything else is a note on the case's own entry below: {case: (variant that cannot show, variant required in its place, why)}.
_M_PLUS_1 = ("m_plus_1", "m_padded",
             "1 / (m + 1) < 10 * SAFETY * (n_t + rl + 1) * u: B and C change by less than ten of the bound's own sum terms for ANY input; "
             "m rounded up to whole blocks (a relative 2e-3 .. 4e-3) is required instead")
_WHOLE_BLOCKS = ("last_count_rpb", None, "63 whole blocks: last_n == rows_per_block, the variant is the reference itself")
BWD_NOTES = {
    ("fp32", 256, 32769, 1, 1): _M_PLUS_1, ("fp32", 64, 70001, 1, 1): _M_PLUS_1,
    ("bf16", 256, 65541, 1, 1): _M_PLUS_1, ("bf16", 64, 70001, 1, 1): _M_PLUS_1,
    ("fp16", 256, 65541, 1, 1): _M_PLUS_1,
}
FWD_NOTES = {("fp32", 256, 8064, 1): _WHOLE_BLOCKS, ("bf16", 256, 8064, 0): _WHOLE_BLOCKS}


def _noted(variants, note):
    if note is None:
        return variants
    hidden, instead, _ = note
    assert hidden in variants
    return [v for v in variants if v != hidden] + ([instead] if instead else [])


def bwd_variants(dt, c, m, relu, training):
    geo = Geo(m, c, dt)
    v = (["drop_last"] if geo.nblk > 1 else []) + (["mask_ge"] if relu else []) + (["m_plus_1"] if training else ["eval_as_training"])
    return _noted(v, BWD_NOTES.get((dt, c, m, relu, training)))


def fwd_variants(dt, c, m, relu=None):
    v = ["drop_last", "last_count_rpb"] if Geo(m, c, dt).nblk > 1 else []
    return _noted(v, FWD_NOTES.get((dt, c, m, relu)))


def case_seed(*key):
    return sum((i + 1) * int(v) for i, v in enumerate(key[1:])) + 7919 * list(DTYPES).index(key[0])


def worst_ratio(ref, other, bounds):
    """max over outputs and elements of |other - ref| / bound; inf where an output with a zero bound differs and wherever `other`
    is not finite (a NaN compares false with everything: it must never pass as a small ratio)"""
    worst = 0.0
    for name, bnd in bounds.items():
        d = (other[name].double().to(bnd.device) - ref[name]).abs()
        inf = torch.full_like(d, float("inf"))
        r = torch.where(bnd > 0, d / bnd.clamp(min=1e-300), torch.where(d > 0, inf, torch.zeros_like(d)))
        r = torch.where(torch.isfinite(d), r, inf)
        worst = max(worst, float(r.max()))
    return worst


def within(got, ref, allowance):
    """every element of `got` is finite and within `allowance` of `ref` -> (ok, number of elements outside)"""
    ok = (got.double() - ref).abs() <= allowance  # (false for a NaN or an infinity in got)
    return bool(ok.all()), int((~ok).sum())
