"""The grouped / two-gradient BatchNorm backward (liso_bn_relu_bwd_multi, three launches) against the launches it replaces, event-timed
over 50 calls after warm-up, at the detector step's sites (B = 2, bf16):
  block 0 output   64 ch @ 256 x 256, two gradients: 2 x liso_bn_relu_bwd + add of the dx maps + adds of dgamma / dbeta
  block 1 output  128 ch @ 128 x 128, two gradients: the same
  concatenation   3 x 128 ch @ 256 x 256, one gradient: 3 x liso_bn_relu_bwd_strided
  single map      64 ch @ 256 x 256, one gradient: the single call (one group, one gradient) next to the grouped call on the same map
python scripts/bn_joint_time.py [B]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from liso_amd import _lib as L  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 2
lib, dev, dt = L.lib(), torch.device("cuda"), torch.bfloat16
code = L.elem_code(dt)


def stats_of(x):
    C = x.shape[1]
    xf = x.float()
    mean, invstd = xf.mean(0), (xf.var(0, unbiased=False) + 1e-3).rsqrt()
    gamma = torch.rand(C, device=dev) + 0.5
    return gamma, torch.cat([gamma * invstd, -mean * gamma * invstd, mean, invstd]).contiguous()


def timed(fn, n=50):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def site(name, cs, hw, n_grads):
    torch.manual_seed(0)
    m, ct = B * hw * hw, sum(cs)
    x = (torch.randn(m, ct, device=dev) * 0.5 + 0.1).to(dt)
    gs = [torch.randn(m, ct, device=dev).to(dt) for _ in range(n_grads)]
    par = [stats_of(x[:, o:o + c]) for o, c in zip([sum(cs[:k]) for k in range(len(cs))], cs)]
    dxs = [torch.empty_like(x) for _ in range(n_grads)]
    gg = [[torch.empty(c, device=dev) for c in cs] for _ in range(2 * n_grads)]
    ws1 = torch.empty(max(lib.liso_bn_workspace_bytes(c) for c in cs), dtype=torch.uint8, device=dev)

    def separate():
        for n, g in enumerate(gs):
            off = 0
            for k, (c, (gamma, st)) in enumerate(zip(cs, par)):
                L.check(lib.liso_bn_relu_bwd_strided(L.ptr(g[:, off:off + c]), ct, L.ptr(x[:, off:off + c]), ct, code, m, c, L.ptr(gamma), L.ptr(st),
                                                     1, 1, L.ptr(dxs[n][:, off:off + c]), ct, L.ptr(gg[2 * n][k]), L.ptr(gg[2 * n + 1][k]),
                                                     L.ptr(ws1), ws1.numel(), L.stream_ptr()), "bn_relu_bwd_strided")
                off += c
        if n_grads == 2:  # (what autograd adds today)
            torch.add(dxs[0], dxs[1])
            for k in range(len(cs)):
                gg[0][k].add_(gg[2][k])
                gg[1][k].add_(gg[3][k])

    tab = (L.BnGroup * len(cs))()
    off = 0
    for k, (c, (gamma, st)) in enumerate(zip(cs, par)):
        tab[k].c_off, tab[k].c = off, c
        tab[k].gamma, tab[k].stats, tab[k].grad_gamma, tab[k].grad_beta = gamma.data_ptr(), st.data_ptr(), gg[0][k].data_ptr(), gg[1][k].data_ptr()
        off += c
    nbytes = lib.liso_bn_multi_workspace_bytes(tab, len(cs), n_grads)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    dx = torch.empty_like(x)

    def joint():
        L.check(lib.liso_bn_relu_bwd_multi(L.ptr(gs[0]), ct, L.ptr(gs[1]) if n_grads == 2 else None, ct, L.ptr(x), ct, code, m, tab, len(cs), 1, 1,
                                           L.ptr(dx), ct, L.ptr(ws), nbytes, None, None, L.stream_ptr()), "bn_relu_bwd_multi")

    a, b = timed(separate), timed(joint)
    n_sep = 3 * len(cs) * n_grads + (1 + 2 * len(cs) if n_grads == 2 else 0)
    print(f"{name:16s} B{B} {'+'.join(str(c) for c in cs):>11s} ch @{hw}: separate {a:7.1f} us ({n_sep} launches)   joint {b:7.1f} us (3 launches)")


site("block 0 output", [64], 256, 2)
site("block 1 output", [128], 128, 2)
site("concatenation", [128, 128, 128], 256, 1)
site("single map", [64], 256, 1)
