"""liso_adamw_step_packed_f32 and liso_conv_pack_weights_placed (include/liso_optim.h, include/liso_conv.h) on the synthetic parameter
list of tests/adamw_pack_cases.py: parameters, both moments, every byte of every panel and every mirror must equal BITWISE what
liso_adamw_step_scaled_f32 followed by liso_conv_pack_weights gives on clones (merged filters: torch.cat / slice assignment, then
liso_conv_pack_weights).  Every buffer sits between guard bands."""
import pytest
import torch

from tests.adamw_pack_cases import CAT, DIAG, DIAG_CO, build_items, layout, table_image

pytestmark = pytest.mark.gpu

GUARD, CANARY, PATTERN = 4096, 0xC7, 0xA5


class _Guarded:
    """device buffers between canary bands"""

    def __init__(self, dev):
        self.dev, self.bases = dev, []

    def raw(self, nbytes, fill):
        pad = (-nbytes) % 256
        base = torch.full((GUARD + nbytes + pad + GUARD,), CANARY, dtype=torch.uint8, device=self.dev)
        base[GUARD:GUARD + nbytes] = fill
        self.bases.append((base, nbytes))
        return base[GUARD:GUARD + nbytes]

    def f32(self, shape, fill=0):
        numel = 1
        for s in shape:
            numel *= s
        return self.raw(4 * numel, fill).view(torch.float32).view(shape)

    def check(self):
        torch.cuda.synchronize()
        for base, nbytes in self.bases:
            assert bool((base[:GUARD] == CANARY).all()) and bool((base[GUARD + nbytes:] == CANARY).all()), f"guard of a {nbytes}-byte buffer overwritten"


def _pack(L, w, transposed, for_dgrad, mode):
    """liso_conv_pack_weights of a contiguous [d0, d1, kh, kw] tensor -> panel bytes"""
    d0, d1, kh, kw = w.shape
    K, N = (d1, d0) if bool(transposed) == bool(for_dgrad) else (d0, d1)
    out = torch.full((L.lib().liso_conv_packed_bytes(K, N, kh * kw, mode),), 0x5A, dtype=torch.uint8, device=w.device)
    L.check(L.lib().liso_conv_pack_weights(L.ptr(w), d0, d1, kh, kw, int(transposed), int(for_dgrad), mode, L.ptr(out), L.stream_ptr()), "pack")
    return out


def _reference(L, flat_p, mode):
    """-> ({(name, for_dgrad): panel bytes}, {name: merged fp32 tensor}) from the parameters in `flat_p`"""
    tensors, offs, _ = layout()
    shapes = {n: (s, t) for n, s, t in tensors}

    def tens(n):
        s, _ = shapes[n]
        numel = 1
        for d in s:
            numel *= d
        return flat_p[offs[n]:offs[n] + numel].view(s)

    merged = {"cat": torch.cat([tens(n) for n, _ in CAT], dim=0).contiguous(), "cat_b": torch.cat([tens(n + "_b") for n, _ in CAT]),
              "diag_b": torch.cat([tens(n + "_b") for n, _ in DIAG])}
    W = torch.zeros((8, 32, 3, 3), device=flat_p.device)
    o = 0
    for i, ((n, _), co) in enumerate(zip(DIAG, DIAG_CO)):
        W[o:o + co, 8 * i:8 * i + 8] = tens(n)
        o += co
    merged["diag"] = W
    panels = {}
    for n, (s, t) in shapes.items():
        if len(s) == 4 and not n.startswith(("cat", "diag")):
            for fd in (0, 1):
                panels[(n, fd)] = _pack(L, tens(n).contiguous(), t, fd, mode)
    for n in ("cat", "diag"):
        for fd in (0, 1):
            panels[(n, fd)] = _pack(L, merged[n], 0, fd, mode)
    return panels, merged


def _placed_jobs(L, flat_p, placed, mode):
    tensors, offs, _ = layout()
    shapes = {n: (s, t) for n, s, t in tensors}
    jobs = []
    for name, fd, dst, K, N, ko, no in placed:
        s, t = shapes[name]
        jobs.append(L.ConvPackPlacedJob(flat_p.data_ptr() + 4 * offs[name], dst.data_ptr(), s[0], s[1], s[2], s[3], t, fd, mode, K, N, ko, no))
    return (L.ConvPackPlacedJob * len(jobs))(*jobs), len(jobs)


def _same_bytes(a, b):
    return torch.equal(a.contiguous().view(torch.uint8).reshape(-1), b.contiguous().view(torch.uint8).reshape(-1))


@pytest.mark.parametrize("mode_name", ["CONV_BF16", "CONV_F32X3", "CONV_F32"])
def test_packed_step_equals_step_then_pack(mode_name):
    from liso_amd import _lib as L

    dev = torch.device("cuda")
    mode = getattr(L, mode_name)
    lib = L.lib()
    _, offs, total = layout()
    gd = _Guarded(dev)
    arr, n_items, panels, mirrors, placed = build_items(L, lambda nb: gd.raw(nb, PATTERN), lambda shape: gd.f32(shape, 0), mode)
    image, blocks = table_image(L, arr, n_items, total)
    table = gd.raw(image.numel(), 0)
    table.copy_(image)
    gen = torch.Generator().manual_seed(11)
    p, g, m, v = (gd.f32((total,)) for _ in range(4))
    p.copy_(torch.randn(total, generator=gen) * 0.05)
    m.copy_(torch.randn(total, generator=gen) * 1e-3)
    v.copy_(torch.rand(total, generator=gen) * 1e-5)
    rp, rm, rv = p.clone(), m.clone(), v.clone()

    def compare(what):
        ref_panels, merged = _reference(L, rp, mode)
        torch.cuda.synchronize()
        for key, (dst, K, N, taps) in panels.items():
            assert _same_bytes(dst, ref_panels[key]), (what, key, "panel bytes")
        return merged

    # the initial fill: panels start as a non-zero pattern; liso_conv_pack_weights_placed(clear = 1) alone must give every byte
    jobs, n_jobs = _placed_jobs(L, p, placed, mode)
    L.check(lib.liso_conv_pack_weights_placed(jobs, n_jobs, 1, L.stream_ptr()), "placed")
    compare("initial fill")
    gd.check()
    # (the mirrors are allocated as zeros, like the panels' padding: the off-diagonal blocks of the merged filter are never written)

    for step, (lr, beta1) in enumerate([(1e-3, 0.95), (3e-3, 0.9), (7e-4, 0.85)], start=1):
        g.copy_(torch.randn(total, generator=gen) * (10.0 ** (step - 3)))
        args = (lr, beta1, 0.999, 1e-8, 0.01, 0.5)
        L.check(lib.liso_adamw_step_scaled_f32(L.ptr(rp), L.ptr(g), L.ptr(rm), L.ptr(rv), total, *args, step, L.stream_ptr()), "ref step")
        L.check(lib.liso_adamw_step_packed_f32(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), total, *args, step, L.ptr(table), blocks,
                                               L.stream_ptr()), "packed step")
        merged = compare(f"step {step}")
        assert _same_bytes(p, rp) and _same_bytes(m, rm) and _same_bytes(v, rv), step
        for k, t in mirrors.items():
            assert _same_bytes(t, merged[k]), (step, k, "mirror")
        gd.check()

    # liso_conv_pack_weights_placed alone, as the repack: values over a stale panel, nothing else touched
    for dst, _, _, _ in panels.values():
        dst.fill_(PATTERN)
    L.check(lib.liso_conv_pack_weights_placed(jobs, n_jobs, 0, L.stream_ptr()), "placed")
    ref_panels, _ = _reference(L, rp, mode)
    torch.cuda.synchronize()
    for key, (dst, K, N, taps) in panels.items():
        ref = ref_panels[key]
        assert bool(((dst == ref) | ((dst == PATTERN) & (ref == 0))).all()), key  # what was not written is zero padding
    assert bool((panels[("w33", 0)][0] == PATTERN).any())  # (K = 8 of Kp = 16: a whole chunk of padding per column)
    L.check(lib.liso_conv_pack_weights_placed(jobs, n_jobs, 1, L.stream_ptr()), "placed")
    compare("repack")
    gd.check()


def test_wrong_table_launch_writes_nothing():
    """a table planned for another buffer length is refused on the device: the launch leaves every buffer as it was"""
    from liso_amd import _lib as L

    dev = torch.device("cuda")
    _, _, total = layout()
    gd = _Guarded(dev)
    arr, n_items, panels, mirrors, placed = build_items(L, lambda nb: gd.raw(nb, PATTERN), lambda shape: gd.f32(shape, 0), L.CONV_BF16)
    image, blocks = table_image(L, arr, n_items, total)
    table = gd.raw(image.numel(), 0)
    table.copy_(image)
    p, g, m, v = (gd.f32((total + 64,), 0) for _ in range(4))
    p.fill_(1.0), g.fill_(1.0)
    L.check(L.lib().liso_adamw_step_packed_f32(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), total + 64, 1e-3, 0.9, 0.999, 1e-8, 0.01, 1.0, 1,
                                               L.ptr(table), blocks, L.stream_ptr()), "packed step")
    gd.check()
    assert bool((p == 1.0).all()) and bool((m == 0).all()) and bool((v == 0).all())
    for dst, _, _, _ in panels.values():
        assert bool((dst == PATTERN).all())
