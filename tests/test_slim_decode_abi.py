"""CPU: the C ABI of include/liso_slim_decode.h -- exported symbols, structure mirrors, and every refusal that returns before a launch:
bad modes, a forced class logit without extrema, pc_stride < 3, more than 8 flow types, a small workspace, samples * h * w >= 2^31."""
import ctypes

SYMBOLS = ("liso_slim_decode_weights_fwd", "liso_slim_decode_weights_bwd", "liso_slim_decode_points_fwd", "liso_slim_decode_points_bwd",
           "liso_slim_loss_workspace_bytes", "liso_slim_static_points_loss_fwd", "liso_slim_static_points_loss_bwd", "liso_slim_knn_queries",
           "liso_slim_nearest_point_loss_fwd", "liso_slim_nearest_point_loss_bwd", "liso_channel_extrema_workspace_bytes",
           "liso_channel_extrema_f32")
EINVAL, EWORKSPACE = -1, -2
ONE = ctypes.c_void_p(8)  # a non-null pointer that is never dereferenced: every call below returns before it launches


def _cfg(samples=2, n=5, h=5, w=7, modes=(0, 0, 0, 0)):
    from liso_amd import _lib

    c = _lib.SlimDecodeCfg()
    c.samples, c.n, c.h, c.w = samples, n, h, w
    for i, m in enumerate(modes):
        c.logit_mode[i] = m
    c.overwrite_flow = c.overwrite_logits = 1
    c.dyn_grad_scale = 1.0
    c.ext_lo[0], c.ext_lo[1], c.ext_span[0], c.ext_span[1] = -10.0, -24.0, 20.0, 56.0
    return c


def _decode_calls(lib, cfg, extrema, out):
    """the four decode entry points with non-null fakes everywhere but `extrema`"""
    c = ctypes.byref(cfg)
    return (lib.liso_slim_decode_weights_fwd(c, ONE, ONE, ONE, extrema, ONE, 3, ONE, ONE, ONE, None),
            lib.liso_slim_decode_weights_bwd(c, ONE, ONE, ONE, extrema, ONE, ONE, ONE, None),
            lib.liso_slim_decode_points_fwd(c, ONE, ONE, ONE, extrema, ONE, ONE, ctypes.byref(out), None),
            lib.liso_slim_decode_points_bwd(c, ONE, ONE, ONE, extrema, ONE, ONE, ctypes.byref(out), ONE, ONE, None))


def test_library_exports_the_symbols_and_the_structures_mirror_the_header():
    from liso_amd import _lib

    lib = _lib.lib()
    for s in SYMBOLS:
        assert s in _lib.SIGNATURES and hasattr(lib, s), s
    # int, long, 2 int, int[4], 6 int, float, (pad), double[2], double[2]
    assert ctypes.sizeof(_lib.SlimDecodeCfg) == 104 and _lib.SlimDecodeCfg.ext_lo.offset == 72 and _lib.SlimDecodeCfg.logit_mode.offset == 24
    assert ctypes.sizeof(_lib.SlimDecodeOut) == 12 * ctypes.sizeof(ctypes.c_void_p)
    assert ctypes.sizeof(_lib.SlimNpLossCfg) == 48 and _lib.SlimNpLossCfg.ext.offset == 24
    assert lib.liso_slim_loss_workspace_bytes() == (2 * 512 + 2) * 8  # block partials of 512 blocks + (sum, count)
    assert lib.liso_channel_extrema_workspace_bytes() == 512 * 8 * 4


def test_decode_refuses_bad_modes_and_grids_before_any_launch():
    from liso_amd import _lib

    lib = _lib.lib()
    out = _lib.SlimDecodeOut()
    for bad in (_cfg(modes=(0, 3, 0, 0)), _cfg(modes=(-1, 0, 0, 0)), _cfg(modes=(0, 0, 0, 7)), _cfg(samples=0), _cfg(h=0), _cfg(w=0), _cfg(n=-1),
                _cfg(samples=2, h=32768, w=32768), _cfg(samples=1 << 11, h=1 << 10, w=1 << 10)):  # samples * h * w >= 2^31
        assert _decode_calls(lib, bad, ONE, out) == (EINVAL,) * 4
    assert lib.liso_slim_decode_weights_fwd(None, ONE, ONE, ONE, ONE, ONE, 3, ONE, ONE, ONE, None) == EINVAL
    ok = _cfg()
    assert lib.liso_slim_decode_weights_fwd(ctypes.byref(ok), ONE, ONE, ONE, None, ONE, 2, ONE, ONE, ONE, None) == EINVAL  # pc_stride < 3
    assert lib.liso_slim_decode_weights_fwd(ctypes.byref(ok), None, ONE, ONE, None, ONE, 3, ONE, ONE, ONE, None) == EINVAL
    assert lib.liso_slim_decode_points_fwd(ctypes.byref(ok), ONE, ONE, ONE, None, ONE, ONE, None, None) == EINVAL  # no output structure
    assert lib.liso_slim_decode_points_bwd(ctypes.byref(ok), ONE, ONE, ONE, None, ONE, ONE, ctypes.byref(out), None, ONE, None) == EINVAL
    assert _decode_calls(lib, _cfg(n=0), None, out) == (0,) * 4  # no rows: nothing launched, nothing needed


def test_decode_refuses_a_forced_class_logit_without_extrema():
    """the kernels read extrema[0..7] exactly when logit_mode[1..3] holds ON / OFF; the disappearing logit's constants need none"""
    from liso_amd import _lib

    lib = _lib.lib()
    out = _lib.SlimDecodeOut()
    for ch in (1, 2, 3):
        for mode in (1, 2):
            modes = [0, 0, 0, 0]
            modes[ch] = mode
            assert _decode_calls(lib, _cfg(modes=modes), None, out) == (EINVAL,) * 4, modes
            assert _decode_calls(lib, _cfg(n=0, modes=modes), None, out) == (0,) * 4


def test_losses_and_queries_refuse_bad_sizes_before_any_launch():
    from liso_amd import _lib

    lib = _lib.lib()
    ws = lib.liso_slim_loss_workspace_bytes()
    st = lib.liso_slim_static_points_loss_fwd
    assert st(2, 5, ONE, 2, ONE, ONE, ONE, ONE, ONE, ONE, ws, None) == EINVAL      # pc_stride < 3
    assert st(2, 5, ONE, 3, ONE, ONE, ONE, ONE, ONE, ONE, ws - 1, None) == EINVAL  # small workspace
    assert st(0, 5, ONE, 3, ONE, ONE, ONE, ONE, ONE, ONE, ws, None) == EINVAL
    assert st(2, 5, ONE, 3, ONE, ONE, ONE, ONE, ONE, None, ws, None) == EINVAL
    assert st(2, 5, None, 3, ONE, ONE, ONE, ONE, ONE, ONE, ws, None) == EINVAL
    sb = lib.liso_slim_static_points_loss_bwd
    assert sb(2, 5, ONE, 2, ONE, ONE, ONE, ONE, ONE, ONE, ONE, ONE, None) == EINVAL
    assert sb(2, 5, ONE, 3, ONE, ONE, ONE, ONE, None, ONE, ONE, ONE, None) == EINVAL  # no upstream gradient
    assert sb(2, 0, None, 3, None, None, None, None, ONE, ONE, None, None, None) == 0
    kq = lib.liso_slim_knn_queries
    flows = (ctypes.c_void_p * 9)(*[8] * 9)
    assert kq(2, 1, 5, 9, ONE, 3, ONE, flows, None, ONE, None) == EINVAL   # types > 8
    assert kq(2, 1, 5, 0, ONE, 3, ONE, flows, None, ONE, None) == EINVAL
    assert kq(2, 0, 5, 3, ONE, 3, ONE, flows, None, ONE, None) == EINVAL   # clouds < 1
    assert kq(2, 1, 5, 3, ONE, 2, ONE, flows, None, ONE, None) == EINVAL   # pc_stride < 3
    assert kq(2, 1, 5, 3, ONE, 3, ONE, None, None, ONE, None) == EINVAL
    holes = (ctypes.c_void_p * 3)(8, None, 8)
    assert kq(2, 1, 5, 3, ONE, 3, ONE, holes, None, ONE, None) == EINVAL   # a missing flow pointer among the first `types`
    assert kq(2, 1, 0, 3, None, 3, None, flows, None, None, None) == 0
    np_cfg = lambda **kw: _lib.SlimNpLossCfg(**dict(dict(samples=2, clouds=1, n=5, n_b=4, fov_mode=1, delta=0.1), **kw))  # noqa: E731
    nf, nb = lib.liso_slim_nearest_point_loss_fwd, lib.liso_slim_nearest_point_loss_bwd
    fwd = lambda c, ps=3, cs=3, w=ws: nf(ctypes.byref(c), ONE, ps, ONE, ONE, ONE, cs, ONE, None, ONE, ONE, ONE, w, None)  # noqa: E731
    bwd = lambda c, ps=3, cs=3: nb(ctypes.byref(c), ONE, ps, ONE, ONE, ONE, cs, ONE, None, ONE, None, ONE, ONE, None)  # noqa: E731
    for bad in (np_cfg(fov_mode=3), np_cfg(fov_mode=-1), np_cfg(delta=-0.1), np_cfg(n_b=0), np_cfg(clouds=0), np_cfg(samples=0), np_cfg(n=-1)):
        assert fwd(bad) == EINVAL and bwd(bad) == EINVAL
    assert fwd(np_cfg(), ps=2) == EINVAL and fwd(np_cfg(), cs=2) == EINVAL and fwd(np_cfg(), w=ws - 8) == EINVAL
    assert bwd(np_cfg(), ps=2) == EINVAL and bwd(np_cfg(), cs=2) == EINVAL
    assert bwd(np_cfg(n=0)) == 0
    ce = lib.liso_channel_extrema_f32
    cws = lib.liso_channel_extrema_workspace_bytes()
    assert ce(ONE, 0, 8, 4, ONE, ONE, cws, None) == EINVAL and ce(ONE, 10, 8, 5, ONE, ONE, cws, None) == EINVAL
    assert ce(ONE, 10, 3, 4, ONE, ONE, cws, None) == EINVAL and ce(None, 10, 8, 4, ONE, ONE, cws, None) == EINVAL
    assert ce(ONE, 10, 8, 4, ONE, ONE, cws - 1, None) == EWORKSPACE
