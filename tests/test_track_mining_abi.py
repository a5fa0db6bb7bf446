"""CPU: the track-mining ABI (include/liso_track_mining.h) -- every prototype of the header matches its ctypes signature argument by
argument, the workspace query refuses what the LDS plans cannot hold, every entry point refuses bad arguments before it launches
anything, and the Python constants are the header's."""
import ctypes
import os
import re

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
EINVAL, EWORKSPACE = -1, -2
SCALARS = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "size_t": ctypes.c_size_t, "long": ctypes.c_long}


def _lib():
    from liso_amd import _lib as L

    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return L


def _header():
    txt = open(os.path.join(ROOT, "include", "liso_track_mining.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def _prototypes():
    """name -> (return ctype, [argument ctypes]) parsed from the header"""
    out = {}
    for ret, name, args in re.findall(r"\b(int|size_t)\s+(liso_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", _header()):
        types = []
        for arg in args.split(","):
            arg = " ".join(arg.split())
            types.append(ctypes.c_void_p if "*" in arg else SCALARS[arg.replace("const ", "").rsplit(" ", 1)[0]])
        out[name] = (SCALARS[ret], types)
    return out


def test_prototypes_match_the_ctypes_signatures():
    L = _lib()
    protos = _prototypes()
    assert set(protos) == {"liso_track_mining_workspace_bytes", "liso_select_tracks", "liso_refine_tracks_apply", "liso_export_tracks"}
    for name, (ret, args) in protos.items():
        assert hasattr(L.lib(), name) and name in L.SIGNATURES, name
        got_ret, got_args = L.SIGNATURES[name]
        assert got_ret is ret, name
        assert len(got_args) == len(args), (name, len(got_args), len(args))
        for i, (g, w) in enumerate(zip(got_args, args)):
            assert g is w, (name, i, g, w)


def test_constants_are_the_headers():
    from liso_amd.tracker import track_mining as TM
    from liso_amd.tracker.track_smoothing import MIN_TRACK_LEN_FOR_SMOOTHING

    defs = {k: int(v) for k, v in re.findall(r"#define\s+(LISO_MINE_[A-Z_]+)\s+(\d+)", _header())}
    assert (TM.AGE_OK, TM.CONF_OK, TM.KEPT, TM.SMOOTHED) == tuple(defs["LISO_MINE_" + k] for k in ("AGE_OK", "CONF_OK", "KEPT", "SMOOTHED"))
    assert (TM.MAX_FRAMES, TM.MAX_TRACKS) == (defs["LISO_MINE_MAX_FRAMES"], defs["LISO_MINE_MAX_TRACKS"])
    assert defs["LISO_MINE_MIN_TRACK_LEN_FOR_SMOOTHING"] == MIN_TRACK_LEN_FOR_SMOOTHING


def test_workspace_query_refuses_what_the_lds_plans_cannot_hold():
    lib = _lib().lib()
    ws = lib.liso_track_mining_workspace_bytes
    assert ws(2, 12, 6, 15, 8) >= 2 * 8 * 12 * 4
    assert ws(0, 12, 6, 15, 8) > 0  # an empty batch is fine
    assert ws(2, 1024, 6, 15, 8192) > 0
    assert ws(2, 1025, 6, 15, 8) == 0 and ws(2, 12, 6, 15, 8193) == 0  # LISO_MINE_MAX_FRAMES, LISO_MINE_MAX_TRACKS
    for bad in ((-1, 12, 6, 15, 8), (2, 0, 6, 15, 8), (2, 12, 0, 15, 8), (2, 12, 6, 0, 8), (2, 12, 6, 15, 0)):
        assert ws(*bad) == 0, bad
    sizes = [ws(s, 12, 6, 15, 8) for s in (1, 2, 4, 8)]
    assert sizes == sorted(sizes)


def test_entry_points_refuse_bad_arguments_before_launching():
    lib = _lib().lib()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 255) // 256 * 256)  # never touched: every call below returns first
    big = 1 << 30

    def select(S=2, T=12, K=6, cap=15, M=8, rows=p, q=0.6, age=p, ws=p, wsb=big):
        return lib.liso_select_tracks(S, T, K, cap, M, rows, p, p, p, p, p, p, 4, 0.5, 1.0, 0.1, 0, 3.0, 5.0, 1, q, age, p, p, p, p, p, p, p, p, p, p,
                                      p, p, ws, wsb, None)

    assert select(T=1025) == EINVAL and select(M=8193) == EINVAL and select(S=-1) == EINVAL and select(K=0) == EINVAL and select(cap=0) == EINVAL
    assert select(rows=None) == EINVAL and select(age=None) == EINVAL and select(ws=None) == EINVAL and select(q=1.5) == EINVAL
    assert select(ws=ctypes.c_void_p(p.value + 4)) == EINVAL
    assert select(wsb=lib.liso_track_mining_workspace_bytes(2, 12, 6, 15, 8) - 1) == EWORKSPACE
    assert select(S=0) == 0  # empty: nothing to launch

    def apply(S=2, T=12, M=8, verdict=p, count=p, fit=p, fit_rot=1, out=p):
        return lib.liso_refine_tracks_apply(S, T, M, verdict, p, p, p, p, p, p, p, p, p, count, fit, fit_rot, 0, 0.1, out, p, p, p, p, p, p, None)

    assert apply(T=0) == EINVAL and apply(T=1025) == EINVAL and apply(M=0) == EINVAL and apply(verdict=None) == EINVAL and apply(out=None) == EINVAL
    assert apply(count=None) == EINVAL and apply(fit=None) == EINVAL and apply(count=None, fit=None) == EINVAL  # a fit is asked for
    assert apply(S=0) == 0

    def export(S=2, T=12, K=6, cap=15, M=8, cap_out=6, verdict=p, fov=p, fov_only=1, n_boxes=p, ws=p, wsb=big):
        return lib.liso_export_tracks(S, T, K, cap, M, cap_out, verdict, p, p, p, p, p, p, p, p, p, fov, fov_only, p, p, n_boxes, p, p, p, p, p, p, p,
                                      p, p, p, ws, wsb, None)

    assert export(cap_out=0) == EINVAL and export(T=1025) == EINVAL and export(M=8193) == EINVAL and export(verdict=None) == EINVAL
    assert export(fov=None) == EINVAL and export(n_boxes=None) == EINVAL and export(ws=None) == EINVAL
    assert export(wsb=100) == EWORKSPACE
    assert export(S=0) == 0
