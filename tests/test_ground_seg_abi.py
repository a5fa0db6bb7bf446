"""CPU: the ground segmentation ABI (include/liso_ground.h) is exported with the declared signatures, its workspace queries
behave, and every entry point refuses bad arguments before it launches anything; the Python wrappers refuse CPU tensors."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
EINVAL, EWORKSPACE, ELENGTH = -1, -2, -4
_C = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "double": ctypes.c_double}


def _lib():
    from liso_amd import _lib as L

    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return L


def _declarations():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "liso_ground.h")).read(), flags=re.S)
    out = {}
    for ret, name, args in re.findall(r"\b(int|size_t)\s+(liso_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", txt):
        out[name] = (_C[ret], [ctypes.c_void_p if "*" in a else _C[a.split()[-2]] for a in args.split(",")])
    return out


def test_symbols_and_signatures_match_the_header():
    L = _lib()
    lib = L.lib()
    decl = _declarations()
    assert set(decl) == {"liso_ground_jcp_workspace_bytes", "liso_ground_jcp_workspace_layout", "liso_ground_jcp_f32", "liso_ground_jcp_stages_f32", "liso_ground_cone_f32",
                         "liso_ground_compact_workspace_bytes", "liso_ground_compact_f32"}
    for name, (res, args) in decl.items():
        assert hasattr(lib, name), name
        assert L.SIGNATURES[name] == (res, args), name
    # liso_ground_cfg: 5 ints, padding, 2 doubles
    assert ctypes.sizeof(L.GroundCfg) == 40 and L.GroundCfg.sensor_height.offset == 24
    hdr = open(os.path.join(ROOT, "include", "liso_ground.h")).read()
    from liso_amd.jcp import jcp

    assert f"#define LISO_GROUND_N_STAGES {jcp.N_STAGES}" in hdr and len(jcp.STAGES) == jcp.N_STAGES
    assert f"#define LISO_GROUND_MAX_HEIGHT {jcp.MAX_HEIGHT}" in hdr
    assert re.search(rf"#define LISO_GROUND_N_LAYOUT {len(jcp.LAYOUT)}\b", hdr)


def _cfg(L, b=2, n=1000, stride=3, w=2083, h=64, sh=1.73, dr=1.0):
    return L.GroundCfg(b, n, stride, w, h, sh, dr)


def test_workspace_query():
    L = _lib()
    lib = L.lib()
    q = lambda **k: lib.liso_ground_jcp_workspace_bytes(ctypes.byref(_cfg(L, **k)))  # noqa: E731
    assert lib.liso_ground_jcp_workspace_bytes(None) == 0
    one, two = q(b=1), q(b=2)
    assert one >= 2083 * 64 * 24 * 8 and 2 * one - 4096 <= two <= 2 * one  # dominated by the per-slot weights
    assert q(n=2000) > q(n=1000)
    for bad in BAD_CFGS:
        assert q(**bad) == 0, bad
    assert lib.liso_ground_compact_workspace_bytes(0, 10) == 0 and lib.liso_ground_compact_workspace_bytes(1, 0) == 0
    assert lib.liso_ground_compact_workspace_bytes(2, 1000) >= 2 * 2 * 1000 * 4


BAD_CFGS = (dict(b=0), dict(n=-1), dict(stride=2), dict(w=0), dict(h=0), dict(h=1025), dict(dr=0.0), dict(dr=-1.0), dict(dr=0.26), dict(w=32, h=64),
            dict(dr=68.0), dict(sh=float("nan")))


def test_workspace_layout():
    L = _lib()
    lib = L.lib()
    from liso_amd.jcp import jcp

    n = len(jcp.LAYOUT)
    assert jcp.LAYOUT == ("ele_key", "ele", "pix", "widx", "minz_key", "minz", "lab0", "lab1", "row_cnt", "cols", "wts")
    hdr = open(os.path.join(ROOT, "include", "liso_ground.h")).read()
    assert tuple(re.findall(r"^ \*\s+\d+ (\w+)\s+(?:uint64|fp64|int32|uint32|uint8)\s+\[B\]", hdr, flags=re.M)) == jcp.LAYOUT  # the header's list
    for kw in (dict(), dict(b=1, n=0), dict(b=3, n=777, stride=5, w=70, h=65), dict(w=1, h=1, n=1), dict(w=1025, h=1024, dr=67.0 / 255.0),
               dict(w=300, h=33, dr=40.0)):
        cfg = _cfg(L, **kw)
        offsets = (ctypes.c_size_t * (n + 1))(*([12345] * (n + 1)))
        assert lib.liso_ground_jcp_workspace_layout(ctypes.byref(cfg), offsets) == 0
        off = list(offsets)
        assert off[n] == 12345  # LISO_GROUND_N_LAYOUT entries, not one more
        off = off[:n]
        total = lib.liso_ground_jcp_workspace_bytes(ctypes.byref(cfg))
        assert off[0] == 0 and all(o % 256 == 0 for o in off) and off == sorted(off) and off[-1] <= total
        # every table fits in front of the next one, the last one in front of the end
        B, N, W, H = cfg.batch, cfg.n_max, cfg.width, cfg.height
        length = int(67.0 / cfg.delta_r)
        stride = (W * H + 15) // 16 * 16
        sizes = [B * 2 * 8, B * N * 8, B * N * 4, B * W * H * 4, B * W * length * 4, B * W * length * 8, B * stride, B * stride, B * H * 4, B * W * H * 4,
                 B * W * H * 24 * 8]
        for i in range(n):
            assert off[i] + sizes[i] <= (off[i + 1] if i + 1 < n else total), (kw, jcp.LAYOUT[i])
        assert total - off[-1] - sizes[-1] < 256
    good = (ctypes.c_size_t * n)()
    for bad in BAD_CFGS:
        assert lib.liso_ground_jcp_workspace_layout(ctypes.byref(_cfg(L, **bad)), good) == EINVAL, bad
    assert lib.liso_ground_jcp_workspace_layout(None, good) == EINVAL
    assert lib.liso_ground_jcp_workspace_layout(ctypes.byref(_cfg(L)), None) == EINVAL


def test_jcp_refuses_bad_arguments_before_launching():
    L = _lib()
    lib = L.lib()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 255) // 256 * 256)  # never touched: every call below returns first
    big = 1 << 40

    def jcp(cfg=None, pcl=p, out=p, ws=p, wsb=big, **k):
        c = cfg if cfg is not None else _cfg(L, **k)
        return lib.liso_ground_jcp_f32(ctypes.byref(c), pcl, None, out, ws, wsb, None)

    assert lib.liso_ground_jcp_f32(None, p, None, p, p, big, None) == EINVAL
    assert jcp(b=0) == EINVAL
    assert jcp(n=-1) == EINVAL
    assert jcp(stride=2) == EINVAL
    assert jcp(h=1025) == EINVAL
    assert jcp(w=32, h=64) == EINVAL
    assert jcp(dr=0.0) == EINVAL
    assert jcp(dr=0.26) == ELENGTH  # int(67 / 0.26) = 257 regions
    assert jcp(pcl=None) == EINVAL
    assert jcp(out=None) == EINVAL
    assert jcp(ws=None) == EINVAL
    assert jcp(ws=ctypes.c_void_p(p.value + 8)) == EINVAL  # workspace not 256-byte aligned
    need = lib.liso_ground_jcp_workspace_bytes(ctypes.byref(_cfg(L)))
    assert jcp(wsb=need - 1) == EWORKSPACE
    assert jcp(n=0) == EINVAL  # N == 0 with non-null arrays
    assert jcp(n=0, pcl=None, out=None, ws=None, wsb=0) == 0  # empty: nothing to launch
    stages = lambda b, e: lib.liso_ground_jcp_stages_f32(ctypes.byref(_cfg(L)), p, None, p, p, big, b, e, None)  # noqa: E731
    assert stages(-1, 3) == EINVAL and stages(0, 8) == EINVAL and stages(4, 3) == EINVAL


def test_cone_and_compact_refuse_bad_arguments_before_launching():
    lib = _lib().lib()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 255) // 256 * 256)
    q = ctypes.c_void_p(p.value + 256)

    def cone(b=2, n=100, stride=3, pcl=p, thr=-1.7, slope=0.014, out=p):
        return lib.liso_ground_cone_f32(b, n, stride, pcl, None, thr, slope, None, out, None)

    assert cone(b=0) == EINVAL and cone(n=-1) == EINVAL and cone(stride=2) == EINVAL
    assert cone(pcl=None) == EINVAL and cone(out=None) == EINVAL
    assert cone(thr=float("nan")) == EINVAL and cone(slope=float("inf")) == EINVAL
    assert cone(n=0) == EINVAL and cone(n=0, pcl=None, out=None) == 0

    def compact(b=2, n=100, stride=4, pcl=p, drop=p, out=q, counts=p, ws=p, wsb=1 << 30):
        return lib.liso_ground_compact_f32(b, n, stride, pcl, None, drop, out, counts, ws, wsb, None)

    assert compact(b=0) == EINVAL and compact(n=-1) == EINVAL and compact(stride=2) == EINVAL
    assert compact(pcl=None) == EINVAL and compact(drop=None) == EINVAL and compact(out=None) == EINVAL
    assert compact(counts=None) == EINVAL and compact(ws=None) == EINVAL
    assert compact(out=p) == EINVAL  # in place
    assert compact(wsb=lib.liso_ground_compact_workspace_bytes(2, 100) - 1) == EWORKSPACE


def test_python_wrappers_refuse_cpu_and_wrong_dtype():
    L = _lib()
    from liso_amd.jcp import jcp

    kw = dict(range_img_width=2083, range_img_height=64, sensor_height=1.73, delta_R=1)
    with pytest.raises(L.LisoHipError, match="CPU tensor"):
        jcp.jcp_device(torch.zeros(8, 3), **kw)
    with pytest.raises(L.LisoHipError, match="CPU tensor"):
        jcp.remove_ground_points(torch.zeros(2, 8, 4), **kw)
    with pytest.raises(L.LisoHipError, match="CPU tensor"):
        jcp.cone_device(torch.zeros(8, 3), -1.7, 0.8)
    with pytest.raises(L.LisoHipError, match="C >= 3"):
        jcp.jcp_device(torch.zeros(8, 2), **kw)
