"""CPU: the odometry ABI (include/liso_odometry.h) -- every prototype of the header matches its ctypes signature argument by argument,
the configuration struct matches its ctypes mirror field by field, the workspace query refuses the sizes the kernels do not take, the
entry points refuse bad arguments before they launch anything, and the Python wrappers refuse CPU tensors and a `map_voxels` that is
not a power of two."""
import ctypes
import os
import re

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
EINVAL, EWORKSPACE = -1, -2
SCALARS = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "size_t": ctypes.c_size_t, "long": ctypes.c_long}
NAMES = {"liso_odometry_workspace_bytes", "liso_odometry_workspace_layout", "liso_odometry_preprocess", "liso_odometry_register",
         "liso_odometry_map_update", "liso_odometry_sequences", "liso_odometry_relative_f64", "liso_correct_kitti_scan_f64"}


def _lib():
    from liso_amd import _lib as L

    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return L


def _header():
    txt = open(os.path.join(ROOT, "include", "liso_odometry.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def _cfg(L, **kw):
    base = dict(n_seq=2, max_frames=5, n_max=3000, point_stride=4, map_voxels=1024, max_points_per_voxel=20, max_num_iterations=500,
                max_range=100.0, min_range=5.0, voxel_size=1.0, initial_threshold=2.0, min_motion_th=0.1, convergence_criterion=1e-4)
    base.update(kw)
    return L.OdometryCfg(**base)


def test_prototypes_match_the_ctypes_signatures():
    L = _lib()
    protos = {}
    for ret, name, args in re.findall(r"\b(int|size_t)\s+(liso_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", _header()):
        types = []
        for arg in args.split(","):
            arg = " ".join(arg.split())
            types.append(ctypes.c_void_p if "*" in arg else SCALARS[arg.replace("const ", "").rsplit(" ", 1)[0]])
        protos[name] = (SCALARS[ret], types)
    assert set(protos) == NAMES
    for name, (ret, args) in protos.items():
        assert hasattr(L.lib(), name) and name in L.SIGNATURES, name
        got_ret, got_args = L.SIGNATURES[name]
        assert got_ret is ret and len(got_args) == len(args), (name, len(got_args), len(args))
        for i, (g, w) in enumerate(zip(got_args, args)):
            assert g is w, (name, i, g, w)


def test_the_configuration_struct_and_constants_match_their_mirrors():
    L = _lib()
    body = re.search(r"typedef struct \{(.*?)\}\s*liso_odometry_cfg;", _header(), flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if decl:
            ctype, names = decl.split(" ", 1)
            fields += [(n.strip(), SCALARS[ctype]) for n in names.split(",")]
    assert fields == [(n, t) for n, t in L.OdometryCfg._fields_]
    from liso_amd.odometry import device as D, host as H

    defs = {k: int(a) << int(b or 0) for k, a, b in re.findall(r"#define\s+(LISO_ODOM_[A-Z_]+)\s+\(?(\d+)(?:\s*<<\s*(\d+))?\)?", _header())}
    assert (D.VOXEL_POINTS, D.KEY_HALF_SPAN, D.N_LAYOUT) == (defs["LISO_ODOM_VOXEL_POINTS"], defs["LISO_ODOM_KEY_HALF_SPAN"], defs["LISO_ODOM_N_LAYOUT"])
    assert H.KEY_HALF_SPAN == D.KEY_HALF_SPAN and len(D.LAYOUT) <= D.N_LAYOUT


def test_workspace_query_refuses_the_sizes_the_kernels_do_not_take():
    L = _lib()
    ws = lambda **kw: L.lib().liso_odometry_workspace_bytes(ctypes.byref(_cfg(L, **kw)))  # noqa: E731
    # at least the two map tables (key, count, 20 points per slot) and the two point tables of every sequence
    assert ws() >= 2 * (2 * 1024 * (8 + 4 + 240) + 2 * 3000 * 12)
    assert ws(n_seq=0) > 0
    sizes = [ws(n_seq=s) for s in (1, 2, 4, 8)]
    assert sizes == sorted(sizes) and len(set(sizes)) == 4
    assert ws(map_voxels=2048) - ws() >= 2 * 2 * 1024 * 252 and ws(max_frames=50) == ws()  # (nothing is kept per frame)
    for bad in (dict(n_seq=-1), dict(max_frames=0), dict(n_max=0), dict(n_max=(1 << 22) + 1), dict(point_stride=2), dict(point_stride=5),
                dict(map_voxels=1000), dict(map_voxels=32), dict(map_voxels=1 << 25), dict(map_voxels=0), dict(max_points_per_voxel=0),
                dict(max_points_per_voxel=21), dict(max_num_iterations=0), dict(max_range=5.0), dict(min_range=-1.0), dict(voxel_size=0.0),
                dict(voxel_size=1e-4), dict(initial_threshold=0.0), dict(min_motion_th=-0.1), dict(convergence_criterion=0.0),
                dict(max_range=float("nan")), dict(n_seq=1 << 20, max_frames=17)):
        assert ws(**bad) == 0, bad
    assert ws(point_stride=3) > 0 and ws(max_points_per_voxel=1) > 0 and ws(map_voxels=64) > 0
    assert L.lib().liso_odometry_workspace_bytes(None) == 0
    offsets = (ctypes.c_size_t * 16)()
    assert L.lib().liso_odometry_workspace_layout(ctypes.byref(_cfg(L)), offsets) == 0
    used = list(offsets)[:10]
    assert len(set(used)) == 10 and all(o % 256 == 0 and o < ws() for o in used) and list(offsets)[10:] == [0] * 6
    assert L.lib().liso_odometry_workspace_layout(ctypes.byref(_cfg(L, map_voxels=1000)), offsets) == EINVAL
    assert L.lib().liso_odometry_workspace_layout(ctypes.byref(_cfg(L)), None) == EINVAL


def test_the_entry_points_refuse_bad_arguments_before_launching():
    """(every call below is one that returns before it launches: the pointers are host memory)"""
    L = _lib()
    lib = L.lib()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 255) // 256 * 256)
    big = 1 << 40
    need = lib.liso_odometry_workspace_bytes(ctypes.byref(_cfg(L)))
    # entry point -> (number of required pointers, call(cfg, frame, pointers, ws, wsb)); counts, guess and sigma_given are optional
    stages = {"preprocess": (3, lambda c, f, a, ws, wsb: lib.liso_odometry_preprocess(c, f, a[0], p, a[1], a[2], ws, wsb, None)),
              "register": (5, lambda c, f, a, ws, wsb: lib.liso_odometry_register(c, f, a[0], None, None, *a[1:], ws, wsb, None)),
              "map_update": (3, lambda c, f, a, ws, wsb: lib.liso_odometry_map_update(c, f, *a, ws, wsb, None)),
              "sequences": (8, lambda c, f, a, ws, wsb: lib.liso_odometry_sequences(c, a[0], p, *a[1:], ws, wsb, None))}
    ok, empty = ctypes.byref(_cfg(L)), ctypes.byref(_cfg(L, n_seq=0))
    for name, (n, call) in stages.items():
        full = [p] * n
        assert call(ctypes.c_void_p(None), 0, full, p, big) == EINVAL, name
        for bad in (dict(map_voxels=1000), dict(max_frames=0), dict(point_stride=2), dict(n_seq=-1), dict(voxel_size=0.0)):
            assert call(ctypes.byref(_cfg(L, **bad)), 0, full, p, big) == EINVAL, (name, bad)
        if name != "sequences":
            assert call(ok, -1, full, p, big) == EINVAL and call(ok, 5, full, p, big) == EINVAL, name
        assert call(ok, 0, full, None, big) == EINVAL and call(ok, 0, full, ctypes.c_void_p(p.value + 8), big) == EINVAL, name
        assert call(ok, 0, full, p, need - 1) == EWORKSPACE, name
        for drop in range(n):
            assert call(ok, 0, [None if i == drop else p for i in range(n)], p, big) == EINVAL, (name, drop)
        assert call(empty, 0, full, p, big) == 0 and call(empty, 0, [None] * n, None, 0) == 0, name  # empty: nothing to launch
    assert lib.liso_odometry_register(ok, 1, p, p, None, p, p, p, p, p, big, None) == EINVAL  # a guess without its sigma
    assert lib.liso_odometry_register(ok, 1, p, None, p, p, p, p, p, p, big, None) == EINVAL
    assert lib.liso_odometry_relative_f64(-1, p, p, p, None) == EINVAL and lib.liso_odometry_relative_f64(0, None, None, None, None) == 0
    assert lib.liso_odometry_relative_f64(3, p, None, p, None) == EINVAL
    assert lib.liso_correct_kitti_scan_f64(-1, p, p, None) == EINVAL and lib.liso_correct_kitti_scan_f64(0, None, None, None) == 0
    assert lib.liso_correct_kitti_scan_f64(5, None, p, None) == EINVAL and lib.liso_correct_kitti_scan_f64(5, p, None, None) == EINVAL


def test_wrappers_refuse_cpu_tensors_and_bad_map_sizes():
    import torch

    L = _lib()
    from liso_amd import odometry as O

    clouds, counts, n_frames = torch.zeros(1, 2, 100, 3), torch.full((1, 2), 100, dtype=torch.int32), torch.full((1,), 2, dtype=torch.int32)
    with pytest.raises(L.LisoHipError, match="CPU tensor"):
        O.lidar_odometry(clouds, counts, n_frames, map_voxels=1024)
    with pytest.raises(L.LisoHipError, match="CPU tensor"):
        O.relative_poses(torch.eye(4, dtype=torch.float64)[None], torch.eye(4, dtype=torch.float64)[None])
    with pytest.raises(L.LisoHipError, match="CPU tensor"):
        O.correct_kitti_scan_device(torch.zeros(4, 3, dtype=torch.float64))
    from liso_amd.odometry.device import make_cfg

    for bad in (1000, 0, 32, 3 << 10):
        with pytest.raises(L.LisoHipError, match="power of two"):
            make_cfg(1, 2, 100, 3, bad)
    with pytest.raises(L.LisoHipError, match="refused"):
        make_cfg(1, 2, 100, 5, 1024)
    with pytest.raises(NotImplementedError):
        make_cfg(1, 2, 100, 3, 1024, deskew=True)
    cfg, nbytes = make_cfg(3, 6, 5760, 3, 1 << 14, max_range=30.0, min_range=1.0)
    assert cfg.voxel_size == 0.3 and nbytes > 0
