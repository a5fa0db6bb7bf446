"""CPU: the sample preparation ABI (include/liso_sample_prep.h) is exported with the declared signatures, its workspace queries
behave, and every entry point refuses bad arguments before it launches anything; the Python wrappers refuse CPU tensors."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
EINVAL, EWORKSPACE = -1, -2
_C = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "double": ctypes.c_double}
INF = float("inf")


def _lib():
    from liso_amd import _lib as L

    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return L


def _declarations():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "liso_sample_prep.h")).read(), flags=re.S)
    out = {}
    for ret, name, args in re.findall(r"\b(int|size_t)\s+(liso_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", txt):
        out[name] = (_C[ret], [ctypes.c_void_p if "*" in a else _C[a.split()[-2]] for a in args.split(",")])
    return out


def _buffers():
    buf = ctypes.create_string_buffer(8192)
    p = (ctypes.addressof(buf) + 255) // 256 * 256  # never touched: every call below returns first
    return buf, ctypes.c_void_p(p), ctypes.c_void_p(p + 2048), ctypes.c_void_p(p + 4096)


def test_symbols_and_signatures_match_the_header():
    L = _lib()
    lib = L.lib()
    decl = _declarations()
    assert set(decl) == {"liso_sample_transform_f32", "liso_sample_transform_poses_f64", "liso_bev_crop_workspace_bytes", "liso_bev_crop_f32",
                         "liso_bev_point_maps_workspace_bytes", "liso_bev_point_maps_f32"}
    for name, (res, args) in decl.items():
        assert hasattr(lib, name), name
        assert L.SIGNATURES[name] == (res, args), name
    from liso_amd.datasets import sample_prep as S

    # liso_bev_crop_cfg: 5 ints, padding, 4 doubles; the job structs: 3 pointers + 3 ints, 3 pointers
    assert ctypes.sizeof(S.CropCfg) == 56 and S.CropCfg.range_x.offset == 24
    assert ctypes.sizeof(S.BoxJob) == 40 and ctypes.sizeof(S.OdomJob) == 24
    hdr = open(os.path.join(ROOT, "include", "liso_sample_prep.h")).read()
    assert f"#define LISO_SAMPLE_MAX_JOBS {S.MAX_JOBS}" in hdr
    mk = open(os.path.join(ROOT, "liso_amd", "csrc", "Makefile")).read()
    assert "FLAGS_sample_prep := -ffp-contract=off" in mk


def test_workspace_queries():
    lib = _lib().lib()
    q = lib.liso_bev_crop_workspace_bytes
    assert q(0, 10) == 0 and q(1, 0) == 0 and q(1, (1 << 24) + 1) == 0
    assert q(2, 1000) >= 2 * 2 * 1000 * 4 and q(2, 2000) > q(2, 1000)
    m = lib.liso_bev_point_maps_workspace_bytes
    for bad in ((0, 8, 8, 1), (1, 0, 8, 1), (1, 8, 0, 1), (1, 8, 8, 3), (1, 8, 8, -1), (1, 1 << 13, 1 << 13, 1)):
        assert m(*bad) == 0, bad
    cells = 2 * 64 * 48
    assert m(2, 64, 48, 0) >= cells * 4
    assert m(2, 64, 48, 1) >= cells * (4 + 3 * 4 + 3 * 8)
    assert m(2, 64, 48, 2) >= cells * (4 + 2 * (3 * 4 + 3 * 8)) and m(2, 64, 48, 2) > m(2, 64, 48, 1) > m(2, 64, 48, 0)


def test_transform_refuses_bad_arguments_before_launching():
    lib = _lib().lib()
    _, p, q, r = _buffers()

    def tf(b=2, n=10, stride=4, T=p, pcl=q, flow=None, out=r, out_flow=None):
        return lib.liso_sample_transform_f32(b, n, stride, T, pcl, None, flow, out, out_flow, None)

    assert tf(b=0) == EINVAL and tf(n=-1) == EINVAL and tf(stride=2) == EINVAL and tf(n=(1 << 24) + 1) == EINVAL
    assert tf(T=None) == EINVAL and tf(pcl=None) == EINVAL and tf(out=None) == EINVAL
    assert tf(flow=p) == EINVAL and tf(out_flow=p) == EINVAL  # flow and out_flow go together
    assert tf(out=ctypes.c_void_p(q.value + 16)) == EINVAL  # partial overlap; out == pcl is in place and allowed
    assert tf(n=0) == EINVAL and tf(n=0, pcl=None, out=None) == 0  # empty: nothing to launch


def test_poses_refuse_bad_arguments_before_launching():
    L = _lib()
    lib = L.lib()
    from liso_amd.datasets.sample_prep import BoxJob, OdomJob

    _, p, q, r = _buffers()
    box = lambda **k: (BoxJob * 1)(BoxJob(**{**dict(pos=q.value, rot=r.value, valid=None, k=4, pos_dim=3, is_f64=1), **k}))  # noqa: E731
    odo = lambda **k: (OdomJob * 1)(OdomJob(**{**dict(in_=q.value, out=r.value, out_inv=None), **k}))  # noqa: E731
    call = lambda b, T, bx, nb, od, no: lib.liso_sample_transform_poses_f64(b, T, bx, nb, od, no, None)  # noqa: E731
    assert call(0, p, box(), 1, None, 0) == EINVAL and call(1, None, box(), 1, None, 0) == EINVAL
    assert call(1, p, None, 1, None, 0) == EINVAL and call(1, p, None, 0, None, 1) == EINVAL
    assert call(1, p, box(), -1, None, 0) == EINVAL and call(1, p, box(), 17, None, 0) == EINVAL and call(1, p, None, 0, odo(), 17) == EINVAL
    assert call(1, p, box(k=-1), 1, None, 0) == EINVAL and call(1, p, box(pos_dim=4), 1, None, 0) == EINVAL
    assert call(1, p, box(is_f64=2), 1, None, 0) == EINVAL and call(1, p, box(pos=None), 1, None, 0) == EINVAL
    assert call(1, p, box(rot=None), 1, None, 0) == EINVAL
    assert call(1, p, None, 0, odo(in_=None), 1) == EINVAL and call(1, p, None, 0, odo(out=None), 1) == EINVAL
    assert call(1, p, None, 0, odo(out_inv=r.value), 1) == EINVAL  # the inverse may not alias the result
    assert call(1, p, None, 0, None, 0) == 0  # nothing to do


def test_crop_refuses_bad_arguments_before_launching():
    L = _lib()
    lib = L.lib()
    from liso_amd.datasets.sample_prep import CropCfg

    _, p, q, r = _buffers()

    def crop(cfg=True, pcl=p, out=q, coors=r, counts=r, ws=p, wsb=1 << 30, flow=None, out_flow=None, rows=None, out_rows=None, attr=None,
             out_attr=None, **k):
        c = CropCfg(**{**dict(batch=2, n_max=100, point_stride=4, grid_x=64, grid_y=64, range_x=40.0, range_y=40.0, z_min=-INF, z_max=INF), **k})
        return lib.liso_bev_crop_f32(ctypes.byref(c) if cfg else None, pcl, None, None, flow, rows, attr, out, out_flow, out_rows, out_attr,
                                     coors, counts, ws, wsb, None)

    assert crop(cfg=False) == EINVAL
    assert crop(batch=0) == EINVAL and crop(n_max=-1) == EINVAL and crop(point_stride=2) == EINVAL
    assert crop(grid_x=0) == EINVAL and crop(grid_y=-3) == EINVAL and crop(grid_x=1 << 13, grid_y=1 << 13) == EINVAL
    assert crop(range_x=0.0) == EINVAL and crop(range_y=-1.0) == EINVAL and crop(range_x=INF) == EINVAL and crop(range_y=float("nan")) == EINVAL
    assert crop(z_min=float("nan")) == EINVAL
    assert crop(pcl=None) == EINVAL and crop(out=None) == EINVAL and crop(coors=None) == EINVAL and crop(counts=None) == EINVAL
    assert crop(ws=None) == EINVAL and crop(out=p) == EINVAL  # not in place
    assert crop(flow=p) == EINVAL and crop(out_flow=p) == EINVAL and crop(rows=p) == EINVAL and crop(out_attr=p) == EINVAL
    assert crop(wsb=lib.liso_bev_crop_workspace_bytes(2, 100) - 1) == EWORKSPACE
    assert crop(n_max=0) == EINVAL  # N == 0 with non-null arrays


def test_maps_refuse_bad_arguments_before_launching():
    lib = _lib().lib()
    _, p, q, r = _buffers()

    def maps(b=2, n=100, stride=4, gx=16, gy=16, pcl=p, coors=q, flow0=p, flow1=None, odom=None, thr=0.05, occ=r, bev0=r, bev1=None, mask=None,
             ws=p, wsb=1 << 30):
        return lib.liso_bev_point_maps_f32(b, n, stride, gx, gy, pcl, None, coors, flow0, flow1, odom, thr, occ, bev0, bev1, mask, ws, wsb, None)

    assert maps(b=0) == EINVAL and maps(n=-1) == EINVAL and maps(stride=2) == EINVAL
    assert maps(gx=0) == EINVAL and maps(gy=0) == EINVAL and maps(gx=1 << 13, gy=1 << 13) == EINVAL
    assert maps(coors=None) == EINVAL and maps(ws=None) == EINVAL and maps(ws=ctypes.c_void_p(p.value + 4)) == EINVAL
    assert maps(flow0=None) == EINVAL  # a flow map without its flow
    assert maps(bev1=r) == EINVAL and maps(bev0=None, bev1=r, flow1=p) == EINVAL
    assert maps(mask=r) == EINVAL and maps(mask=r, odom=p, pcl=None) == EINVAL and maps(mask=r, odom=p, thr=float("nan")) == EINVAL
    assert maps(wsb=lib.liso_bev_point_maps_workspace_bytes(2, 16, 16, 1) - 1) == EWORKSPACE


def test_python_wrappers_refuse_cpu_tensors():
    L = _lib()
    from liso_amd.datasets import sample_prep as S
    from liso_amd.datasets import torch_dataset_commons as tdc
    from liso_amd.kabsch.shape_utils import Shape

    T = np.eye(4)
    kw = dict(bev_range_m=(40.0, 40.0), img_grid_size=(64, 64))
    with pytest.raises(L.LisoHipError, match="CPU tensor"):
        tdc.transform_pcl_maybe_with_intensity(torch.zeros(8, 4), T)
    with pytest.raises(L.LisoHipError, match="CPU tensor"):
        tdc.transform_flow(torch.zeros(8, 3), T)
    with pytest.raises(L.LisoHipError, match="CPU tensor"):
        tdc.transform_odometry(torch.eye(4, dtype=torch.float64), T)
    with pytest.raises(L.LisoHipError, match="CPU tensor"):
        tdc.transform_boxes(Shape(pos=torch.zeros(2, 3), dims=torch.ones(2, 3), rot=torch.zeros(2, 1), probs=torch.ones(2, 1)), T)
    with pytest.raises(L.LisoHipError, match="CPU tensor"):
        tdc.pillarize_bev(torch.zeros(2, 8, 4), **kw)
    with pytest.raises(L.LisoHipError, match="CPU tensor"):
        S.bev_point_maps(torch.zeros(8, 2, dtype=torch.int32), None, (64, 64))
    with pytest.raises(L.LisoHipError, match="CPU tensor"):
        tdc.moving_mask(torch.zeros(8, 3), torch.zeros(8, 3), torch.eye(4, dtype=torch.float64), 0.05)
    with pytest.raises(L.LisoHipError, match="C >= 3"):
        tdc.pillarize_bev(torch.zeros(8, 2), **kw)
    # every name the reference's module has is found under the same name
    for name in ("get_augmentation_transform", "augment_sample_content", "add_bev_flow", "add_bev_ground_height_occupancy_maps",
                 "assemble_bev_sample"):
        assert getattr(tdc, name) is getattr(S, name)
