"""CPU: the numpy host path of liso_amd/datasets/label_prep.py against the reference fixture tests/golden/label_prep_reference.npz
(tests/golden/make_label_prep_golden.py states the margins under which exact agreement is demanded), the ABI of
include/liso_label_prep.h, and the argument checks that return before anything is launched.

Measured: the object velocities differ from the reference by at most 4.0e-14 (printed by the test)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from liso_amd.datasets import label_prep as P
from liso_amd.datasets import torch_dataset_commons as tdc
from liso_amd.kabsch.shape_utils import Shape

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "label_prep_reference.npz"))
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
EINVAL = -1
MAP_KEYS = ("probs", "dims", "pos", "rot", "velo")


class _Cfg(dict):
    __getattr__ = dict.__getitem__


def box_cfg(dims="predict_abs_size", rot="vector", act="softplus", pos="local_relative_offset"):
    return _Cfg(dimensions_representation=_Cfg(method=dims), rotation_representation=_Cfg(method=rot),
                position_representation=_Cfg(method=pos), activations=_Cfg(dims=act))


VARIANTS = {"vec": (box_cfg(), True, False), "norm": (box_cfg(), False, True),
            "log_direct": (box_cfg("predict_log_size", "direct", "exp"), True, False), "bins": (box_cfg(rot="class_bins"), False, False)}
SCENES = {"g64": ("vec", "norm", "log_direct", "bins"), "g128": ("vec", "norm")}


def fixture_shape(prefix, to=lambda a: a):
    return Shape(**{a: to(G[f"{prefix}_{a}"]) for a in ("pos", "dims", "rot", "velo", "probs", "valid")})


def grid_range(tag):
    g, r = G[f"{tag}_grid_range"]
    return (int(g), int(g)), np.array([r, r], np.float32)


def check_filtered(got, has, tag, which, to_np=lambda a: a):
    """the compacted `[K]` result against the reference's kept boxes: the same boxes, in the same order, padding zero behind them"""
    n = G[f"{tag}_{which}_pos"].shape[0]
    valid = to_np(got.valid)
    assert valid.sum() == n and valid[:n].all()
    for a in ("pos", "dims", "rot", "velo", "probs"):
        v = to_np(getattr(got, a))
        assert np.array_equal(v[:n], G[f"{tag}_{which}_{a}"]), (tag, which, a)
        assert (v[n:] == 0).all(), (tag, which, a, "padding")
    for a in ("class_id", "difficulty"):
        assert (to_np(getattr(got, a))[n:] == 0).all()
    assert np.array_equal(to_np(has), G[f"{tag}_has_points"])


def check_maps(got, prefix, ties=None, to_np=lambda a: a):
    skip = np.zeros(G[f"{prefix}_center_bool_mask"].shape, bool)
    if ties is not None:
        assert len(ties) <= 2  # a cap on the listed cells, as tests/test_gpu_targets.py allows
        skip[ties[:, 0], ties[:, 1]] = True
    for k in MAP_KEYS:
        want, have = G[f"{prefix}_{k}"], to_np(got[k])
        assert have.dtype == np.float32 and have.shape == want.shape, (prefix, k, have.shape, want.shape)
        err = np.abs(have - want)[~skip].max()
        assert err <= 1e-4 * max(np.abs(want).max(), 1.0), (prefix, k, err)
        if skip.any():
            # the listed cells are the deliberate pair's: placed symmetrically about the cell centre at dyadic offsets, its two heats
            # are equal to the last bit in any evaluation that is odd in the offset, so both boxes win and their attributes add up
            # (the fixture holds the reference's sum)
            assert np.abs(have - want)[skip].max() <= 1e-4 * max(np.abs(want).max(), 1.0), (prefix, k, "tying cell")
            if k == "pos":
                pair = G[f"{prefix.split('_')[0]}_in_pos"][[6, 7]].sum(0)
                assert np.abs(have[skip] - pair).max() <= 1e-4 * np.abs(pair).max(), (prefix, "the pair's positions add up")
    mask = to_np(got["center_bool_mask"])
    assert mask.dtype == bool and np.array_equal(mask, G[f"{prefix}_center_bool_mask"]), prefix


@pytest.mark.parametrize("tag", list(SCENES))
def test_filter_host_matches_reference(tag):
    _, rng = grid_range(tag)
    boxes = fixture_shape(f"{tag}_in")
    nusc, has = tdc.filter_objects_to_bev_non_empty(boxes, G[f"{tag}_pcl"], bev_range_m=rng, filter_bev=False, filter_range_m=50.0)
    check_filtered(nusc, has, tag, "nusc")
    bev, has2 = tdc.filter_objects_to_bev_non_empty(boxes, G[f"{tag}_pcl"], bev_range_m=rng, box_has_points_inside=has)
    check_filtered(bev, has2, tag, "bev")
    assert np.array_equal(boxes.valid, G[f"{tag}_in_valid"])  # the input is not changed
    # the box placed exactly on the BEV edge is kept, the one outside is not
    assert (np.abs(bev.pos[bev.valid, 0]) == 50.0).sum() == 1 and (np.abs(bev.pos[:, 0]) <= 50.0).all()


@pytest.mark.parametrize("tag,variant", [(t, v) for t, vs in SCENES.items() for v in vs])
def test_draw_host_matches_reference(tag, variant):
    grid, rng = grid_range(tag)
    bcfg, scaled, normalize = VARIANTS[variant]
    boxes = fixture_shape(f"{tag}_in")
    maps = tdc.draw_heat_regression_maps(boxes, grid, rng, bcfg, per_obj_prob_scale=G[f"{tag}_scale"] if scaled else None,
                                         normalize_gaussian=normalize)
    check_maps(maps, f"{tag}_{variant}", G[f"{tag}_{variant}_ties"])


@pytest.mark.parametrize("tag", list(SCENES))
def test_gt_maps_and_ignore_mask_host(tag):
    grid, rng = grid_range(tag)
    bev = fixture_shape(f"{tag}_bev")
    check_maps(tdc.draw_heat_regression_maps(bev, grid, rng, box_cfg(), per_obj_prob_scale=G[f"{tag}_gt_scale"]), f"{tag}_gt")
    mask = tdc.create_true_where_ignore_region_mask(fixture_shape(f"{tag}_ignore"), grid, rng)
    assert mask.dtype == bool and np.array_equal(mask, G[f"{tag}_ignore_mask"])


def test_no_valid_box_host():
    boxes = fixture_shape("g64_in")
    boxes.valid = np.zeros_like(boxes.valid)
    for v in ("vec", "bins"):
        check_maps(tdc.draw_heat_regression_maps(boxes, (64, 64), np.array([100.0, 100.0], np.float32), VARIANTS[v][0]), f"empty_{v}")
    out, has = tdc.filter_objects_to_bev_non_empty(boxes, G["g64_pcl"], bev_range_m=(100.0, 100.0))
    assert not out.valid.any() and (out.pos == 0).all() and np.array_equal(has, G["g64_has_points"])
    assert not tdc.create_true_where_ignore_region_mask(boxes, (64, 64), (100.0, 100.0)).any()


def test_velocity_host_matches_reference():
    got = tdc.object_velocity_in_obj_coords(G["velo_odom"], G["velo_pose_ta"], G["velo_pose_tb"])
    err = np.abs(got - G["velo_out"]).max()
    print(f"object velocity: max |host - reference| = {err:.3e}")
    assert got.dtype == np.float64 and err <= 1e-9
    batched = tdc.object_velocity_in_obj_coords(G["velo_odom"][None], G["velo_pose_ta"][None], G["velo_pose_tb"][None])
    assert np.array_equal(batched[0], got)


def test_unsupported_methods_raise():
    boxes = fixture_shape("g64_in")
    args = (boxes, (64, 64), np.array([100.0, 100.0], np.float32))
    for bad in (box_cfg(dims="predict_rel_size"), box_cfg(rot="quaternion"), box_cfg(pos="polar")):
        with pytest.raises(NotImplementedError):
            tdc.draw_heat_regression_maps(*args, bad)
    with pytest.raises(AssertionError):
        tdc.draw_heat_regression_maps(*args, box_cfg("predict_log_size", act="softplus"))
    with pytest.raises(AssertionError):
        tdc.draw_heat_regression_maps(*args, box_cfg(), per_obj_prob_scale=G["g64_scale"], normalize_gaussian=True)
    cfg = _Cfg(loss=_Cfg(supervised=_Cfg(centermaps=_Cfg(confidence_target="speed"))))
    with pytest.raises(NotImplementedError):
        tdc.select_centermaps_target_confidence(cfg, boxes)


def sample_cfg(grid, target="gaussian"):
    return _Cfg(network=_Cfg(name="centerpoint"), data=_Cfg(bev_range_m=(100.0, 100.0), img_grid_size=(4 * grid, 4 * grid)),
                box_prediction=box_cfg(), loss=_Cfg(supervised=_Cfg(centermaps=_Cfg(active=True, confidence_target=target))))


def test_assemble_box_labels_host():
    tag, grid = "g64", 64
    boxes = fixture_shape(f"{tag}_in")
    movable = np.ones_like(boxes.valid)
    movable[0] = False
    sample = {"pcl_full_no_ground_ta": G[f"{tag}_pcl"], "mined": {"objects_ta": fixture_shape(f"{tag}_in"), "objects_tb": fixture_shape(f"{tag}_in")},
              "gt": {"objects": None, "kitti_ignore_region_boxes_ta": fixture_shape(f"{tag}_ignore")}}
    tdc.assemble_box_labels(sample, cfg=sample_cfg(grid), gt_boxes=boxes, centermaps_grid_size=(grid, grid))
    gt, mined = sample["gt"], sample["mined"]
    assert "objects" not in gt and "objects_ta" not in mined and "objects_tb" not in mined and mined["boxes"] is not None
    check_filtered(gt["boxes_nusc"], G[f"{tag}_has_points"], tag, "nusc")
    check_filtered(gt["boxes"], G[f"{tag}_has_points"], tag, "bev")
    # a scale of ones: the scaled heats are the heats, the tying cell stays the fixture's
    unscaled = tdc.draw_heat_regression_maps(fixture_shape(f"{tag}_in"), (grid, grid), (100.0, 100.0), box_cfg())
    for k in MAP_KEYS + ("center_bool_mask",):
        assert np.array_equal(mined[f"centermaps_{k}"], unscaled[k]), k
        assert gt[f"centermaps_{k}"].dtype == (bool if k == "center_bool_mask" else np.float32)
    assert np.array_equal(gt["ignore_region_is_true_mask"], G[f"{tag}_ignore_mask"])
    # the movable mask removes a box from both sets
    s2 = {"pcl_full_no_ground_ta": G[f"{tag}_pcl"]}
    tdc.assemble_box_labels(s2, cfg=sample_cfg(grid), gt_boxes=boxes, gt_object_is_movable=movable, centermaps_grid_size=(grid, grid))
    assert s2["gt"]["boxes"].valid.sum() == gt["boxes"].valid.sum() - 1 and "ignore_region_is_true_mask" not in s2["gt"]
    assert np.array_equal(s2["gt"]["boxes"].pos[0], G[f"{tag}_bev_pos"][1])
    with pytest.raises(NotImplementedError):
        tdc.assemble_box_labels({"pcl_full_no_ground_ta": G[f"{tag}_pcl"]}, cfg=sample_cfg(grid, "speed"), gt_boxes=boxes,
                                centermaps_grid_size=(grid, grid))
    # a network without a centermaps grid: a clear error where maps are asked for, none where they are not
    other = sample_cfg(grid)
    other["network"] = _Cfg(name="slim")
    with pytest.raises(ValueError, match="centermaps grid"):
        tdc.assemble_box_labels({"pcl_full_no_ground_ta": G[f"{tag}_pcl"], "mined": {"objects_ta": fixture_shape(f"{tag}_in")}}, cfg=other,
                                gt_boxes=boxes)
    s3 = tdc.assemble_box_labels({"pcl_full_no_ground_ta": G[f"{tag}_pcl"]}, cfg=other, gt_boxes=boxes)
    assert "centermaps_probs" not in s3["gt"] and s3["gt"]["boxes"].valid.sum() == gt["boxes"].valid.sum()


# ---- ABI --------------------------------------------------------------------------------------------------------------------------
def _lib():
    from liso_amd import _lib as L

    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return L


def test_structs_and_flags_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "liso_label_prep.h")).read()
    assert f"#define LISO_LABEL_MAX_ATTRS {P.MAX_ATTRS}" in hdr
    assert ctypes.sizeof(P.AttrJob) == 24 and ctypes.sizeof(P.FilterCfg) == 40 and P.FilterCfg.range_x.offset == 16
    assert ctypes.sizeof(P.TargetsExCfg) == 48 and P.TargetsExCfg.range_x.offset == 32
    mk = open(os.path.join(ROOT, "liso_amd", "csrc", "Makefile")).read()
    assert "FLAGS_label_prep := -ffp-contract=off" in mk
    L = _lib()
    for name in ("liso_box_has_points_f32", "liso_filter_boxes", "liso_object_velocity_f64", "liso_ignore_region_mask",
                 "liso_render_center_targets_ex_f32"):
        assert name in L.SIGNATURES and hasattr(L.lib(), name), name


def test_entries_refuse_bad_arguments_before_launching():
    lib = _lib().lib()
    buf = ctypes.create_string_buffer(8192)
    base = (ctypes.addressof(buf) + 255) // 256 * 256  # never touched: every call below returns first
    p, q, r = (ctypes.c_void_p(base + o) for o in (0, 2048, 4096))

    def has(b=1, k=4, n=10, stride=3, pos=p, pcl=q, flags=r):
        return lib.liso_box_has_points_f32(b, k, n, stride, pos, pos, pos, pcl, None, flags, None)

    assert has(b=0) == EINVAL and has(k=-1) == EINVAL and has(n=-1) == EINVAL and has(stride=2) == EINVAL
    assert has(pos=None) == EINVAL and has(pcl=None) == EINVAL and has(flags=None) == EINVAL and has(k=0, pos=None, flags=None) == 0

    def flt(cfg=True, pos=p, valid=q, flags=r, has_in=None, jobs=None, n=0, out_valid=r, **kw):
        c = P.FilterCfg(**{**dict(batch=1, n_boxes=4, filter_bev=1, filter_range=1, range_x=100.0, range_y=100.0, filter_range_m=50.0), **kw})
        return lib.liso_filter_boxes(ctypes.byref(c) if cfg else None, pos, valid, flags, has_in, jobs, n, out_valid, None, None)

    job = lambda **k: (P.AttrJob * 1)(P.AttrJob(**{**dict(src=p.value, dst=q.value, row_bytes=24), **k}))  # noqa: E731
    assert flt(cfg=False) == EINVAL and flt(batch=0) == EINVAL and flt(n_boxes=-1) == EINVAL and flt(range_x=0.0) == EINVAL
    assert flt(filter_range_m=float("nan")) == EINVAL and flt(pos=None) == EINVAL and flt(valid=None) == EINVAL and flt(out_valid=None) == EINVAL
    assert flt(flags=None) == EINVAL and flt(has_in=p) == EINVAL  # exactly one source of "has points"
    assert flt(out_valid=q) == EINVAL  # not in place
    assert flt(n=9) == EINVAL and flt(n=1) == EINVAL and flt(jobs=job(row_bytes=6), n=1) == EINVAL and flt(jobs=job(dst=p.value), n=1) == EINVAL
    assert flt(jobs=job(src=None), n=1) == EINVAL and flt(n_boxes=0, pos=None) == 0

    velo = lambda b=1, k=4, o=p, a=q, out=r: lib.liso_object_velocity_f64(b, k, o, a, a, out, None)  # noqa: E731
    assert velo(b=0) == EINVAL and velo(k=-1) == EINVAL and velo(o=None) == EINVAL and velo(a=None) == EINVAL and velo(out=None) == EINVAL
    assert velo(k=0) == 0

    def ign(b=1, k=4, h=8, w=8, rx=100.0, ry=100.0, pos=p, valid=q, mask=r):
        return lib.liso_ignore_region_mask(b, k, h, w, rx, ry, pos, pos, pos, valid, mask, None)

    assert ign(b=0) == EINVAL and ign(k=-1) == EINVAL and ign(h=0) == EINVAL and ign(h=1 << 13, w=1 << 13) == EINVAL and ign(rx=0.0) == EINVAL
    assert ign(ry=float("inf")) == EINVAL and ign(pos=None) == EINVAL and ign(valid=None) == EINVAL and ign(mask=None) == EINVAL

    def ren(cfg=True, pos=p, scale=None, probs=r, box_max=q, **kw):
        c = P.TargetsExCfg(**{**dict(batch=1, n_boxes=4, h=8, w=8, rot_channels=2, log_dims=0, normalize_gaussian=0, reserved=0, range_x=100.0,
                                    range_y=100.0), **kw})
        return lib.liso_render_center_targets_ex_f32(ctypes.byref(c) if cfg else None, pos, pos, pos, pos, scale, q, box_max, probs, r, r, r, r, r,
                                                     None)

    assert ren(cfg=False) == EINVAL and ren(batch=0) == EINVAL and ren(n_boxes=-1) == EINVAL and ren(h=0) == EINVAL and ren(rot_channels=3) == EINVAL
    assert ren(range_x=-1.0) == EINVAL and ren(pos=None) == EINVAL and ren(probs=None) == EINVAL and ren(box_max=None) == EINVAL
    assert ren(normalize_gaussian=1, scale=p) == EINVAL  # the scale is not defined for the normalised gaussian


def test_device_entries_refuse_cpu_tensors():
    L = _lib()
    to = torch.from_numpy
    boxes = fixture_shape("g64_in", to)
    with pytest.raises(L.LisoHipError):
        tdc.filter_objects_to_bev_non_empty(boxes, to(G["g64_pcl"]), bev_range_m=(100.0, 100.0))
    with pytest.raises(L.LisoHipError):
        tdc.draw_heat_regression_maps(boxes, (64, 64), (100.0, 100.0), box_cfg())
    with pytest.raises(L.LisoHipError):
        tdc.create_true_where_ignore_region_mask(boxes, (64, 64), (100.0, 100.0))
    with pytest.raises(L.LisoHipError):
        tdc.object_velocity_in_obj_coords(to(G["velo_odom"]), to(G["velo_pose_ta"]), to(G["velo_pose_tb"]))
    for name in ("assemble_box_labels", "filter_objects_to_bev_non_empty", "object_velocity_in_obj_coords", "draw_heat_regression_maps",
                 "create_true_where_ignore_region_mask"):
        assert getattr(tdc, name) is getattr(P, name)
