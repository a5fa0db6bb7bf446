"""Flow labels and KITTI rows / columns on the host: the numpy restatement of include/liso_flow_labels.h
(liso_amd/datasets/flow_labels.py, range_projection.py) against arrays produced by the reference's own functions
(tests/golden/make_flow_labels_golden.py), the three overlap situations against a brute-force statement, and the C entry points'
argument checks.  No GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

from liso_amd.datasets import flow_labels as F
from liso_amd.datasets import range_projection as R
from liso_amd.kabsch.shape_utils import Shape

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
G = np.load(os.path.join(ROOT, "tests", "golden", "flow_labels_reference.npz"))
EINVAL = -1


def homog(p):
    return np.concatenate([p[:, :3].astype(np.float64), np.ones((p.shape[0], 1))], -1)


def assert_flow_close(flow, gold):
    """1e-9 m absolute (the fp64 noise that the LU inverse and the closed form leave for a still object is ~1e-13 m, representable in
    fp32 and different between the two) plus one fp32 ulp of the value (the one rounding to fp32)"""
    assert flow.dtype == np.float32
    tol = 1e-9 + np.spacing(np.abs(gold).astype(np.float32)).astype(np.float64)
    err = np.abs(flow.astype(np.float64) - gold)
    assert (err <= tol).all(), (err.max(), int((err > tol).sum()))


# ---- against the reference's own output -------------------------------------------------------------------------------------------
def test_kitti_extract_lidar_flow_matches_the_reference():
    flow, ids = F.extract_lidar_flow_ta_tb(pcl_homog_ta=homog(G["kitti_pcl"]), lidar_Tta_obj=G["kitti_pose_a"], obj_dims_ta=G["kitti_dims"],
                                           track_ids_ta=G["kitti_ids_a"], track_ids_tb=G["kitti_ids_b"], lidar_Ttb_obj=G["kitti_pose_b"],
                                           odom_ta_tb=G["kitti_odom"])
    assert ids.dtype == np.uint16 and np.array_equal(ids.astype(np.int64), G["kitti_ids_mask"])
    assert_flow_close(flow, G["kitti_flow"])
    ph = homog(G["kitti_pcl"])
    for k in range(G["kitti_pose_a"].shape[0]):
        mask = F.get_points_in_box_mask(ph, G["kitti_pose_a"][k], G["kitti_dims"][k])
        assert mask.dtype == bool and np.array_equal(mask, G["kitti_inside"][k])


def nusc_sample():
    """the two directions of the nuScenes fixture as `sample_flow_labels` takes them: padded clouds, the gate at t0 only"""
    p0, p1 = G["nusc_pcl_t0"], G["nusc_pcl_t1"]
    n_max = max(p0.shape[0], p1.shape[0]) + 5
    clouds = np.full((2, n_max, 3), np.nan, np.float32)
    clouds[0, :p0.shape[0]], clouds[1, :p1.shape[0]] = p0, p1
    sem = np.full((2, n_max), -7, np.int32)
    sem[0, :p0.shape[0]] = G["nusc_sem_t0"]
    odom = G["nusc_odom"]
    return dict(clouds=clouds, counts=np.array([p0.shape[0], p1.shape[0]], np.int32), poses_per_time=np.stack([G["nusc_pose_t0"], G["nusc_pose_t1"]]),
                sizes=G["nusc_size"], labels=G["nusc_ann_idx"], odoms=np.stack([odom, np.linalg.inv(odom)]),
                box_class=np.stack([G["nusc_box_class"], np.full_like(G["nusc_box_class"], -1)]), point_class=sem, directions=((0, 1), (1, 0)),
                no_label=-1)


def check_nusc(out, to_np=np.asarray):
    n0, n1 = G["nusc_pcl_t0"].shape[0], G["nusc_pcl_t1"].shape[0]
    for t, n in ((0, n0), (1, n1)):
        ids, box = to_np(out[f"track_ids_mask_t{t}"]), to_np(out[f"point_box_t{t}"])
        found = G[f"nusc_found_t{t}"]
        assert np.array_equal(box[:n] >= 0, found) and np.array_equal(ids[:n][found], G[f"nusc_idx_t{t}"][found].astype(np.int32))
        assert (ids[:n][~found] == -1).all() and (ids[n:] == -1).all() and (box[n:] == -1).all()
    assert np.array_equal(to_np(out["num_lidar_pts_t0"]), G["nusc_num_pts_t0"])  # geometric: not gated
    f01, f10 = to_np(out["flow_t0_t1"]), to_np(out["flow_t1_t0"])
    assert_flow_close(f01[:n0], G["nusc_flow_t0_t1"])
    assert_flow_close(f10[:n1], G["nusc_flow_t1_t0"])
    assert np.isnan(f01[n0:]).all() and np.isnan(f10[n1:]).all()


def test_nuscenes_gated_sample_matches_the_reference():
    check_nusc(F.sample_flow_labels(**nusc_sample()))


def av2_boxes(which, cat, to=lambda a: a):
    m = G["av2_cats"] == cat
    return Shape(pos=to(G[f"av2_pos_{which}"][m]), dims=to(G["av2_dims"][m]), rot=to(G[f"av2_rot_{which}"][m]), probs=to(np.ones((int(m.sum()), 1))))


def test_av2_update_dynamic_flow_matches_the_reference():
    ph = homog(G["av2_pcl"])
    for dtype in (np.float64, np.float32):  # the builder's fp64 array in place, and the fp32 array of the device path
        flow = G["av2_flow_rigid"].astype(dtype)
        for cat in (0, 1):
            res = F.update_dynamic_flow(ph, flow, av2_boxes("a", cat), av2_boxes("b", cat))
            assert res is flow
        assert_flow_close(flow.astype(np.float32), G["av2_flow"])
    untouched = np.abs(G["av2_flow"] - G["av2_flow_rigid"]).max(-1) == 0
    assert untouched.sum() > 2000 and np.array_equal(flow[untouched], G["av2_flow_rigid"].astype(np.float32)[untouched])


def test_rows_and_columns_match_the_reference():
    rows, cols = R.kitti_pcl_projection_get_rows_cols(G["rp_full"])
    assert rows.dtype == np.int32 and cols.dtype == np.int32
    assert np.array_equal(rows, G["rp_full_rows"]) and np.array_equal(cols, G["rp_full_cols"])
    assert np.array_equal(R.find_jumps(G["rp_short"]), G["rp_short_rows"])
    assert np.array_equal(R.find_jumps(G["rp_short"], auto_correct=True), G["rp_short_rows_corrected"])
    assert np.array_equal(R.find_cols(G["rp_short"]), G["rp_short_cols"])
    assert np.array_equal(R.find_cols(G["rp_short"], num_columns=512), G["rp_short_cols_512"])
    sample = {"pcl_t0": G["rp_full"], "pcl_t1": G["rp_short"]}
    R.add_lidar_rows_to_kitti_sample(sample, ("t0", "t1", "t2"))
    assert sample["lidar_rows_t0"].dtype == np.uint8 and np.array_equal(sample["lidar_rows_t0"], G["rp_full_rows"].astype(np.uint8))
    assert np.array_equal(sample["lidar_rows_t1"], G["rp_short_rows"].astype(np.uint8)) and "lidar_rows_t2" not in sample


# ---- the overlap rules against a brute-force statement ----------------------------------------------------------------------------
def yaw_pose(x, y, z, yaw):
    T = np.eye(4)
    T[:2, :2] = [[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]]
    T[:3, 3] = x, y, z
    return T


def two_box_scene(seed=0):
    g = np.random.default_rng(seed)
    pose_a = np.stack([yaw_pose(5.0, 1.0, -0.5, 0.3), yaw_pose(5.8, 1.4, -0.5, 0.5)])
    pose_b = np.stack([yaw_pose(6.0, 1.2, -0.5, 0.35), yaw_pose(5.0, 2.4, -0.5, 0.4)])
    size = np.array([[4.0, 2.0, 1.6], [4.2, 1.9, 1.7]])
    pcl = np.concatenate([g.uniform(2, 9, (600, 1)), g.uniform(-2, 4, (600, 1)), g.uniform(-1.5, 0.5, (600, 1))], -1).astype(np.float32)
    odom = yaw_pose(0.8, 0.0, 0.0, 0.01)
    return pcl, pose_a, pose_b, size, odom


def brute_force(pcl, pose_a, pose_b, size, odom, has_b, label, overlap, gate=None):
    """the rules in ten lines: numpy's LU inverse and matrix products, one point at a time"""
    flow = (homog(pcl) @ (np.linalg.inv(odom) - np.eye(4)).T)[:, :3]
    ids, box, count = np.full(len(pcl), -1), np.full(len(pcl), -1), np.zeros(len(size), int)
    order = range(len(size)) if overlap == F.LAST else range(len(size) - 1, -1, -1)  # FIRST: the first box is written last
    for k in order:
        for i, p in enumerate(homog(pcl)):
            inside = (np.abs((np.linalg.inv(pose_a[k]) @ p)[:3]) < size[k] / 2).all()
            count[k] += inside
            if inside and (gate is None or gate[1][k] < 0 or gate[0][i] == gate[1][k]):
                ids[i], box[i] = label[k], k
                if has_b[k]:
                    flow[i] = ((pose_b[k] @ np.linalg.inv(pose_a[k]) - np.eye(4)) @ p)[:3]
    return flow, ids, box, count


def run_host(pcl, pose_a, pose_b, size, odom, has_b, label, overlap, gate=None, **kw):
    K = len(size)
    extra = {} if gate is None else dict(point_class=np.asarray(gate[0], np.int32)[None], box_class=np.asarray(gate[1], np.int32)[None])
    return F.flow_labels_host(pcl[None], None, np.zeros(1, np.int32), odom[None], pose_a[None], pose_b[None], size[None], np.ones((1, K), bool),
                              np.asarray(has_b, bool)[None], np.asarray(label, np.int32)[None], overlap=overlap, **extra, **kw)


def check_against_brute_force(scene, has_b, overlap, gate=None):
    label = [11, 22]
    res = run_host(*scene, has_b, label, overlap, gate)
    flow, ids, box, count = brute_force(*scene, has_b, label, overlap, gate)
    assert np.array_equal(res.point_label[0], ids) and np.array_equal(res.point_box[0], box) and np.array_equal(res.count[0], count)
    assert_flow_close(res.flow[0], flow)
    return res, np.stack([F.get_points_in_box_mask(homog(scene[0]), scene[1][k], scene[3][k]) for k in range(2)])


@pytest.mark.parametrize("overlap", [F.LAST, F.FIRST])
def test_two_overlapping_partnered_boxes(overlap):
    res, inside = check_against_brute_force(two_box_scene(), [True, True], overlap)
    both = inside[0] & inside[1]
    assert both.sum() > 10 and (res.point_box[0][both] == (1 if overlap == F.LAST else 0)).all()


def test_unpartnered_box_over_a_partnered_one():
    scene = two_box_scene()
    res, inside = check_against_brute_force(scene, [True, False], F.LAST)
    both = inside[0] & inside[1]
    assert both.sum() > 10 and (res.point_label[0][both] == 22).all()  # the id of the later box ...
    partnered = run_host(*scene, [True, True], [11, 22], F.FIRST)  # ... and the flow of the earlier one
    assert np.array_equal(res.flow[0][both], partnered.flow[0][both])
    only_1 = inside[1] & ~inside[0]
    rigid = run_host(*scene, [False, False], [11, 22], F.LAST)
    assert only_1.sum() > 10 and np.array_equal(res.flow[0][only_1], rigid.flow[0][only_1])


def test_class_gated_box_over_an_ungated_one():
    scene = two_box_scene()
    point_class = np.random.default_rng(3).integers(0, 2, scene[0].shape[0])
    res, inside = check_against_brute_force(scene, [True, True], F.LAST, gate=(point_class, [-1, 1]))
    both = inside[0] & inside[1]
    assert (res.point_box[0][both & (point_class == 1)] == 1).all() and (res.point_box[0][both & (point_class == 0)] == 0).all()
    assert res.count[0][1] == inside[1].sum()  # the count is not gated


def test_keep_flow_leaves_other_points_bit_identical():
    scene = two_box_scene()
    before = np.random.default_rng(1).normal(size=(1, scene[0].shape[0], 3)).astype(np.float32)
    before[0, 5] = np.float32(np.nan)  # any bit pattern is kept
    flow = before.copy()
    res = run_host(*scene, [True, False], [11, 22], F.FIRST, keep_flow=True, flow=flow)
    assert res.flow is flow
    fresh = run_host(*scene, [True, False], [11, 22], F.FIRST)
    inside = F.get_points_in_box_mask(homog(scene[0]), scene[1][0], scene[3][0])
    assert inside.sum() > 10 and np.array_equal(flow[0][inside], fresh.flow[0][inside])
    assert np.array_equal(flow[0][~inside].view(np.uint32), before[0][~inside].view(np.uint32))


def test_rows_behind_the_count_and_nan_rows():
    pcl, pose_a, pose_b, size, odom = two_box_scene()
    pcl = pcl.copy()
    inside = F.get_points_in_box_mask(homog(pcl), pose_a[0], size[0])
    hit = np.flatnonzero(inside)[:2]
    pcl[hit[0], 1] = np.nan
    counts = np.array([400], np.int32)
    res = F.flow_labels_host(pcl[None], counts, np.zeros(1, np.int32), odom[None], pose_a[None], pose_b[None], size[None], np.ones((1, 2), bool),
                             np.ones((1, 2), bool), np.array([[11, 22]], np.int32), no_label=99)
    dead = np.arange(600) >= 400
    dead[hit[0]] = True
    assert np.isnan(res.flow[0][dead]).all() and (res.point_label[0][dead] == 99).all() and (res.point_box[0][dead] == -1).all()
    assert np.isfinite(res.flow[0][~dead]).all()
    inside[dead] = False
    assert res.count[0][0] == inside.sum()


# ---- ABI --------------------------------------------------------------------------------------------------------------------------
def _lib():
    from liso_amd import _lib as L

    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return L


def test_constants_match_the_header_and_the_makefile():
    hdr = open(os.path.join(ROOT, "include", "liso_flow_labels.h")).read()
    assert f"#define LISO_FLOW_LABELS_MAX_BOXES {F.MAX_BOXES}" in hdr and f"#define LISO_FLOW_LABELS_CHUNK {F.CHUNK}" in hdr
    assert f"#define LISO_OVERLAP_LAST {F.LAST}" in hdr and f"#define LISO_OVERLAP_FIRST {F.FIRST}" in hdr
    assert ctypes.sizeof(F.FlowLabelsCfg) == 32
    assert "FLAGS_flow_labels := -ffp-contract=off" in open(os.path.join(ROOT, "liso_amd", "csrc", "Makefile")).read()
    L = _lib()
    for name in ("liso_flow_labels_workspace_bytes", "liso_flow_labels_f32", "liso_kitti_rows_cols_f32"):
        assert name in L.SIGNATURES and hasattr(L.lib(), name), name


def test_entries_refuse_bad_arguments_before_launching():
    lib = _lib().lib()
    buf = ctypes.create_string_buffer(1 << 16)
    base = (ctypes.addressof(buf) + 255) // 256 * 256  # never touched: every call below returns first
    p, q, ws = (ctypes.c_void_p(base + o) for o in (0, 2048, 4096))

    def call(box_class=None, point_class=None, pcl=p, flow=q, cloud_of=p, odom=p, pose=p, workspace=ws, ws_bytes=None, **kw):
        c = F.FlowLabelsCfg(**{**dict(n_jobs=2, n_clouds=2, n_boxes=3, n_max=10, point_stride=3, overlap=F.LAST, keep_flow=0, no_label=-1), **kw})
        need = lib.liso_flow_labels_workspace_bytes(c.n_jobs, c.n_boxes)
        return lib.liso_flow_labels_f32(ctypes.byref(c), pcl, None, cloud_of, odom, pose, pose, p, p, p, p, box_class, point_class, flow, None, None,
                                        None, workspace, need if ws_bytes is None else ws_bytes, None)

    assert lib.liso_flow_labels_workspace_bytes(2, 3) > 0 and lib.liso_flow_labels_workspace_bytes(2, F.MAX_BOXES) > 0
    assert lib.liso_flow_labels_workspace_bytes(2, F.MAX_BOXES + 1) == 0 and lib.liso_flow_labels_workspace_bytes(0, 3) == 0
    assert call(n_boxes=F.MAX_BOXES + 1) == EINVAL  # K above the stated limit
    assert call(n_boxes=-1) == EINVAL and call(n_jobs=0) == EINVAL and call(n_jobs=-2) == EINVAL and call(n_max=-1) == EINVAL
    assert call(n_clouds=0) == EINVAL and call(point_stride=2) == EINVAL and call(overlap=2) == EINVAL
    assert call(box_class=p) == EINVAL and call(point_class=p) == EINVAL  # the gate needs both tables
    assert call(pcl=None) == EINVAL and call(flow=None) == EINVAL and call(cloud_of=None) == EINVAL and call(odom=None) == EINVAL
    assert call(pose=None) == EINVAL and call(workspace=None) == EINVAL and call(ws_bytes=16) == EINVAL
    assert call(workspace=ctypes.c_void_p(base + 4096 + 8)) == EINVAL  # alignment
    assert lib.liso_flow_labels_f32(None, p, None, p, p, p, p, p, p, p, p, None, None, q, None, None, None, ws, 1 << 15, None) == EINVAL

    def rc(batch=1, n=10, stride=3, pcl=p, thr=-0.005, ncol=2000, rows=q, cols=q):
        return lib.liso_kitti_rows_cols_f32(batch, n, stride, pcl, None, thr, 0, ncol, rows, cols, None)

    assert rc(batch=0) == EINVAL and rc(n=-1) == EINVAL and rc(stride=2) == EINVAL and rc(pcl=None) == EINVAL and rc(ncol=0) == EINVAL
    assert rc(thr=float("nan")) == EINVAL and rc(rows=None, cols=None) == EINVAL and rc(n=0, pcl=None) == 0


def test_device_entries_refuse_cpu_tensors_and_bad_tables():
    L = _lib()
    pcl = torch.zeros(4, 3)
    with pytest.raises(L.LisoHipError):
        R.find_jumps(pcl)
    with pytest.raises(L.LisoHipError):
        F.get_points_in_box_mask(torch.zeros(4, 4), torch.eye(4, dtype=torch.float64), torch.ones(3, dtype=torch.float64))
    with pytest.raises(ValueError):
        run_host(*two_box_scene(), [True, True], [1, 2], F.LAST, gate=None, box_class=np.zeros((1, 2), np.int32))


def test_reference_names_through_install_as():
    import importlib

    import liso_amd

    liso_amd.install_as("liso")
    kitti = importlib.import_module("liso.datasets.kitti.create_kitti_tracking")
    assert kitti.extract_lidar_flow_ta_tb is F.extract_lidar_flow_ta_tb and kitti.get_points_in_box_mask is F.get_points_in_box_mask
    assert importlib.import_module("liso.datasets.argoverse2.create").update_dynamic_flow is F.update_dynamic_flow
    helper = importlib.import_module("liso.datasets.kitti.kitti_range_image_projection_helper")
    assert helper.find_jumps is R.find_jumps and helper.find_cols is R.find_cols
    assert helper.kitti_pcl_projection_get_rows_cols is R.kitti_pcl_projection_get_rows_cols
    assert importlib.import_module("liso.datasets.torch_dataset_commons").add_lidar_rows_to_kitti_sample is R.add_lidar_rows_to_kitti_sample
