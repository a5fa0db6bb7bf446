"""Generates tests/golden/sample_prep_reference.npz from the reference's own python, called UNBOUND on a plain attribute holder:
  liso.datasets.torch_dataset_commons.LidarDataset.augment_sample_content                    (:1291-1433)
  ... .augment_objects_from_category_with_trafo, .transform_pcl_maybe_with_intensity           (:1435-1483)
  ... .pillarize_bev, .voxelize_sample, .add_bev_flow, .add_bev_ground_height_occupancy_maps   (:1147-1223, :975-987)
  liso.datasets.torch_dataset_commons.get_augmentation_transform                             (:1870-1899)
and the moving_mask expression of assemble_sample_data (:776-792), copied as it stands.  Absent third-party modules are stubbed
with empty modules (no arithmetic).  Every case stores its inputs, its seeds and the outputs.  The generator asserts what the tests
rely on: every moving_mask decision has a margin of at least 1e-6 of its threshold, and no transformed point of the chained case
lies within 1e-9 cells of a pillar boundary.  Run in the build container only:
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_sample_prep_golden.py
"""
import copy
import os
import sys
import types

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, "/root/reference")

from make_targets_golden import cfg, import_with_stubs  # noqa: E402

THRESHOLD_MPS, DT = 0.5, 0.1


def holder(LD, grid, rng, height=None):
    self = types.SimpleNamespace()
    self.bev_range_m_np = np.array(rng, np.float32)
    self.img_grid_size_np = np.array(grid, np.int32)
    self.height_range_m_np = np.array(height if height is not None else [-np.inf, np.inf], np.float32)
    self.for_tracking = False
    for name in ("pillarize_bev", "voxelize_sample", "add_bev_flow", "add_bev_ground_height_occupancy_maps",
                 "transform_pcl_maybe_with_intensity", "augment_objects_from_category_with_trafo"):
        setattr(self, name, types.MethodType(getattr(LD, name), self))
    self.get_sample_data_downsample_keys = LD.get_sample_data_downsample_keys
    return self


def make_cloud(g, n, stride, rng, dense_cell=0, nan_rows=0, edges=True):
    half = 0.5 * np.array(rng)
    xy = g.uniform(-1.08, 1.08, (n, 2)) * half  # some outside the range
    z = g.uniform(-3.0, 2.0, (n, 1))
    p = np.concatenate([xy, z] + [g.uniform(0, 1, (n, 1)) for _ in range(stride - 3)], -1).astype(np.float32)
    k = 0
    if edges and n >= 40:
        cell = np.array(rng) / 64.0
        # both BEV edges, exactly and next to them, and the (-1, 0) coordinate band below the negative edge
        p[0, :2] = [-half[0], 0.3]
        p[1, :2] = [half[0], 0.3]
        p[2, :2] = [0.3, -half[1]]
        p[3, :2] = [0.3, half[1]]
        p[4, :2] = [np.nextafter(np.float32(half[0]), np.float32(0)), np.nextafter(np.float32(half[1]), np.float32(0))]
        for i in range(5, 15):
            p[i, 0] = -half[0] - g.uniform(0.05, 0.95) * cell[0] * 0.2
            p[i + 10, 1] = -half[1] - g.uniform(0.05, 0.95) * cell[1] * 0.2
        k = 25
    if dense_cell:
        p[k:k + dense_cell, :2] = np.array([3.3, -4.4]) + g.uniform(0.0, 0.05, (dense_cell, 2))
        k += dense_cell
    if nan_rows:
        at = g.choice(np.arange(k, n), nan_rows, replace=False)
        p[at[: nan_rows // 2]] = np.nan
        p[at[nan_rows // 2:], g.integers(0, 3)] = np.nan
    return p


def reference_moving_mask(pcl, flow, odom_tb_ta, homogenize_pcl):
    pcl_homog = homogenize_pcl(pcl[:, :3])
    norm = np.linalg.norm(np.einsum("ij,kj->ki", odom_tb_ta - np.eye(4), pcl_homog)[..., 0:3] - flow, axis=-1)
    thr = THRESHOLD_MPS * DT
    assert (np.abs(norm - thr) >= 1e-6 * thr).all(), "a moving_mask decision is too close to its threshold"
    return norm > thr


def small_odom(g, compose_matrix):
    return compose_matrix(angles=[0.0, 0.0, g.uniform(-0.05, 0.05)], translate=[g.uniform(0.5, 1.5), g.uniform(-0.1, 0.1), 0.0])


def main():
    def _imp():
        import liso.datasets.torch_dataset_commons as tdc
        from liso.kabsch.shape_utils import Shape
        from liso.transformations.transformations import compose_matrix
        from liso.utils.torch_transformation import homogenize_pcl
        return tdc, Shape, compose_matrix, homogenize_pcl

    tdc, Shape, compose_matrix, homogenize_pcl = import_with_stubs(_imp)
    LD = tdc.LidarDataset
    out = {}

    # ---- get_augmentation_transform under recorded seeds ----------------------------------------------------------------------
    draws = [(101, 90.0, 5.0, None), (102, 90.0, 0.0, None), (103, 0.0, 5.0, None), (104, 45.0, 2.0, 0.1), (105, 90.0, 5.0, 0.05)]
    out["aug_args"] = np.array([[s, r, o, np.nan if d is None else d] for s, r, o, d in draws])
    mats = []
    for s, r, o, d in draws:
        np.random.seed(s)
        mats.append(tdc.get_augmentation_transform(r, o, d))
    out["aug_T"] = np.stack(mats)

    # ---- transforms: rotations 0, +90, -90, generic; with / without offset; one with xy scale; strides 3, 4, 5 -----------------
    fixed = {"rot0": (0.0, [0, 0, 0], None), "rot0_off": (0.0, [1.5, -2.25, 0], None), "p90": (90.0, [0, 0, 0], None),
             "m90_off": (-90.0, [-3.0, 0.7, 0], None), "gen": (33.3, [0, 0, 0], None), "gen_off": (-71.9, [4.1, 2.2, 0], None),
             "gen_scale": (12.5, [0.4, -4.4, 0], [1.07, 1.07, 1.0])}
    g = np.random.default_rng(7)
    self = holder(LD, (64, 64), (40.0, 40.0))
    for i, (tag, (deg, tr, sc)) in enumerate(fixed.items()):
        T = compose_matrix(angles=[0.0, 0.0, np.deg2rad(deg)], translate=tr, scale=sc)
        stride = 3 + i % 3
        pcl = make_cloud(g, 400, stride, (40.0, 40.0), edges=False)
        flow = g.normal(size=(400, 3)).astype(np.float32)
        res3 = self.transform_pcl_maybe_with_intensity(pcl[:, :4] if stride == 4 else pcl[:, :3], T)
        out[f"tf_{tag}_T"], out[f"tf_{tag}_pcl"], out[f"tf_{tag}_flow"] = T, pcl, flow
        out[f"tf_{tag}_out_pcl"] = np.concatenate([res3[:, :3], pcl[:, 3:]], -1)
        out[f"tf_{tag}_out_flow"] = np.einsum("ij,nj->ni", T, tdc.homogenize_flow(flow))[..., 0:3].astype(np.float32)
    out["tf_tags"] = np.array(list(fixed))

    # ---- augment_sample_content on a dictionary -------------------------------------------------------------------------------
    for tag, dataset, seed in (("aw", "waymo", 21), ("ak", "kitti_object", 22)):
        g = np.random.default_rng(seed)
        c = cfg({"data": {"augmentation": {"rotation": {"max_rot_deg": 90.0}, "translation": {"max_sensor_pos_offset_m": 5.0}},
                          "odom_source": "kiss_icp", "flow_source": "slim_flow"}})
        self = holder(LD, (64, 64), (40.0, 40.0))
        self.cfg = c
        n0, n1, K = 400, 500, 9

        def boxes(k, dtype):
            s = Shape(pos=g.uniform(-15, 15, (k, 3)).astype(dtype), dims=g.uniform(1, 4, (k, 3)).astype(dtype),
                      rot=g.uniform(-np.pi, np.pi, (k, 1)).astype(dtype), probs=np.ones((k, 1), dtype))
            s.valid = g.uniform(size=k) > 0.3
            return s

        sample = {
            "pcl_t0": make_cloud(g, n0, 4, (40.0, 40.0), edges=False), "pcl_t1": make_cloud(g, n1, 4, (40.0, 40.0), edges=False),
            "pcl_tx": make_cloud(g, 300, 4, (40.0, 40.0), edges=False),
            "gt": {"flow_t0_t1": g.normal(size=(n0, 3)).astype(np.float32), "flow_t1_t0": g.normal(size=(n1, 3)).astype(np.float32),
                   "odom_t0_t1": small_odom(g, compose_matrix), "odom_t0_tx": small_odom(g, compose_matrix),
                   "objects_t0": boxes(K, np.float64), "objects_t1": boxes(K - 2, np.float32)},
            "kiss_icp": {"odom_t0_t1": small_odom(g, compose_matrix)},
            "slim_flow": {"flow_t0_t1": g.normal(size=(n0, 3)).astype(np.float32)},
            "mined": {"boxes_t0": boxes(5, np.float32)},
        }
        if dataset == "kitti_object":
            sample["gt"]["kitti_ignore_region_boxes_t0"] = boxes(4, np.float64)
            sample["gt"]["objects_t0"] = {"poses": sample["gt"]["objects_t0"].get_poses()}
            sample["gt"].pop("objects_t1")

        def dump(prefix, d):
            for k, v in d.items():
                if isinstance(v, dict):
                    dump(f"{prefix}{k}/", v)
                elif isinstance(v, Shape):
                    for a in ("pos", "rot", "dims", "valid"):
                        out[f"{prefix}{k}/{a}"] = np.asarray(getattr(v, a))
                else:
                    out[f"{prefix}{k}"] = np.asarray(v)

        dump(f"{tag}_in/", sample)
        res = copy.deepcopy(sample)
        np.random.seed(seed)
        LD.augment_sample_content(self, res, "t0", "t1", dataset)
        np.random.seed(seed)
        out[f"{tag}_T"] = tdc.get_augmentation_transform(90.0, 5.0, None)
        out[f"{tag}_seed"] = np.array(seed)
        dump(f"{tag}_out/", res)

    # ---- crop, maps, moving mask ----------------------------------------------------------------------------------------------
    crops = {
        # tag: (grid, range, height, n, stride, dense, nan rows, seed)
        "ca": ((64, 64), (40.0, 40.0), None, 2300, 4, 1000, 12, 31),
        "cb": ((64, 64), (40.0, 40.0), None, 1300, 4, 0, 5, 32),
        "ch": ((48, 80), (30.0, 50.0), (-1.5, 0.75), 1500, 3, 0, 0, 33),
        "c5": ((32, 32), (60.0, 60.0), None, 700, 5, 0, 3, 34),
        "c0": ((64, 64), (40.0, 40.0), None, 0, 4, 0, 0, 35),
        "c1": ((64, 64), (40.0, 40.0), None, 1, 4, 0, 0, 36),
    }
    for tag, (grid, rng, height, n, stride, dense, nans, seed) in crops.items():
        g = np.random.default_rng(seed)
        self = holder(LD, grid, rng, height)
        pcl = make_cloud(g, n, stride, rng, dense, nans)
        if n == 1:
            pcl[0, :3] = [1.0, -2.0, 0.5]
        flow = (g.normal(size=(n, 3)) * g.choice([0.01, 1.0, 20.0], (n, 1))).astype(np.float32)
        rows = g.integers(0, 64, n).astype(np.int32)
        is_ground = g.uniform(size=n) < 0.3
        odom_t1_t0 = np.linalg.inv(small_odom(g, compose_matrix))
        out[f"{tag}_meta"] = np.array(list(grid) + list(rng) + list(self.height_range_m_np.astype(np.float64)) + [stride, seed], np.float64)
        out[f"{tag}_pcl"], out[f"{tag}_flow"], out[f"{tag}_rows"], out[f"{tag}_is_ground"] = pcl, flow, rows, is_ground
        out[f"{tag}_odom_t1_t0"] = odom_t1_t0
        coors_all, in_range = self.voxelize_sample(pcl)
        out[f"{tag}_coors_all"], out[f"{tag}_in_range"] = coors_all.astype(np.int32), in_range
        sample = {"pcl_t0": pcl.copy(), "lidar_rows_t0": rows.copy(), "gt": {"flow_t0_t1": flow.copy(), "is_ground_t0": is_ground.copy()}}
        with np.errstate(invalid="ignore"):
            sample = self.pillarize_bev(sample, "t0", "t1")

        def record(prefix, s):
            out[f"{prefix}_pcl"], out[f"{prefix}_coors"] = s["pcl_t0"], s["pillar_coors_t0"].astype(np.int32)
            out[f"{prefix}_rows"], out[f"{prefix}_flow"] = s["lidar_rows_t0"], s["gt"]["flow_t0_t1"]
            out[f"{prefix}_is_ground"] = s["gt"]["is_ground_t0"]
            self.add_bev_ground_height_occupancy_maps(s, "t0")
            out[f"{prefix}_occupancy"] = s["occupancy_f32_t0"]
            view = {"pcl_t0": {"pillar_coors": s["pillar_coors_t0"]}, "gt": {"flow_t0_t1": s["gt"]["flow_t0_t1"]}}
            self.add_bev_flow(view, "gt", "t0", "t1")
            out[f"{prefix}_flow_bev"] = view["gt"]["flow_bev_t0_t1"]
            out[f"{prefix}_moving"] = reference_moving_mask(s["pcl_t0"], s["gt"]["flow_t0_t1"], odom_t1_t0, homogenize_pcl)

        record(f"{tag}_crop", copy.deepcopy(sample))
        # crop, then the ground removal of :1165-1185 with the recorded label
        removed = tdc.downsample_dict(copy.deepcopy(sample), ~sample["gt"]["is_ground_t0"], self.get_sample_data_downsample_keys("t0", "t1"))
        record(f"{tag}_removed", removed)
        print(tag, pcl.shape, "kept", sample["pcl_t0"].shape[0], "after removal", removed["pcl_t0"].shape[0])
    out["crop_tags"] = np.array(list(crops))

    # ---- the chained case: two samples, transform -> crop -> maps -------------------------------------------------------------
    grid, rng = (64, 64), (40.0, 40.0)
    self = holder(LD, grid, rng)
    for s, seed in enumerate((41, 42)):
        g = np.random.default_rng(seed)
        n = 1500
        ring = g.integers(0, 32, n)
        az = g.uniform(-np.pi, np.pi, n)
        elev = np.deg2rad(-24.0 + ring * 0.8)
        r = np.minimum(g.uniform(4.0, 30.0, n), np.where(elev < -0.02, 1.73 / np.maximum(np.tan(-elev), 1e-3), 1e9))
        pcl = np.stack([r * np.cos(az), r * np.sin(az), r * np.tan(elev), g.uniform(0, 1, n)], -1).astype(np.float32)
        flow = g.normal(size=(n, 3)).astype(np.float32)
        np.random.seed(seed)
        T = tdc.get_augmentation_transform(90.0, 5.0, None)
        tp = self.transform_pcl_maybe_with_intensity(pcl, T)
        tf = np.einsum("ij,nj->ni", T, tdc.homogenize_flow(flow))[..., 0:3].astype(np.float32)
        cells = (tp[:, :2].astype(np.float64) + 0.5 * np.array(rng)) / np.array(rng) * np.array(grid)
        assert (np.abs(cells - np.rint(cells)) > 1e-9).all(), "a transformed point lies on a pillar boundary"
        sample = self.pillarize_bev({"pcl_t0": tp, "gt": {"flow_t0_t1": tf}}, "t0", "t1")
        self.add_bev_ground_height_occupancy_maps(sample, "t0")
        view = {"pcl_t0": {"pillar_coors": sample["pillar_coors_t0"]}, "gt": {"flow_t0_t1": sample["gt"]["flow_t0_t1"]}}
        self.add_bev_flow(view, "gt", "t0", "t1")
        out[f"chain{s}_pcl"], out[f"chain{s}_flow"], out[f"chain{s}_T"], out[f"chain{s}_seed"] = pcl, flow, T, np.array(seed)
        out[f"chain{s}_out_pcl"], out[f"chain{s}_out_coors"] = sample["pcl_t0"], sample["pillar_coors_t0"].astype(np.int32)
        out[f"chain{s}_out_flow"], out[f"chain{s}_out_occupancy"] = sample["gt"]["flow_t0_t1"], sample["occupancy_f32_t0"]
        out[f"chain{s}_out_flow_bev"] = view["gt"]["flow_bev_t0_t1"]
    out["chain_meta"] = np.array(list(grid) + list(rng), np.float64)
    np.savez_compressed(os.path.join(HERE, "sample_prep_reference.npz"), **out)
    print("wrote", len(out), "arrays,", os.path.getsize(os.path.join(HERE, "sample_prep_reference.npz")), "bytes")


if __name__ == "__main__":
    main()
