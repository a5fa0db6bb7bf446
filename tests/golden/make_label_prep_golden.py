"""Generates tests/golden/label_prep_reference.npz from the reference's own python, called UNBOUND on a plain attribute holder:
  liso.datasets.torch_dataset_commons.LidarDataset.filter_objects_to_bev_non_empty            (:1013-1059)
  ... .object_is_in_bev_range, get_points_in_boxes_mask(use_double_precision=False)           (:1228-1231, :1902-1935)
  ... .get_object_velocity_in_obj_coords                                                      (:1116-1145)
  ... .create_true_where_ignore_region_mask                                                   (:919-941)
  liso.datasets.torch_dataset_commons.draw_heat_regression_maps                               (:190-339)
Absent third-party modules are stubbed with empty modules (no arithmetic).  Every case stores its inputs and the outputs.

The generator asserts the conditions under which the tests may demand exact agreement, and fails loudly otherwise:
  * every contained-point decision keeps >= 1e-3 m from the box face (the fp32 four-term product at coordinates within 100 m is
    uncertain by less than 4 * 2^-23 * sum |terms| < 1e-4 m, whatever the summation order);
  * every range decision keeps >= 1e-3 m from 50 m; every box that is not placed exactly on the BEV edge keeps >= 1e-3 m from it;
  * every ignore-mask cell centre keeps >= 1e-9 m from a box edge;
  * no heat value lies within 1e-6 of 0.01;
  * no two scaled heats tie for the maximum of a cell -- a relative gap under 1e-9 counts as a tie -- where one of them occupies
    it, except in the deliberate overlap pair; those cells are listed per map (`*_ties`, at most 2 per map) and the tests skip them.
Run in the build container only:
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_label_prep_golden.py
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

K, N, RANGE = 12, 4096, 100.0
INVALID_SLOT, TIE_A, TIE_B = 8, 6, 7
MAX_TIES = 2


def box_cfg(dims="predict_abs_size", rot="vector", act="softplus"):
    return cfg({"dimensions_representation": {"method": dims}, "rotation_representation": {"method": rot},
                "position_representation": {"method": "local_relative_offset"}, "activations": {"dims": act}})


VARIANTS = {  # tag: (box_pred_cfg, scaled, normalize_gaussian)
    "vec": (box_cfg(), True, False),
    "norm": (box_cfg(), False, True),
    "log_direct": (box_cfg("predict_log_size", "direct", "exp"), True, False),
    "bins": (box_cfg(rot="class_bins"), False, False),
}


def make_boxes(g, grid):
    """12 fp64 boxes: many / one / no contained point, outside the BEV, beyond 50 m, exactly on the BEV edge, an overlapping pair
    placed symmetrically about a cell centre with equal shape (the deliberate tie), an invalid slot"""
    cell = RANGE / grid
    c0 = np.array([-0.5 * RANGE + 20.5 * cell, -0.5 * RANGE + 40.5 * cell])  # the centre of cell (20, 40)
    pos = np.array([[10.3, 5.2, -0.9], [-12.7, 20.1, -1.0], [25.4, -30.2, -0.8], [61.5, 4.4, -1.0], [40.2, 35.1, -0.7],
                    [50.0, 10.6, -0.9], [c0[0] - 1.25, c0[1] - 0.5, -1.0], [c0[0] + 1.25, c0[1] + 0.5, -1.0], [-30.3, -8.8, -1.1],
                    [-5.6, -17.3, -0.6], [18.9, 33.3, -1.2], [-41.2, 12.9, -0.8]])
    dims = np.stack([g.uniform(3.5, 5.0, K), g.uniform(1.6, 2.2, K), g.uniform(1.4, 1.9, K)], -1)
    rot = g.uniform(-np.pi, np.pi, (K, 1))
    dims[TIE_B], rot[TIE_B] = dims[TIE_A], rot[TIE_A]
    rot[5] = 0.3
    velo = g.uniform(-8.0, 8.0, (K, 1))
    valid = np.ones(K, bool)
    valid[INVALID_SLOT] = False
    return pos, dims, rot, velo, valid


def box_frame(pos, rot, pts):
    """fp64 coordinates of pts [N,3] in the frames of the boxes -> [N,K,3]"""
    c, s = np.cos(rot[:, 0]), np.sin(rot[:, 0])
    d = pts[:, None, :] - pos[None]
    return np.stack([d[..., 0] * c + d[..., 1] * s, d[..., 1] * c - d[..., 0] * s, d[..., 2]], -1)


def make_cloud(g, pos, dims, rot):
    """fp32 [N,3]: a uniform background with the boxes 2 and 10 emptied, box 1 given exactly one point, the others many"""
    p = np.concatenate([g.uniform(-62.0, 62.0, (N, 2)), g.uniform(-3.0, 2.0, (N, 1))], -1)
    inside = (np.abs(box_frame(pos, rot, p)) < 0.5 * dims[None] + 0.05).all(-1)
    p[inside[:, [1, 2, 10]].any(-1), 2] = 30.0  # lifted out of the three boxes (and out of every other one)
    row = 0
    for k in range(K):
        n = {1: 1, 2: 0, 10: 0}.get(k, 40)
        local = g.uniform(-0.45, 0.45, (n, 3)) * dims[k]
        c, s = np.cos(rot[k, 0]), np.sin(rot[k, 0])
        p[row:row + n] = np.stack([pos[k, 0] + c * local[:, 0] - s * local[:, 1], pos[k, 1] + s * local[:, 0] + c * local[:, 1],
                                   pos[k, 2] + local[:, 2]], -1)
        row += n
    p = p[g.permutation(N)].astype(np.float32)
    f = np.abs(box_frame(pos, rot, p.astype(np.float64))) - 0.5 * dims[None]  # signed distance to the faces, per axis
    is_in = (f < 0).all(-1)
    margin = np.where(is_in, (-f).min(-1), np.where(f > 0, f, 0.0).max(-1))
    assert margin.min() >= 1e-3, f"a contained-point decision is {margin.min():.2e} m from a box face"
    counts = is_in.sum(0)
    assert counts[1] == 1 and counts[2] == 0 and counts[10] == 0 and (np.delete(counts, [1, 2, 10]) >= 30).all(), counts
    return p, is_in.any(0)


def shape_arrays(prefix, s, out):
    for a in ("pos", "dims", "rot", "velo", "probs", "valid"):
        out[f"{prefix}_{a}"] = np.asarray(getattr(s, a))


def main():
    def _imp():
        import liso.datasets.torch_dataset_commons as tdc
        from liso.kabsch.kabsch_mask import batched_render_gaussian_kabsch_mask
        from liso.kabsch.shape_utils import Shape
        from liso.transformations.transformations import compose_matrix
        from liso.utils.bev_utils import get_metric_voxel_center_coords
        from liso.utils.torch_transformation import homogenize_pcl
        return tdc, batched_render_gaussian_kabsch_mask, Shape, compose_matrix, homogenize_pcl, get_metric_voxel_center_coords

    tdc, render_gauss, Shape, compose_matrix, homogenize_pcl, cell_centers = import_with_stubs(_imp)
    LD = tdc.LidarDataset
    out = {"variants": np.array(list(VARIANTS)), "scenes": np.array(["g64", "g128"])}

    for tag, grid, seed, variants in (("g64", 64, 11, list(VARIANTS)), ("g128", 128, 12, ["vec", "norm"])):
        g = np.random.default_rng(seed)
        self = types.SimpleNamespace(bev_range_m_np=np.array([RANGE, RANGE], np.float32), centermaps_output_grid_size=np.array([grid, grid]))
        self.object_is_in_bev_range = types.MethodType(LD.object_is_in_bev_range, self)
        pos, dims, rot, velo, valid = make_boxes(g, grid)
        pcl, has_want = make_cloud(g, pos, dims, rot)
        boxes = Shape(pos=pos, dims=dims, rot=rot, probs=np.ones((K, 1)), velo=velo, valid=valid)
        scale = g.uniform(0.5, 1.0, (K, 1))
        scale[TIE_B] = scale[TIE_A]
        out[f"{tag}_grid_range"] = np.array([grid, RANGE])
        out[f"{tag}_pcl"], out[f"{tag}_scale"] = pcl, scale
        shape_arrays(f"{tag}_in", boxes, out)
        norm = np.linalg.norm(pos, axis=-1)
        assert (np.abs(norm - 50.0) >= 1e-3).all(), "a box is too close to the 50 m range"
        edge = np.abs(np.abs(pos[:, :2]) - 0.5 * RANGE)
        assert ((edge >= 1e-3) | (edge == 0.0)).all() and (edge == 0.0).sum() == 1, "BEV edge: one box exactly on it, the others clear"

        homog = homogenize_pcl(pcl)
        nusc, has = LD.filter_objects_to_bev_non_empty(self, copy.deepcopy(boxes), homog, filter_range_m=50.0, filter_bev=False)
        bev, _ = LD.filter_objects_to_bev_non_empty(self, copy.deepcopy(boxes), homog, box_has_points_inside=has)
        assert np.array_equal(has, has_want)
        shape_arrays(f"{tag}_nusc", nusc, out)
        shape_arrays(f"{tag}_bev", bev, out)
        out[f"{tag}_has_points"] = has
        print(tag, "has points", has.astype(int), "nusc", nusc.valid.sum(), "bev", bev.valid.sum())
        assert 0 < nusc.valid.sum() < bev.valid.sum() < valid.sum(), "the two filters must keep different, non-empty sets"

        # ---- target maps of every valid box (as the mined boxes are drawn: unfiltered, some outside the BEV) -------------------
        drawn = boxes.drop_padding_boxes()
        drawn_scale = scale[valid]
        for v in variants:
            bcfg, scaled, normalize = VARIANTS[v]
            sc = drawn_scale if scaled else None
            maps = tdc.draw_heat_regression_maps(copy.deepcopy(drawn), np.array([grid, grid]), np.array([RANGE, RANGE], np.float32), bcfg,
                                                 per_obj_prob_scale=sc, normalize_gaussian=normalize)
            heat = render_gauss(box_x=drawn.pos[None, :, 0], box_y=drawn.pos[None, :, 1], box_len=drawn.dims[None, :, 0],
                                box_w=drawn.dims[None, :, 1], box_theta=drawn.rot[None, :, 0], bev_range_x=np.float32(RANGE),
                                bev_range_y=np.float32(RANGE), img_shape=np.array([grid, grid]), normalize_gaussian=normalize)[0]
            assert np.abs(heat - 0.01).min() >= 1e-6, f"{tag}/{v}: a heat value is {np.abs(heat - 0.01).min():.2e} from the threshold"
            scaled_heat = heat if sc is None else sc[:, :, None] * heat
            order = np.argsort(scaled_heat, axis=0)
            top, second = np.take_along_axis(scaled_heat, order[-1:], 0)[0], np.take_along_axis(scaled_heat, order[-2:-1], 0)[0]
            occupied = (np.take_along_axis(heat, order[-1:], 0)[0] > 0.01) | (np.take_along_axis(heat, order[-2:-1], 0)[0] > 0.01)
            ties = np.argwhere(occupied & (top - second <= 1e-9 * top))
            pair = {TIE_A - (TIE_A > INVALID_SLOT), TIE_B - (TIE_B > INVALID_SLOT)}
            for i, j in ties:
                assert {int(order[-1, i, j]), int(order[-2, i, j])} == pair, f"{tag}/{v}: an unplanned tie in cell {(i, j)}"
            assert 1 <= len(ties) <= MAX_TIES, f"{tag}/{v}: {len(ties)} tying cells"
            out[f"{tag}_{v}_ties"] = ties.astype(np.int32).reshape(-1, 2)
            for k, m in maps.items():
                out[f"{tag}_{v}_{k}"] = m
            print(tag, v, "ties", ties.tolist(), "occupied cells", int((maps["pos"] != 0).any(-1).sum()))

        # ---- the maps the reference trains on: gt.boxes with the confidence scale --------------------------------------------
        gt_scale = g.uniform(0.5, 1.0, (int(bev.valid.sum()), 1))
        maps = tdc.draw_heat_regression_maps(copy.deepcopy(bev), np.array([grid, grid]), np.array([RANGE, RANGE], np.float32), box_cfg(),
                                             per_obj_prob_scale=gt_scale)
        out[f"{tag}_gt_scale"] = gt_scale
        for k, m in maps.items():
            out[f"{tag}_gt_{k}"] = m

        # ---- ignore regions: axis-aligned, rotated, straddling the grid edge, small --------------------------------------------
        ig = Shape(pos=np.array([[-20.3, 14.2, 0.0], [12.8, -33.1, 0.0], [48.3, -20.4, 0.0], [3.1, 2.7, 0.0]]),
                   dims=np.array([[7.3, 4.9, 2.0], [11.7, 6.1, 2.0], [10.3, 6.7, 2.0], [2.9, 2.3, 2.0]]),
                   rot=np.array([[0.0], [0.7], [-0.4], [2.1]]), probs=np.ones((4, 1)))
        c, s = np.cos(ig.rot[:, 0]), np.sin(ig.rot[:, 0])
        centers = cell_centers(np.float32(RANGE), np.float32(RANGE), np.array([grid, grid]))[..., :2]
        d = centers[:, :, None, :] - ig.pos[None, None, :, :2]
        u, w = d[..., 0] * c + d[..., 1] * s, d[..., 1] * c - d[..., 0] * s
        gap = min(np.abs(np.abs(u) - 0.5 * ig.dims[:, 0]).min(), np.abs(np.abs(w) - 0.5 * ig.dims[:, 1]).min())
        assert gap >= 1e-9, f"{tag}: a cell centre is {gap:.2e} m from an ignore-box edge"
        mask = LD.create_true_where_ignore_region_mask(self, ig)
        assert mask.dtype == bool and mask.any() and mask[-1].any(), "the edge box must reach the last row"
        shape_arrays(f"{tag}_ignore", ig, out)
        out[f"{tag}_ignore_mask"] = mask

    # ---- a sample without a valid box -------------------------------------------------------------------------------------------
    g = np.random.default_rng(13)
    pos, dims, rot, velo, _ = make_boxes(g, 64)
    empty = Shape(pos=pos, dims=dims, rot=rot, probs=np.ones((K, 1)), velo=velo, valid=np.zeros(K, bool))
    for v in ("vec", "bins"):
        maps = tdc.draw_heat_regression_maps(copy.deepcopy(empty), np.array([64, 64]), np.array([RANGE, RANGE], np.float32), VARIANTS[v][0])
        for k, m in maps.items():
            out[f"empty_{v}_{k}"] = m

    # ---- object velocities ------------------------------------------------------------------------------------------------------
    g = np.random.default_rng(14)
    odom = compose_matrix(angles=[0.0, 0.0, 0.03], translate=[1.2, -0.05, 0.0])
    ta = np.stack([compose_matrix(angles=[0.0, 0.0, g.uniform(-np.pi, np.pi)], translate=[g.uniform(-90, 90), g.uniform(-90, 90), g.uniform(-2, 1)])
                   for _ in range(K)])
    tb = np.stack([compose_matrix(angles=[0.0, 0.0, g.uniform(-0.1, 0.1)], translate=[g.uniform(-2, 2), g.uniform(-0.3, 0.3), 0.0]) @ t
                   for t in ta])
    out["velo_odom"], out["velo_pose_ta"], out["velo_pose_tb"] = odom, ta, tb
    out["velo_out"] = LD.get_object_velocity_in_obj_coords(None, odom, ta, tb)
    assert out["velo_out"].shape == (K, 3) and out["velo_out"].dtype == np.float64

    path = os.path.join(HERE, "label_prep_reference.npz")
    np.savez_compressed(path, **out)
    print("wrote", len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
