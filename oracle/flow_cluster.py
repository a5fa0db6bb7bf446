"""TEST INFRASTRUCTURE ONLY: torch-CPU restatement of rows D1 and D3.  Pinned by
tests/golden/flow_cluster_reference.npz generated from the reference's own python
(tests/golden/make_flow_cluster_golden.py)."""
import torch


def scatter_mean_2d(valid, batch_idx, rows, cols, values, B, H, W):
    """liso/utils/torch_differentiable_forward_scatter.py:22-87: scatter_add of values + counts, divide where count > 1"""
    C = values.shape[-1]
    v = values[valid].double()
    lin = ((batch_idx[valid] * H + rows[valid].long()) * W + cols[valid].long())
    tgt = torch.zeros(B * H * W, C, dtype=torch.float64)
    tgt.index_add_(0, lin, v)
    cnt = torch.zeros(B * H * W, dtype=torch.int64)
    cnt.index_add_(0, lin, torch.ones_like(lin))
    out = torch.where(cnt[:, None] > 1, tgt / cnt[:, None].clamp(min=1), tgt)
    return out.float().view(B, H, W, C)


def bev_dynamic_flow(pcl_is_valid, pcl, pillar_coors, point_flow, odom_ta_tb, target_shape):
    """liso/utils/bev_flow_utils.py:6-77 -> (dynamicness[B,H,W,1], nonrigid_flow[B,H,W,3])"""
    homog = torch.cat([pcl[..., :3], torch.ones_like(pcl[..., :1])], -1)
    homog = torch.where(pcl_is_valid[..., None], homog, torch.zeros(()))
    flow = torch.where(pcl_is_valid[..., None], point_flow, torch.zeros(()))
    M = torch.linalg.inv(odom_ta_tb.double()) - torch.eye(4, dtype=torch.float64)[None]
    stat = torch.einsum("bij,bnj->bni", M, homog.double())[..., :3].float()
    stat = torch.where(pcl_is_valid[..., None], stat, torch.zeros(()))
    nonrigid = flow - stat
    length = torch.linalg.norm(nonrigid, dim=-1, keepdim=True)
    B, N = pcl_is_valid.shape
    bidx = torch.arange(B)[:, None].repeat(1, N)
    H, W = int(target_shape[0]), int(target_shape[1])
    return (scatter_mean_2d(pcl_is_valid, bidx, pillar_coors[..., 0], pillar_coors[..., 1], length, B, H, W),
            scatter_mean_2d(pcl_is_valid, bidx, pillar_coors[..., 0], pillar_coors[..., 1], nonrigid, B, H, W))


def fit_box_z(pcl, pos, dims, rot, box_height=1000.0):
    """flow_cluster_detector.py:339-384"""
    K = pos.shape[0]
    c, s = torch.cos(rot.double()), torch.sin(rot.double())
    bz = pos[:, 2].double() if pos.shape[-1] == 3 else torch.zeros(K, dtype=torch.float64)
    dx = pcl[:, None, 0].double() - pos[None, :, 0].double()
    dy = pcl[:, None, 1].double() - pos[None, :, 1].double()
    lx, ly = (c * dx + s * dy).float(), (-s * dx + c * dy).float()
    lz = (pcl[:, None, 2].double() - bz[None]).float()
    d = dims if dims.shape[-1] == 3 else torch.cat([dims, box_height * torch.ones_like(dims[:, :1])], -1)
    inside = (lx.abs() < 0.5 * d[None, :, 0]) & (ly.abs() < 0.5 * d[None, :, 1]) & (lz.abs() < 0.5 * d[None, :, 2])
    zmax = torch.where(inside, lz, torch.tensor(-box_height)).max(dim=0).values
    zmin = torch.where(inside, lz, torch.tensor(box_height)).min(dim=0)
    h = torch.clip(zmax - zmin.values, min=1.0, max=2.0)
    return inside.sum(0), pcl[:, 2][zmin.indices] + 0.5 * h, h


# ---- D2: clustering block (flow_cluster_detector.py:151-189) ---------------------------------------------------------
# Both libraries are third-party arithmetic: scikit-learn (pinned 0.24.2 by the reference; 1.7.2 in this
# image -- DBSCAN is deterministic given the point order, the labelling rule has not changed) is CALLED here exactly as
# the reference calls it; scikit-image (pinned 0.19.2) is absent from the image, so regionprops' four properties are
# restated from its published formulas (skimage/measure/_regionprops.py, _moments.py: inertia_tensor,
# inertia_tensor_eigvals, orientation, axis_major_length / axis_minor_length).  Pinned (round 2) by
# tests/golden/regionprops_reference.npz, which scikit-image 0.18.3 itself produced (tests/golden/make_regionprops_golden.py, run
# with the build container's /opt/conda/bin/python3.9): tests/test_regionprops_reference.py; analytic shapes in
# tests/test_oracle_flow_cluster.py.
def dbscan_bev_labels(valid_mask, bev_nonrigid_flow, grid_pts_xy, eps=1.0, min_samples=5, flow_similarity_importance=2.0):
    """one sample: valid_mask [G,G] bool numpy, bev_nonrigid_flow [G,G,3] float32 numpy, grid_pts_xy [G,G,2] float32
    -> label image int64 [G,G] (0 = background / noise), exactly lines :151-172 of the reference"""
    import numpy as np
    from sklearn.cluster import DBSCAN

    bev_labels = np.zeros(valid_mask.shape, dtype=np.int64)
    if np.count_nonzero(valid_mask) <= 1:
        return bev_labels
    dynamic_coors = grid_pts_xy[valid_mask]
    dynamic_flow = flow_similarity_importance * bev_nonrigid_flow[valid_mask]
    cluster_coords = np.concatenate([dynamic_coors, dynamic_flow], axis=-1)
    db = DBSCAN(eps=eps, min_samples=min_samples, metric="euclidean", algorithm="auto", n_jobs=1).fit(cluster_coords)
    labels = np.where(db.labels_ >= 0, db.labels_ + 1, 0)
    rows, cols = np.nonzero(valid_mask)
    bev_labels[rows, cols] = labels
    return bev_labels


def regionprops_restated(label_img):
    """skimage.measure.regionprops(label_img) -> float64 [K,5] rows (centroid_row, centroid_col, orientation,
    axis_major_length, axis_minor_length) for labels 1..K in ascending order (labels without pixels are skipped by
    skimage; DBSCAN labels are dense so none are)."""
    import math

    import numpy as np

    out = []
    for lab in range(1, int(label_img.max()) + 1):
        rr, cc = np.nonzero(label_img == lab)
        if rr.size == 0:
            continue
        r0, c0 = rr.mean(), cc.mean()
        mu00 = float(rr.size)
        mu20 = ((rr - r0) ** 2).sum() / mu00  # second central moment along rows (axis 0)
        mu02 = ((cc - c0) ** 2).sum() / mu00
        mu11 = ((rr - r0) * (cc - c0)).sum() / mu00
        # _moments.inertia_tensor: [[mu02, -mu11], [-mu11, mu20]] / mu00
        a, b, c = mu02, -mu11, mu20
        if a - c == 0:  # _regionprops.orientation
            orientation = -math.pi / 4.0 if b < 0 else math.pi / 4.0
        else:
            orientation = 0.5 * math.atan2(-2 * b, c - a)
        ev = np.clip(np.sort(np.linalg.eigvalsh(np.array([[a, b], [b, c]])))[::-1], 0.0, None)  # inertia_tensor_eigvals
        out.append([r0, c0, orientation, 4.0 * math.sqrt(ev[0]), 4.0 * math.sqrt(ev[1])])
    return np.array(out, dtype=np.float64).reshape(-1, 5)


# ---- the per-box steps between the clusters and the detector targets (include/liso_box_mining.h) ------------------------------
# numpy, fp64, one plain statement per line of the reference; `flow_cluster_detector_forward` below is built from the first
# three, so the end-to-end oracle and the per-kernel oracles of tests/test_gpu_box_mining.py are one text.
UNKNOWN_CLASS_ID = 2**31 - 1             # shape_utils.py:15
INVALID_CLASS_ID = UNKNOWN_CLASS_ID - 1  # shape_utils.py:16


def boxes_from_regions(props, row_coords, col_coords, pix_per_m):
    """flow_cluster_detector.py:176-206.  props fp64 [..., 5] = (centroid_row, centroid_col, orientation, axis_major, axis_minor);
    row_coords fp32 [gx] / col_coords fp32 [gy]: the metric centres of a separable pillar grid (grid_pts_3d[r, c] =
    (row_coords[r], col_coords[c])); pix_per_m fp32 [2].
    -> (center fp32 [..., 2], dims fp64 [..., 2], rot fp64 [...], dims fp32, rot fp32)"""
    import numpy as np

    props = np.asarray(props, np.float64)
    row_coords, col_coords = np.asarray(row_coords, np.float32), np.asarray(col_coords, np.float32)
    # :177-181: astype(int) truncates toward zero; BOTH indices are clipped to the smaller grid extent
    pix = np.clip(props[..., 0:2].astype(np.int64), 0, min(row_coords.shape[0], col_coords.shape[0]) - 1)
    center = np.stack([row_coords[pix[..., 0]], col_coords[pix[..., 1]]], axis=-1)  # :197-199
    dims = props[..., 3:5] * 1.0 / np.asarray(pix_per_m, np.float32).astype(np.float64)  # :191-195 (fp64 / fp32 -> fp64)
    rot = props[..., 2].copy()  # :182-184
    return center, dims, rot, dims.astype(np.float32), rot.astype(np.float32)


def mine_filter_compact(num_labels, center, dims2, rot, num_pts, fit_z, fit_h, *, min_points, aspect_ratio_max, max_box_len_m,
                        min_box_area_m2, min_box_volume_m3, park_invalid=False):
    """flow_cluster_detector.py:221-250 (the five rules), :250 drop_padding_boxes (survivors first, label order kept) and :310
    Shape.from_list_of_shapes(numeric_padding_value=0.0), for fixed K slots per sample.
    num_labels int [B]; center fp32 [B,K,2]; dims2 fp64 [B,K,2]; rot fp64 [B,K]; num_pts int64 [B,K]; fit_z / fit_h fp32 [B,K].
    -> dict of numpy arrays with the shapes and dtypes of liso_mine_filter_compact: pos, dims, rot, probs, velo, valid, class_id,
    difficulty, counts, kabsch_pos, kabsch_dims, kabsch_rot.  The volume is (d0 * d1) * h, the order a left-to-right product takes."""
    import numpy as np

    center, dims2, rot = np.asarray(center, np.float32), np.asarray(dims2, np.float64), np.asarray(rot, np.float64)
    fit_z, fit_h, num_pts = np.asarray(fit_z, np.float32), np.asarray(fit_h, np.float32), np.asarray(num_pts, np.int64)
    B, K = center.shape[:2]
    d0, d1, h = dims2[..., 0], dims2[..., 1], fit_h.astype(np.float64)
    with np.errstate(all="ignore"):
        ok = np.arange(K)[None, :] < np.asarray(num_labels, np.int64).reshape(B, 1)  # regions 1..num_labels exist
        ok &= num_pts >= min_points                                                   # :221
        ok &= d0 / np.maximum(d1, 0.001) <= aspect_ratio_max                          # :222-226
        ok &= d0 <= max_box_len_m                                                     # :227
        ok &= d0 * d1 > min_box_area_m2                                               # :228-230
        ok &= (d0 * d1) * h > min_box_volume_m3                                       # :237-240
    park = np.float32(1e6 if park_invalid else 0.0)
    o = {"pos": np.zeros((B, K, 3), np.float32), "dims": np.zeros((B, K, 3), np.float64), "rot": np.zeros((B, K, 1), np.float64),
         "probs": np.zeros((B, K, 1), np.float64), "velo": np.zeros((B, K, 1), np.float64), "valid": np.zeros((B, K), np.uint8),
         "class_id": np.full((B, K, 1), INVALID_CLASS_ID, np.int32), "difficulty": np.full((B, K, 1), INVALID_CLASS_ID, np.int32),
         "counts": ok.sum(1).astype(np.int32), "kabsch_pos": np.full((B, K, 3), park, np.float32),
         "kabsch_dims": np.zeros((B, K, 3), np.float32), "kabsch_rot": np.zeros((B, K), np.float32)}
    for b in range(B):
        s = np.nonzero(ok[b])[0]
        n = s.size
        o["pos"][b, :n] = np.concatenate([center[b, s], fit_z[b, s, None]], -1)      # :234-236
        o["dims"][b, :n] = np.concatenate([dims2[b, s], h[b, s, None]], -1)          # :231-233
        o["rot"][b, :n, 0] = rot[b, s]
        o["probs"][b, :n] = 1.0                                                      # :202
        o["valid"][b, :n] = 1
        o["class_id"][b, :n] = UNKNOWN_CLASS_ID                                      # shape_utils.py:66
        o["difficulty"][b, :n] = 1                                                   # shape_utils.py:82
        o["kabsch_pos"][b, :n] = o["pos"][b, :n]
        o["kabsch_dims"][b, :n] = o["dims"][b, :n].astype(np.float32)
        o["kabsch_rot"][b, :n] = rot[b, s].astype(np.float32)
    return o


def box_motion(trafos, pos, rot):
    """flow_cluster_detector.py:325-331 with shape_utils.py:563-605 and torch_transformation.py:16-62.
    trafos fp64 [B,S+1,4,4] (slot S = background); pos [B,S,3]; rot fp64 [B,S,1] -> (rot + atan2(t_y, t_x) [B,S,1], |t| [B,S,1]),
    t = the translation of inv(T_box) inv(T_bg) (T_fg T_box), T_box = translation(pos) * yaw(rot); inverses by LU (torch.linalg.inv)"""
    trafos, pos, rot = torch.as_tensor(trafos).double(), torch.as_tensor(pos), torch.as_tensor(rot).double()
    B, S = pos.shape[:2]
    fg, bg = trafos[:, :-1], trafos[:, -1:]
    c, s = torch.cos(rot[..., 0]), torch.sin(rot[..., 0])
    Tb = torch.zeros(B, S, 4, 4, dtype=torch.float64)  # shape_utils.py:271-319: translation * yaw
    Tb[..., 0, 0], Tb[..., 0, 1], Tb[..., 1, 0], Tb[..., 1, 1] = c, -s, s, c
    Tb[..., 0, 3], Tb[..., 1, 3], Tb[..., 2, 3] = pos[..., 0].double(), pos[..., 1].double(), pos[..., 2].double()
    Tb[..., 2, 2] = Tb[..., 3, 3] = 1.0
    M = torch.linalg.inv(Tb) @ torch.linalg.inv(bg) @ (fg @ Tb)  # shape_utils.py:583-605
    tr = M[..., :3, 3]
    return rot + torch.atan2(tr[..., [1]], tr[..., [0]]), torch.linalg.norm(tr, dim=-1)[..., None]


_BOX_KEYS = ("pos", "dims", "rot", "probs", "velo", "valid", "class_id", "difficulty")


def nms_prepare(arrays, pre_nms_max):
    """nms_iou.py:33-44 and :257-268 for fixed slots: per sample, every field permuted into the STABLE descending order of
    key = probs where valid else -inf (a NaN confidence ranks as -inf too, so the order stays a permutation); the first
    `pre_nms_max` (<= 0: all) valid slots enter the NMS.  arrays: dict of numpy [B,K,...] (pos fp32, dims / rot / probs / velo
    fp64, valid uint8, class_id / difficulty int32).
    -> (permuted dict, enters uint8 [B,K], dense fp32 [B,K,7]); a slot that does not enter is parked at (1e6 + 10 rank, 1e6, 0)
    with 1e-3 edges (perform_nms_on_shapes_padded)."""
    import numpy as np

    B, K = arrays["valid"].shape
    out = {k: np.array(arrays[k], copy=True) for k in _BOX_KEYS}
    enters = np.zeros((B, K), np.uint8)
    dense = np.zeros((B, K, 7), np.float32)
    for b in range(B):
        valid = arrays["valid"][b] != 0
        p = np.asarray(arrays["probs"][b], np.float64).reshape(K)
        key = np.where(valid & ~np.isnan(p), p, -np.inf)
        order = np.argsort(-key, kind="stable")
        for k in _BOX_KEYS:
            out[k][b] = arrays[k][b][order]
        rank = np.arange(K)
        enters[b] = valid[order] & ((rank < pre_nms_max) if pre_nms_max > 0 else True)
        dense[b, :, 0] = np.float32(1e6) + np.float32(10.0) * rank.astype(np.float32)
        dense[b, :, 1] = 1e6
        dense[b, :, 3:6] = 1e-3
        e = enters[b] != 0
        dense[b, e] = np.concatenate([out["pos"][b, e], out["dims"][b, e].astype(np.float32),
                                      out["rot"][b, e].reshape(-1, 1).astype(np.float32)], -1)  # :230-242
    return out, enters, dense


def nms_finish(b, arrays, enters, keep, num, max_boxes, targets):
    """nms_iou.py:54-58, :10-20 and :277-282 for sample b of fixed slots: of keep[:num] (num clamped to [0, K], indices outside
    [0, K) ignored) the slots that entered and are valid survive, the first `max_boxes` of them in slot order stay valid; every
    other slot of the sample takes the padding values of Shape.set_padding_val_to(0.0) (shape_utils.py:439-462).
    targets = (t_pos fp32 [B,K,3], t_dims fp32 [B,K,3], t_rot fp32 [B,K], t_valid uint8 [B,K]): sample b is rewritten with the
    fp32 box arrays (dims clamped to >= 1e-3).  -> (dict, targets), copies; the other samples pass through."""
    import numpy as np

    out = {k: np.array(arrays[k], copy=True) for k in _BOX_KEYS}
    t_pos, t_dims, t_rot, t_valid = (np.array(t, copy=True) for t in targets)
    K = out["valid"].shape[1]
    hit = np.zeros(K, bool)
    for j in np.asarray(keep).reshape(-1)[:min(max(int(num), 0), K)]:
        if 0 <= j < K:
            hit[j] = True
    kept = hit & (np.asarray(enters)[b] != 0) & (out["valid"][b] != 0)
    ok = kept & (np.cumsum(kept) <= max_boxes)
    for k in ("pos", "dims", "rot", "probs", "velo"):
        out[k][b][~ok] = 0.0
    for k in ("class_id", "difficulty"):
        out[k][b][~ok] = INVALID_CLASS_ID
    out["valid"][b] = ok
    t_valid[b] = ok
    t_pos[b] = out["pos"][b]
    t_dims[b] = np.maximum(out["dims"][b].astype(np.float32), np.float32(1e-3))
    t_rot[b] = out["rot"][b].reshape(K).astype(np.float32)
    return out, (t_pos, t_dims, t_rot, t_valid)


def flow_cluster_detector_forward(pcl, pcl_is_valid, pcl_w_ground, pillar_coors, point_flow, odom_ta_tb, time_delta_s,
                                  grid_pts_xy, pix_per_m, *, min_num_pts_per_box=10, max_box_len_m=7.0, aspect_ratio_max=4.0,
                                  min_box_area_m2=0.35, min_box_volume_m3=0.5, slope=15.0, buffer=0.25):
    """FlowClusterDetector.forward (flow_cluster_detector.py:87-336) restated on the CPU from the oracle pieces.
    All tensors CPU torch; grid_pts_xy [G,G,2] float32 numpy (pcl_bev_center_coords_homog[..., :2]), pix_per_m [2] float32.
    -> dict(pos [B,S,3], dims [B,S,3], rot [B,S,1], velo [B,S,1], valid [B,S], labels [B,G,G])"""
    import numpy as np

    from . import kabsch as OK

    B = pcl.shape[0]
    G = grid_pts_xy.shape[0]
    dyn, nrf = bev_dynamic_flow(pcl_is_valid, pcl, pillar_coors, point_flow, odom_ta_tb, (G, G))
    mask = (dyn[..., 0] > (time_delta_s * 1.0)[:, None, None]).numpy()
    per_sample, label_imgs = [], []
    for b in range(B):
        lab = dbscan_bev_labels(mask[b], nrf[b].numpy(), grid_pts_xy)
        label_imgs.append(lab)
        props = regionprops_restated(lab)
        K = props.shape[0]
        center, dims2, rot1, dims2_f32, rot1_f32 = boxes_from_regions(props, grid_pts_xy[:, 0, 0], grid_pts_xy[0, :, 1], pix_per_m)
        if K > 0:
            n, z, h = fit_box_z(pcl_w_ground[b][:, :3], torch.from_numpy(center), torch.from_numpy(dims2_f32), torch.from_numpy(rot1_f32),
                                box_height=1000.0)
        else:
            n, z, h = torch.zeros(0, dtype=torch.int64), torch.zeros(0), torch.zeros(0)
        o = mine_filter_compact([K], center[None], dims2[None], rot1[None], n.numpy()[None], z.numpy()[None], h.numpy()[None],
                                min_points=min_num_pts_per_box, aspect_ratio_max=aspect_ratio_max, max_box_len_m=max_box_len_m,
                                min_box_area_m2=min_box_area_m2, min_box_volume_m3=min_box_volume_m3)
        k = int(o["counts"][0])
        per_sample.append((torch.from_numpy(o["pos"][0, :k]), torch.from_numpy(o["dims"][0, :k]), torch.from_numpy(o["rot"][0, :k])))
    S = max(p[0].shape[0] for p in per_sample)
    pos = torch.zeros(B, S, 3)
    dims = torch.zeros(B, S, 3, dtype=torch.float64)
    rot = torch.zeros(B, S, 1, dtype=torch.float64)
    valid = torch.zeros(B, S, dtype=torch.bool)
    for b, (p, d, r) in enumerate(per_sample):
        k = p.shape[0]
        pos[b, :k], dims[b, :k], rot[b, :k], valid[b, :k] = p, d, r, True
    velo = torch.zeros(B, S, 1, dtype=torch.float64)
    if S > 0:
        T, _, _ = OK.kabsch_trafos(pos, dims.float(), rot.float(), pcl[..., :3], pcl_is_valid, point_flow, slope=slope, buffer=buffer)
        rot, velo = box_motion(T, pos, rot)
    return dict(pos=pos, dims=dims, rot=rot, velo=velo, valid=valid, labels=np.stack(label_imgs))
