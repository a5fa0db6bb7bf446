"""Generates tests/golden/flow_labels_reference.npz with the reference's own python.

Called directly from the reference: `get_points_in_box_mask` and `extract_lidar_flow_ta_tb`
(liso/datasets/kitti/create_kitti_tracking.py), `update_dynamic_flow` (liso/datasets/argoverse2/create.py) on the reference's
`Shape`, and `find_jumps`, `find_cols`, `kitti_pcl_projection_get_rows_cols`
(liso/datasets/kitti/kitti_range_image_projection_helper.py).  The two builder modules cannot be imported whole (pykitti, av2, the
nuScenes devkit): the three functions are compiled at generation time from the reference files' own text; nothing of the reference
is stored.  Absent third-party modules are stubbed with empty modules (no arithmetic).  nuScenes' loop
(liso/datasets/nuscenes/create.py:229-238, :301-366) is inline in a 450-line function: it is stated here in the generator's own
words around `get_points_in_box_mask` -- the sequential overwrite, the semantic gate at t0 (:339-342), the ungated
num_lidar_pts_t0 (:374).

The generator asserts what the tests rely on, and fails loudly otherwise:
  * no kept point lies within 1e-6 m of a box face in the box frame (points that do are removed beforehand, at most 1 % of them);
  * the reference's LU inverse and the closed form [R^T | -R^T t] give the same membership on the remaining points;
  * no azimuth difference lies within 1e-5 rad of the jump threshold, no column value within 1e-3 of an integer (points that do
    are removed beforehand).
Run in the build container only:
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_flow_labels_golden.py
"""
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, "/root/reference")

from make_targets_golden import import_with_stubs  # noqa: E402
from make_tracking_golden import function_from_reference_file  # noqa: E402

REF = "/root/reference/liso/datasets"
FACE_MARGIN, AZ_MARGIN, COL_MARGIN, THRESHOLD = 1e-6, 1e-5, 1e-3, -0.005


def rot(axis, a):
    c, s = np.cos(a), np.sin(a)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.eye(3)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def pose(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def closed_inverse(T):
    out = np.eye(4)
    out[:3, :3] = T[:3, :3].T
    out[:3, 3] = -(T[:3, :3].T @ T[:3, 3])
    return out


def box_frame(T, pts, inverse):
    return np.einsum("ij,nj->ni", inverse(T), np.concatenate([pts.astype(np.float64), np.ones((pts.shape[0], 1))], -1))[:, :3]


def cloud_around(g, poses, sizes, n, per_box=120):
    """n float32 points: a cluster in and around every box, the rest uniform; points near a box face removed (at most 1 %)"""
    p = np.concatenate([g.uniform(-45, 45, (n, 2)), g.uniform(-3, 2, (n, 1))], -1)
    for k, (T, s) in enumerate(zip(poses, sizes)):
        local = g.uniform(-0.75, 0.75, (per_box, 3)) * s
        p[k * per_box:(k + 1) * per_box] = local @ T[:3, :3].T + T[:3, 3]
    p = p[g.permutation(n)].astype(np.float32)
    near = np.zeros(n, bool)
    for T, s in zip(poses, sizes):
        for inverse in (np.linalg.inv, closed_inverse):
            near |= (np.abs(np.abs(box_frame(T, p, inverse)) - s / 2.0) < FACE_MARGIN).any(-1)
    assert near.sum() <= 0.01 * n, near.sum()
    p = p[~near]
    for T, s in zip(poses, sizes):  # the LU inverse and the closed form agree on who is inside
        lu = (np.abs(box_frame(T, p, np.linalg.inv)) < s / 2.0).all(-1)
        cf = (np.abs(box_frame(T, p, closed_inverse)) < s / 2.0).all(-1)
        assert np.array_equal(lu, cf)
    return p


def homog(p):
    return np.concatenate([p[:, :3].astype(np.float64), np.ones((p.shape[0], 1))], -1)


def kitti_case(K, out):
    g = np.random.default_rng(5)
    # velo_T_cam: the axis swap of the KITTI calibration with a small 3-D misalignment; objects rotate about the camera's y axis
    velo_T_cam = pose(rot(0, 0.013) @ rot(1, -0.007) @ rot(2, 0.011) @ np.array([[0.0, 0, 1], [-1, 0, 0], [0, -1, 0]]), [0.27, 0.06, -0.08])

    def obj(xz, ry, y=1.6):
        return velo_T_cam @ pose(rot(1, ry), [xz[0], y, xz[1]])

    ids_a = np.array([7, 3, 12, 3000, 5, 9, 41], np.int64)
    cam_xz = np.array([[4.0, 12.0], [-6.0, 20.0], [4.6, 12.4], [10.0, 30.0], [-3.0, 8.0], [-3.2, 8.3], [15.0, 15.0]])  # 0/2 and 4/5 overlap
    ry_a = g.uniform(-np.pi, np.pi, 7)
    ry_a[2], ry_a[5] = ry_a[0] + 0.2, ry_a[4] - 0.15
    dims = np.stack([g.uniform(3.6, 4.8, 7), g.uniform(1.6, 2.1, 7), g.uniform(1.4, 1.9, 7)], -1)
    pose_a = np.stack([obj(cam_xz[k], ry_a[k]) for k in range(7)])
    # at tb: another order; id 12 (box 2, the later one of an overlapping pair) and id 41 are gone, id 77 is new; id 9 stands still
    ids_b = np.array([5, 77, 3000, 7, 9, 3], np.int64)
    odom = pose(rot(2, 0.02) @ rot(1, 0.001), [1.1, 0.03, -0.01])
    pose_b = []
    for tid in ids_b:
        if tid == 77:
            pose_b.append(obj([20.0, 5.0], 0.3))
            continue
        k = int(np.flatnonzero(ids_a == tid)[0])
        moved = obj(cam_xz[k] + g.uniform(-1.0, 1.0, 2), ry_a[k] + g.uniform(-0.1, 0.1))
        pose_b.append(np.linalg.inv(odom) @ (pose_a[k] if tid == 9 else moved))
    pose_b = np.stack(pose_b)
    pcl = cloud_around(g, pose_a, dims, 4000)
    ph = homog(pcl)
    flow, mask = K.extract_lidar_flow_ta_tb(pcl_homog_ta=ph, lidar_Tta_obj=pose_a, obj_dims_ta=dims, track_ids_ta=ids_a, track_ids_tb=ids_b,
                                            lidar_Ttb_obj=pose_b, odom_ta_tb=odom)
    inside = np.stack([K.get_points_in_box_mask(ph, pose_a[k], dims[k]) for k in range(7)])
    # (np.where promotes the uint16 mask by the ids' dtype: the values, not the dtype, are the fixture)
    assert mask.max() == 65535 and inside.sum(1).min() > 20 and (inside.sum(0) > 1).sum() > 20, (inside.sum(1), (inside.sum(0) > 1).sum())
    mask = mask.astype(np.int64)
    assert ((mask == 12) & inside[0]).sum() > 5  # id from the unpartnered later box, flow from the partnered earlier one
    out.update(kitti_pcl=pcl, kitti_pose_a=pose_a, kitti_dims=dims, kitti_ids_a=ids_a, kitti_ids_b=ids_b, kitti_pose_b=pose_b,
               kitti_odom=odom, kitti_flow=flow, kitti_ids_mask=mask, kitti_inside=inside)
    print("kitti points per box", inside.sum(1))


def nusc_case(K, out):
    g = np.random.default_rng(6)
    n_box = 6
    ann_idx = np.array([0, 2, 3, 5, 6, 9])  # annotations that cannot move are skipped by the builder: the index is not the slot
    box_class = np.array([4, 4, 7, 4, 7, 4], np.int32)
    xy = np.array([[8.0, 3.0], [8.5, 3.4], [-12.0, 6.0], [20.0, -9.0], [-5.0, -14.0], [-5.3, -14.2]])  # 0/1 and 4/5 overlap
    yaw0 = g.uniform(-np.pi, np.pi, n_box)
    yaw0[1], yaw0[5] = yaw0[0] + 0.1, yaw0[4] + 0.2
    size = np.stack([g.uniform(3.8, 4.9, n_box), g.uniform(1.7, 2.1, n_box), g.uniform(1.4, 1.8, n_box)], -1)
    tilt = [rot(0, a) @ rot(1, b) for a, b in g.uniform(-0.03, 0.03, (n_box, 2))]
    pose_t0 = np.stack([pose(rot(2, yaw0[k]) @ tilt[k], [xy[k, 0], xy[k, 1], -0.9]) for k in range(n_box)])
    step = g.uniform(-1.2, 1.2, (n_box, 2))
    pose_t1 = np.stack([pose(rot(2, yaw0[k] + 0.05) @ tilt[k], [xy[k, 0] + step[k, 0], xy[k, 1] + step[k, 1], -0.9]) for k in range(n_box)])
    odom = pose(rot(2, -0.015), [0.9, -0.02, 0.0])
    pcl_t0, pcl_t1 = cloud_around(g, pose_t0, size, 3000), cloud_around(g, pose_t1, size, 3000)
    sem_t0 = g.choice(np.array([4, 7, 11], np.int32), pcl_t0.shape[0], p=[0.6, 0.3, 0.1])
    h0, h1, eye = homog(pcl_t0), homog(pcl_t1), np.eye(4)
    flow_01 = np.einsum("ij,kj->ki", np.linalg.inv(odom) - eye, h0)
    flow_10 = np.einsum("ij,kj->ki", odom - eye, h1)
    found_t0, found_t1 = np.zeros(h0.shape[0], bool), np.zeros(h1.shape[0], bool)
    idx_t0, idx_t1 = np.zeros(h0.shape[0], np.uint8), np.zeros(h1.shape[0], np.uint8)
    num_pts = np.zeros(n_box, np.int64)
    for k in range(n_box):
        in_t0 = K.get_points_in_box_mask(h0, pose_t0[k], size[k])
        own_t0 = in_t0 & (sem_t0 == box_class[k])
        dyn = np.einsum("ij,nj->ni", pose_t1[k] @ np.linalg.inv(pose_t0[k]) - eye, h0)
        flow_01[own_t0] = dyn[own_t0]
        idx_t0[own_t0], found_t0[own_t0] = ann_idx[k], True
        num_pts[k] = np.count_nonzero(in_t0)
        in_t1 = K.get_points_in_box_mask(h1, pose_t1[k], size[k])
        idx_t1[in_t1], found_t1[in_t1] = ann_idx[k], True
        dyn = np.einsum("ij,nj->ni", pose_t0[k] @ np.linalg.inv(pose_t1[k]) - eye, h1)
        flow_10[in_t1] = dyn[in_t1]
    assert 0 < found_t0.sum() < num_pts.sum() and found_t1.sum() > 100
    out.update(nusc_pcl_t0=pcl_t0, nusc_pcl_t1=pcl_t1, nusc_sem_t0=sem_t0, nusc_pose_t0=pose_t0, nusc_pose_t1=pose_t1, nusc_size=size,
               nusc_ann_idx=ann_idx.astype(np.int32), nusc_box_class=box_class, nusc_odom=odom, nusc_flow_t0_t1=flow_01[:, :3],
               nusc_flow_t1_t0=flow_10[:, :3], nusc_idx_t0=idx_t0, nusc_idx_t1=idx_t1, nusc_found_t0=found_t0, nusc_found_t1=found_t1,
               nusc_num_pts_t0=num_pts)
    print("nusc points per box", num_pts, "gated", found_t0.sum())


def av2_case(update_dynamic_flow, Shape, out):
    g = np.random.default_rng(7)
    cats = np.array([0, 0, 1, 0, 1, 1, 0])
    pos_a = np.array([[9.0, 2.0, -0.8], [9.5, 2.3, -0.8], [-15.0, 8.0, -0.7], [25.0, -11.0, -0.9], [-4.0, -16.0, -0.8], [-4.3, -16.3, -0.8],
                      [30.0, 20.0, -0.6]])  # 0/1 overlap within category 0, 4/5 within category 1
    rot_a = g.uniform(-np.pi, np.pi, (7, 1))
    rot_a[1], rot_a[5] = rot_a[0] + 0.15, rot_a[4] - 0.1
    dims = np.stack([g.uniform(3.8, 4.9, 7), g.uniform(1.7, 2.1, 7), g.uniform(1.4, 1.8, 7)], -1)
    pos_b = pos_a + np.concatenate([g.uniform(-1.0, 1.0, (7, 2)), np.zeros((7, 1))], -1)
    rot_b = rot_a + g.uniform(-0.08, 0.08, (7, 1))
    odom = pose(rot(2, 0.01), [1.3, 0.01, 0.0])
    boxes_a = Shape(pos=pos_a, dims=dims, rot=rot_a, probs=np.ones((7, 1)))
    boxes_b = Shape(pos=pos_b, dims=dims, rot=rot_b, probs=np.ones((7, 1)))
    pcl = cloud_around(g, boxes_a.get_poses(), dims, 3000)
    ph = homog(pcl)
    flow = np.einsum("ij,nj->ni", np.linalg.inv(odom) - np.eye(4), ph)[:, :3]
    out["av2_flow_rigid"] = flow.copy()
    for cat in (0, 1):
        flow = update_dynamic_flow(ph, flow, boxes_a[cats == cat], boxes_b[cats == cat])
    assert (np.abs(flow - out["av2_flow_rigid"]).max(-1) > 1e-3).sum() > 200
    out.update(av2_pcl=pcl, av2_cats=cats, av2_pos_a=pos_a, av2_rot_a=rot_a, av2_pos_b=pos_b, av2_rot_b=rot_b, av2_dims=dims, av2_odom=odom,
               av2_flow=flow)


def scan(g, rings, per_ring, num_columns=2000):
    """a KITTI-like scan in file order: per ring the flipped azimuth rises from -pi to pi with a little backward jitter (smaller
    than the threshold), then falls back.  Points within the margins of a decision are removed until none is left."""
    az = []
    for _ in range(rings):
        a = np.sort(g.uniform(-3.1, 3.1, per_ring))
        a[1:-1] += g.uniform(-0.002, 0.002, per_ring - 2)
        az.append(a)
    az = np.concatenate(az)
    rho = g.uniform(4.0, 60.0, az.shape[0])
    pc = np.stack([-np.cos(az) * rho, -np.sin(az) * rho, g.uniform(-2, 1, az.shape[0])], -1).astype(np.float32)
    n0 = pc.shape[0]
    while True:
        flipped = -np.arctan2(pc[:, 1], -pc[:, 0])
        bad = np.zeros(pc.shape[0], bool)
        bad[1:] = np.abs(np.ediff1d(flipped).astype(np.float64) - THRESHOLD) < AZ_MARGIN
        col = ((num_columns - 1) * (np.pi - np.arctan2(pc[:, 1], pc[:, 0]).astype(np.float64)) / (2 * np.pi))
        bad |= np.abs(col - np.round(col)) < COL_MARGIN
        if not bad.any():
            break
        pc = pc[~bad]
    assert pc.shape[0] >= 0.98 * n0, (pc.shape[0], n0)
    return pc


def projection_case(P, out):
    g = np.random.default_rng(8)
    full, short = scan(g, 64, 40), scan(g, 41, 30)
    rows, cols = P.kitti_pcl_projection_get_rows_cols(full)
    assert rows.dtype == np.int32 and cols.dtype == np.int32 and rows[-1] == 63 and 0 <= cols.min() and cols.max() <= 1999
    short_rows = P.find_jumps(short)
    assert short_rows[-1] == 40
    out.update(rp_full=full, rp_full_rows=rows, rp_full_cols=cols, rp_short=short, rp_short_rows=short_rows,
               rp_short_rows_corrected=P.find_jumps(short, auto_correct=True), rp_short_cols=P.find_cols(short),
               rp_short_cols_512=P.find_cols(short, num_columns=512))


def main():
    import types

    def _imp():
        import liso.datasets.kitti.kitti_range_image_projection_helper as P
        from liso.kabsch.shape_utils import Shape
        return P, Shape

    P, Shape = import_with_stubs(_imp)
    env = {"np": np}
    K = types.SimpleNamespace(**{name: function_from_reference_file(f"{REF}/kitti/create_kitti_tracking.py", name, env)
                                 for name in ("get_points_in_box_mask", "extract_lidar_flow_ta_tb")})
    update_dynamic_flow = function_from_reference_file(f"{REF}/argoverse2/create.py", "update_dynamic_flow", {"np": np})
    out = {}
    kitti_case(K, out)
    nusc_case(K, out)
    av2_case(update_dynamic_flow, Shape, out)
    projection_case(P, out)
    np.savez_compressed(os.path.join(HERE, "flow_labels_reference.npz"), **out)
    print({k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
