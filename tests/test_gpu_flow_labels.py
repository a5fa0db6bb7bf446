"""Flow labels and KITTI rows / columns on the device (include/liso_flow_labels.h) against the numpy restatement of
liso_amd/datasets/flow_labels.py and range_projection.py: bit for bit, flow included, at the smallest shapes that take every path
-- one and several point tiles, no box, one box and more than one LDS chunk of boxes, jobs that share a cloud, an empty cloud, a job
without a valid box, NaN rows, both overlap rules, the class gate, keep_flow, absent outputs -- the golden cases once, and one
capture and replay."""
import numpy as np
import pytest
import torch

from liso_amd.datasets import flow_labels as F
from liso_amd.datasets import range_projection as R
from liso_amd.utils import graph_capture
from test_flow_labels import G, assert_flow_close, av2_boxes, check_nusc, homog, nusc_sample

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
J, C = 5, 3
CLOUD_OF = np.array([0, 1, 1, 2, 0], np.int32)  # jobs 1 and 2 share cloud 1; cloud 2 is empty; job 4 has no valid box


def to(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def random_rotation(g):
    q = g.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def scene(n_max, K, seed):
    """the inputs of flow_labels as numpy arrays: points and box centres within +-6 m, boxes of 2 .. 6 m, so that with 131 slots a
    point lies in about four boxes (131 * 0.85 * 4^3 / 12^3); every pose_a a full 3-D rotation"""
    g = np.random.default_rng(seed)
    pcl = g.uniform(-6, 6, (C, n_max, 4)).astype(np.float32)
    counts = np.array([n_max, max(n_max - 7, 0) if n_max > 1 else 1, 0], np.int32)
    if n_max > 20:
        pcl[0, 3, 0], pcl[1, 11, 2], pcl[0, 17, 1] = np.nan, np.inf, np.nan  # rows with a non-finite coordinate, inside the count
    pose_a, pose_b = np.tile(np.eye(4), (J, K, 1, 1)), np.tile(np.eye(4), (J, K, 1, 1))
    for j in range(J):
        for k in range(K):
            pose_a[j, k, :3, :3], pose_a[j, k, :3, 3] = random_rotation(g), g.uniform(-6, 6, 3)
            pose_b[j, k, :3, :3], pose_b[j, k, :3, 3] = random_rotation(g), pose_a[j, k, :3, 3] + g.uniform(-1, 1, 3)
    odom = np.tile(np.eye(4), (J, 1, 1))
    for j in range(J):
        odom[j, :3, :3], odom[j, :3, 3] = random_rotation(g), g.uniform(-1, 1, 3)
    valid = g.uniform(size=(J, K)) < 0.85
    valid[4] = False
    return dict(pcl=pcl, counts=counts, cloud_of=CLOUD_OF.copy(), odom=odom, pose_a=pose_a, pose_b=pose_b, size=g.uniform(2, 6, (J, K, 3)),
                valid=valid, has_b=g.uniform(size=(J, K)) < 0.6, label=g.integers(0, 60000, (J, K)).astype(np.int32),
                box_class=g.integers(-1, 3, (J, K)).astype(np.int32), point_class=g.integers(0, 3, (C, n_max)).astype(np.int32))


def call_both(s, gate, **kw):
    """-> (device result, host result) of the same call"""
    names = ("pcl", "counts", "cloud_of", "odom", "pose_a", "pose_b", "size", "valid", "has_b", "label") + (("box_class", "point_class") if gate else ())
    flow = kw.pop("flow", None)
    dev = F.flow_labels(*(to(s[k]) for k in names), flow=to(flow), **kw)
    host_kw = {k: v for k, v in kw.items() if not k.startswith("want_")}
    host = F.flow_labels_host(*(s[k] for k in names), flow=None if flow is None else flow.copy(), **host_kw)
    torch.cuda.synchronize()
    return dev, host


def assert_same(dev, host):
    assert np.array_equal(dev.flow.cpu().numpy().view(np.uint32), host.flow.view(np.uint32))  # bit for bit, NaN rows included
    for name in ("point_label", "point_box", "count"):
        d = getattr(dev, name)
        if d is not None:
            assert d.dtype == torch.int32 and np.array_equal(d.cpu().numpy(), getattr(host, name)), name


@pytest.mark.parametrize("K", [0, 1, F.CHUNK + 3])
@pytest.mark.parametrize("n_max", [1, 63, 257, 1000])
def test_device_equals_host_bit_for_bit(n_max, K):
    s = scene(n_max, K, seed=100 * n_max + K)
    before = np.random.default_rng(2).normal(size=(J, n_max, 3)).astype(np.float32)
    for overlap, gate, keep in ((F.LAST, False, False), (F.FIRST, False, False), (F.LAST, True, False), (F.FIRST, True, True),
                                (F.LAST, False, True)):
        dev, host = call_both(s, gate, overlap=overlap, keep_flow=keep, flow=before if keep else None, no_label=65535)
        assert_same(dev, host)
        if K > 1 and n_max >= 257:  # the scene does what it is meant to: shared points, both kinds of winner, an empty job
            assert (host.count.sum(0) > 0).sum() > K // 2 and (host.point_box[0] >= 0).sum() > n_max // 2
            assert (host.point_box[4] == -1).all() and np.isnan(host.flow[3]).all()
    dev, host = call_both(s, True, overlap=F.LAST, want_label=False, want_box=False, want_count=False)  # absent outputs
    assert dev.point_label is None and dev.point_box is None and dev.count is None
    assert_same(dev, host)
    dev, host = call_both({**s, "counts": None}, False, want_box=False)  # without counts every row is read
    assert_same(dev, host)


def test_golden_cases_on_the_device():
    flow, ids = F.extract_lidar_flow_ta_tb(pcl_homog_ta=to(homog(G["kitti_pcl"])), lidar_Tta_obj=to(G["kitti_pose_a"]), obj_dims_ta=to(G["kitti_dims"]),
                                           track_ids_ta=to(G["kitti_ids_a"]), track_ids_tb=to(G["kitti_ids_b"]), lidar_Ttb_obj=to(G["kitti_pose_b"]),
                                           odom_ta_tb=to(G["kitti_odom"]))
    hflow, hids = F.extract_lidar_flow_ta_tb(pcl_homog_ta=homog(G["kitti_pcl"]), lidar_Tta_obj=G["kitti_pose_a"], obj_dims_ta=G["kitti_dims"],
                                             track_ids_ta=G["kitti_ids_a"], track_ids_tb=G["kitti_ids_b"], lidar_Ttb_obj=G["kitti_pose_b"],
                                             odom_ta_tb=G["kitti_odom"])
    assert ids.dtype == torch.uint16 and np.array_equal(ids.cpu().numpy(), hids) and np.array_equal(hids.astype(np.int64), G["kitti_ids_mask"])
    assert np.array_equal(flow.cpu().numpy().view(np.uint32), hflow.view(np.uint32))
    assert_flow_close(flow.cpu().numpy(), G["kitti_flow"])
    mask = F.get_points_in_box_mask(to(homog(G["kitti_pcl"])), to(G["kitti_pose_a"][2]), to(G["kitti_dims"][2]))
    assert mask.dtype == torch.bool and np.array_equal(mask.cpu().numpy(), G["kitti_inside"][2])

    sample = nusc_sample()
    out = F.sample_flow_labels(**{k: to(v) if isinstance(v, np.ndarray) else v for k, v in sample.items()})
    check_nusc(out, lambda t: t.cpu().numpy())
    host = F.sample_flow_labels(**sample)
    for k, v in host.items():
        assert np.array_equal(out[k].cpu().numpy(), v, equal_nan=True), k

    flow = to(G["av2_flow_rigid"].astype(np.float32))
    for cat in (0, 1):  # (the poses come from the device's cos / sin: against the reference, not bitwise against the host)
        assert F.update_dynamic_flow(to(homog(G["av2_pcl"])), flow, av2_boxes("a", cat, to), av2_boxes("b", cat, to)) is flow
    assert_flow_close(flow.cpu().numpy(), G["av2_flow"])
    untouched = np.abs(G["av2_flow"] - G["av2_flow_rigid"]).max(-1) == 0
    assert np.array_equal(flow.cpu().numpy()[untouched], G["av2_flow_rigid"].astype(np.float32)[untouched])


def test_capture_and_replay_on_new_contents():
    names = ("pcl", "counts", "cloud_of", "odom", "pose_a", "pose_b", "size", "valid", "has_b", "label", "box_class", "point_class")
    first, second = scene(257, F.CHUNK + 3, seed=1), scene(257, F.CHUNK + 3, seed=2)
    second["cloud_of"] = np.array([1, 0, 0, 2, 1], np.int32)
    static = [to(first[k]) for k in names]
    stream = torch.cuda.Stream()
    graph, res = graph_capture.capture(lambda: F.flow_labels(*static, overlap=F.FIRST), stream, warm_ups=1)
    torch.cuda.synchronize()
    for t, k in zip(static, names):
        t.copy_(to(second[k]))
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        graph.replay()
    torch.cuda.synchronize()
    eager = F.flow_labels(*(to(second[k]) for k in names), overlap=F.FIRST)
    host = F.flow_labels_host(*(second[k] for k in names), overlap=F.FIRST)
    torch.cuda.synchronize()
    assert_same(res, host)
    assert_same(eager, host)


# ---- rows and columns -------------------------------------------------------------------------------------------------------------
def ring_scan(g, rings, per_ring, lead=None):
    """a scan in file order whose every decision keeps the golden generator's margins: per ring the flipped azimuth rises with a little
    backward jitter and falls back at the ring's end; `lead`: the flipped azimuth of one extra first point"""
    az = []
    for _ in range(rings):
        a = np.sort(g.uniform(-3.1, 3.1, per_ring))
        a[1:-1] += g.uniform(-0.002, 0.002, per_ring - 2)
        az.append(a)
    az = np.concatenate(([np.array([lead])] if lead is not None else []) + az)
    rho = g.uniform(4.0, 60.0, az.shape[0])
    pc = np.stack([-np.cos(az) * rho, -np.sin(az) * rho, g.uniform(-2, 1, az.shape[0])], -1).astype(np.float32)
    while True:
        flipped = -np.arctan2(pc[:, 1], -pc[:, 0])
        bad = np.zeros(pc.shape[0], bool)
        bad[1:] = np.abs(np.ediff1d(flipped).astype(np.float64) + 0.005) < 1e-5
        col = 1999 * (np.pi - np.arctan2(pc[:, 1], pc[:, 0]).astype(np.float64)) / (2 * np.pi)
        bad |= np.abs(col - np.round(col)) < 1e-3
        if not bad.any():
            return pc
        pc = pc[~bad]


def check_rows_cols(clouds, auto_correct=False):
    n_max = max(c.shape[0] for c in clouds)
    batch = np.full((len(clouds), n_max, 4), np.nan, np.float32)
    for b, c in enumerate(clouds):
        batch[b, :c.shape[0], :3] = c
    counts = np.array([c.shape[0] for c in clouds], np.int32)
    rows, cols = R.rows_cols_device(to(batch), to(counts), auto_correct=auto_correct)
    rows, cols = rows.cpu().numpy(), cols.cpu().numpy()
    assert rows.dtype == np.int32 and cols.dtype == np.int32
    for b, c in enumerate(clouds):
        n = c.shape[0]
        assert np.array_equal(rows[b, :n], R.find_jumps(c, auto_correct=auto_correct)), b
        assert np.array_equal(cols[b, :n], R.find_cols(c)), b
        assert (rows[b, n:] == -1).all() and (cols[b, n:] == -1).all()


def test_rows_and_columns_equal_the_host():
    g = np.random.default_rng(4)
    full = ring_scan(g, 76, 41)[:3000]  # three tiles of 1024 rows: the running sum and the last azimuth cross tile borders
    no_jump = ring_scan(g, 1, 3200)[:3000]
    lead = ring_scan(g, 5, 20, lead=3.0)
    assert full.shape[0] == 3000 and no_jump.shape[0] == 3000
    assert R.find_jumps(full)[-1] >= 63 and R.find_jumps(no_jump)[-1] == 0 and R.find_jumps(lead)[1] == 1
    check_rows_cols([full[:1], full[:64], full])
    check_rows_cols([full[:65], no_jump, lead])
    check_rows_cols([G["rp_short"], full, full[:64]], auto_correct=True)  # ends at row 40, beyond row 63 (nothing added), at row 1
    rows = R.find_jumps(to(G["rp_short"]), auto_correct=True).cpu().numpy()
    assert np.array_equal(rows, G["rp_short_rows_corrected"]) and rows[-1] == 63
    rows, cols = R.kitti_pcl_projection_get_rows_cols(to(G["rp_full"]))
    assert np.array_equal(rows.cpu().numpy(), G["rp_full_rows"]) and np.array_equal(cols.cpu().numpy(), G["rp_full_cols"])
    assert np.array_equal(R.find_cols(to(G["rp_short"]), num_columns=512).cpu().numpy(), G["rp_short_cols_512"])
    sample = {"pcl_t0": to(G["rp_full"])}
    R.add_lidar_rows_to_kitti_sample(sample, ("t0", "t1"))
    assert sample["lidar_rows_t0"].dtype == torch.uint8 and np.array_equal(sample["lidar_rows_t0"].cpu().numpy(), G["rp_full_rows"].astype(np.uint8))
