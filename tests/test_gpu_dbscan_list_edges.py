"""DBSCAN on the list of dynamic pillars (liso_dbscan_components / liso_dbscan_labels, liso_amd/csrc/flow_dbscan.hip) against the
oracle's scikit-learn labels and against a host restatement of the core and root flags, on masks built around the list: none and
one listed cell, a one-cell-wide chain across the grid and across the 16 x 32 union tiles, two blobs that share one border cell (it
takes the smaller rank), a blob of 8 x 14 cells, a fully dynamic grid (the list names every cell), an empty sample between two
others.  Core flags, root flags, the parents of non-core cells and labels are compared in full; a captured replay must equal the
eager call.  The same cases at 0.12 m pillars (window 9) go through the union kernel for windows above 8.  The region moments of
more than 1024 labels (their own kernel) are compared with the oracle's regionprops.  Every device buffer lies between guard bands
(tests/guarded_alloc.py)."""
import ctypes

import numpy as np
import pytest
import torch

from tests.guarded_alloc import guarded

pytestmark = pytest.mark.gpu
DEV = "cuda"
PITCH = 100.0 / 512.0  # eps 1 m = 5 cells in a row, window 6
GRIDS = [(16, 16), (40, 24)]


def centres(gx, gy, pitch=PITCH):
    from liso_amd.utils.bev_utils import get_metric_voxel_center_coords

    return get_metric_voxel_center_coords(np.float32(gx * pitch), np.float32(gy * pitch), np.array([gx, gy], np.int32)).astype(np.float32)


def cases(gx, gy):
    """name -> (mask [B,gx,gy] bool, flow [B,gx,gy,3] float32)"""
    rng = np.random.default_rng(gx * 100 + gy)
    noise = lambda B: (rng.normal(0, 0.02, (B, gx, gy, 3))).astype(np.float32)  # noqa: E731
    out = {}
    out["no dynamic cell"] = (np.zeros((1, gx, gy), bool), noise(1))
    m = np.zeros((1, gx, gy), bool)
    m[0, gx - 1, gy - 2] = True
    out["one dynamic cell"] = (m, noise(1))
    m = np.zeros((1, gx, gy), bool)
    m[0, :, 5] = True  # down every row: across the union tiles of 16 rows
    m[0, gx // 2, :] = True  # and along a row: across the tiles of 32 columns where the grid has them
    out["one-cell-wide chains across the grid"] = (m, np.zeros((1, gx, gy, 3), np.float32))
    # two lines of five cells whose flows differ by 0.8 (weighted 1.6 > eps: never neighbours) and one cell between them at flow 0.4
    # (weighted 0.8 to either: neighbours up to 3 cells away only) that reaches the end of each line: 3 neighbours, not core
    m, f = np.zeros((1, gx, gy), bool), np.zeros((1, gx, gy, 3), np.float32)
    m[0, 3, 0:5], m[0, 3, 7], m[0, 3, 10:15] = True, True, True
    f[0, 3, 7, 0], f[0, 3, 10:15, 0] = 0.4, 0.8
    out["two blobs joined by one border cell"] = (m, f)
    m = np.zeros((1, gx, gy), bool)
    m[0, 4:12, 1:15] = True
    out["a blob of 8 x 14 cells"] = (m, noise(1))
    out["a fully dynamic grid"] = (np.ones((1, gx, gy), bool), noise(1) * 10)
    m = np.zeros((3, gx, gy), bool)
    m[0] = rng.random((gx, gy)) < 0.35
    m[2, 2, :] = True
    m[2, gx - 3:, gy - 4:] = True
    out["batch 3 with an empty middle sample"] = (m, noise(3) * 5)
    return out


def device_labels(mask, flow, xy, pitch=PITCH):
    from liso_amd.networks.flow_cluster_detector.flow_cluster_detector import cluster_dynamic_pillars

    xs, ys = torch.from_numpy(xy[:, 0, 0].copy()).to(DEV), torch.from_numpy(xy[0, :, 1].copy()).to(DEV)
    return cluster_dynamic_pillars(torch.from_numpy(mask).to(DEV), torch.from_numpy(flow).to(DEV), xs, ys, pitch=pitch)


@pytest.mark.parametrize("gx,gy", GRIDS)
def test_labels_equal_scikit_learn(gx, gy):
    from oracle.flow_cluster import dbscan_bev_labels

    xy = centres(gx, gy)
    for name, (mask, flow) in cases(gx, gy).items():
        with guarded() as gd:
            labels, num = device_labels(mask, flow, xy)
            gd.check()
        want = np.stack([dbscan_bev_labels(mask[b], flow[b], xy[..., :2]) for b in range(mask.shape[0])]).astype(np.int32)
        got = labels.cpu().numpy()
        assert got.dtype == np.int32 and got.shape == want.shape
        assert np.array_equal(got, want), (name, int((got != want).sum()))
        assert np.array_equal(num.cpu().numpy(), want.reshape(len(want), -1).max(1)), name
        if name == "two blobs joined by one border cell":
            assert want[0, 3, 4] == 1 and want[0, 3, 10] == 2 and want[0, 3, 7] == 1, want[0, 3]
        if name == "one-cell-wide chains across the grid":
            assert set(np.unique(want)) == {0, 1}


def sklearn_labels(mask, flow, xy):
    from oracle.flow_cluster import dbscan_bev_labels

    return np.stack([dbscan_bev_labels(mask[b], flow[b], xy[..., :2]) for b in range(mask.shape[0])]).astype(np.int32)


def host_restatement(mask, flow, xy, pitch=PITCH, eps=1.0, min_samples=5, flow_weight=2.0):
    """core uint8, is_root int32, labels int32 [B,gx,gy] in numpy: a dynamic cell is core when at least min_samples dynamic cells of
    its window (itself included) lie within eps -- squared distance in fp64 from the fp32 features (x, y, flow_weight * flow), summed
    in feature order as dist_sqr does; a root is the first core cell, in row-major order, of a scikit-learn label"""
    win = int(eps / pitch) + 1
    core, is_root, labels = np.zeros(mask.shape, np.uint8), np.zeros(mask.shape, np.int32), sklearn_labels(mask, flow, xy)
    for b in range(mask.shape[0]):
        r, c = np.nonzero(mask[b])  # row-major
        feat = np.concatenate([xy[r, 0, 0][:, None], xy[0, c, 1][:, None], np.float32(flow_weight) * flow[b, r, c]], -1)
        assert feat.dtype == np.float32
        d = feat.astype(np.float64)[:, None] - feat.astype(np.float64)[None]
        dist = d[..., 0] ** 2 + d[..., 1] ** 2 + d[..., 2] ** 2 + d[..., 3] ** 2 + d[..., 4] ** 2
        in_window = (np.abs(r[:, None] - r[None]) <= win) & (np.abs(c[:, None] - c[None]) <= win)
        is_core = ((dist <= eps * eps) & in_window).sum(1) >= min_samples
        core[b, r, c] = is_core
        lab = labels[b, r, c]
        for k in range(1, int(labels[b].max()) + 1):
            first = np.flatnonzero(is_core & (lab == k))[0]
            is_root[b, r[first], c[first]] = 1
    return dict(core=core, is_root=is_root, labels=labels)


def device_passes(mask, flow, xy):
    """core, parent, is_root, labels of the two entry points (poisoned outputs, a workspace of exactly the bytes asked for)"""
    from liso_amd import _lib as L
    from liso_amd.networks.flow_cluster_detector.mining_ops import inclusive_scan_i32

    lib = L.lib()
    B, gx, gy = mask.shape
    dyn = torch.from_numpy(mask.astype(np.uint8)).to(DEV)
    fl = torch.from_numpy(flow).to(DEV)
    xs, ys = torch.from_numpy(xy[:, 0, 0].copy()).to(DEV), torch.from_numpy(xy[0, :, 1].copy()).to(DEV)
    cfg = L.DbscanCfg(B, gx, gy, int(1.0 / PITCH) + 1, 5, 1.0, 2.0)
    nbytes = lib.liso_dbscan_workspace_bytes(ctypes.byref(cfg))
    assert nbytes > 0
    poison = lambda dt: torch.empty((B, gx, gy), dtype=dt, device=DEV).fill_(0x5A)  # noqa: E731
    core, parent, is_root, labels = poison(torch.uint8), poison(torch.int32), poison(torch.int32), poison(torch.int32)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV).fill_(0xA5)
    a = (ctypes.byref(cfg), L.ptr(dyn), L.ptr(xs), L.ptr(ys), L.ptr(fl), L.ptr(core), L.ptr(parent), L.ptr(is_root))
    assert lib.liso_dbscan_components(*a, L.ptr(ws), nbytes, L.stream_ptr()) == 0
    rank = inclusive_scan_i32(is_root.view(B, -1)).view(B, gx, gy)
    la = (ctypes.byref(cfg), L.ptr(dyn), L.ptr(xs), L.ptr(ys), L.ptr(fl), L.ptr(core), L.ptr(parent), L.ptr(rank), L.ptr(labels))
    assert lib.liso_dbscan_labels(*la, L.ptr(ws), nbytes, L.stream_ptr()) == 0
    assert lib.liso_dbscan_components(*a, L.ptr(ws), nbytes - 1, L.stream_ptr()) == -2  # a short workspace is refused
    assert lib.liso_dbscan_labels(*la, L.ptr(ws), nbytes - 1, L.stream_ptr()) == -2
    return {k: v.cpu().numpy() for k, v in dict(core=core, parent=parent, is_root=is_root, labels=labels).items()}


@pytest.mark.parametrize("gx,gy", GRIDS)
def test_core_flags_roots_and_labels_equal_the_host_restatement(gx, gy):
    xy = centres(gx, gy)
    for name, (mask, flow) in cases(gx, gy).items():
        with guarded() as gd:
            got = device_passes(mask, flow, xy)
            gd.check()
        want = host_restatement(mask, flow, xy)
        for k in want:
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (name, k)
            assert got[k].tobytes() == want[k].tobytes(), (name, k, int((got[k] != want[k]).sum()))
        assert np.all(got["parent"][got["core"] == 0] == -1), name


WIDE_PITCH = 0.12  # eps 1 m = 8 cells in a row, window 9: above the 8 the tiled union holds in LDS


@pytest.mark.parametrize("gx,gy", GRIDS[1:])
def test_labels_equal_scikit_learn_with_window_9(gx, gy):
    assert int(1.0 / WIDE_PITCH) + 1 == 9
    xy = centres(gx, gy, WIDE_PITCH)
    todo = cases(gx, gy)
    # a line of five cells (all core: each sees the five) and one cell 8 columns = 0.96 m behind its end: two neighbours, a border cell
    m = np.zeros((1, gx, gy), bool)
    m[0, 3, 0:5], m[0, 3, 12] = True, True
    todo["a line with a border cell"] = (m, np.zeros((1, gx, gy, 3), np.float32))
    for name, (mask, flow) in todo.items():
        with guarded() as gd:
            labels, num = device_labels(mask, flow, xy, WIDE_PITCH)
            gd.check()
        want = sklearn_labels(mask, flow, xy)
        got = labels.cpu().numpy()
        assert got.dtype == np.int32 and got.shape == want.shape
        assert np.array_equal(got, want), (name, int((got != want).sum()))
        assert np.array_equal(num.cpu().numpy(), want.reshape(len(want), -1).max(1)), name
        if name == "a line with a border cell":
            assert want[0, 3, 12] == 1 and host_restatement(mask, flow, xy, WIDE_PITCH)["core"][0, 3, 12] == 0


def test_region_props_of_more_than_1024_labels():
    """max_labels = 1025: the workspace query gives 0 and the moments are summed by the kernel with global atomics"""
    from liso_amd import _lib as L
    from liso_amd.networks.flow_cluster_detector.flow_cluster_detector import label_region_props
    from oracle.flow_cluster import regionprops_restated

    K = 1025
    assert L.lib().liso_region_props_workspace_bytes(2, 16, 16, K - 1) > 0 and L.lib().liso_region_props_workspace_bytes(2, 16, 16, K) == 0
    lab = np.zeros((2, 16, 16), np.int32)
    lab[0, 1:4, 2:9], lab[0, 5:12, 0], lab[0, 15, 15], lab[0, 9:11, 9:11] = 1, 2, 3, 1025
    lab[0, 6, 5], lab[0, 7, 6], lab[0, 8, 7], lab[0, 8, 8] = 700, 700, 700, 700
    lab[1, 0, :], lab[1, 2:16, 3:5], lab[1, 4, 10] = 1025, 1, 1024
    lab[1, 14, 14] = 1026  # above max_labels: ignored
    with guarded() as gd:
        props = label_region_props(torch.from_numpy(lab).to(DEV), K)
        gd.check()
    props = props.cpu().numpy()
    assert props.dtype == np.float64 and props.shape == (2, K, 5)
    for b in range(2):
        img = np.where(lab[b] <= K, lab[b], 0)
        present = np.unique(img[img > 0])
        np.testing.assert_allclose(props[b, present - 1], regionprops_restated(img), rtol=1e-9, atol=1e-9)
        absent = np.setdiff1d(np.arange(1, K + 1), present)
        assert not props[b, absent - 1].any()


def test_a_captured_replay_equals_the_eager_call():
    from liso_amd.utils.graph_capture import capture

    gx, gy = GRIDS[1]
    xy = centres(gx, gy)
    mask, flow = cases(gx, gy)["batch 3 with an empty middle sample"]
    eager, _ = device_labels(mask, flow, xy)
    md, fd = torch.from_numpy(mask).to(DEV), torch.from_numpy(flow).to(DEV)
    xs, ys = torch.from_numpy(xy[:, 0, 0].copy()).to(DEV), torch.from_numpy(xy[0, :, 1].copy()).to(DEV)
    from liso_amd.networks.flow_cluster_detector.flow_cluster_detector import cluster_dynamic_pillars

    stream = torch.cuda.Stream()
    graph, (labels, num) = capture(lambda: cluster_dynamic_pillars(md, fd, xs, ys, pitch=PITCH), stream, warm_ups=2)
    for _ in range(2):  # a replay on changed inputs, then on the first ones again: nothing of the list survives between replays
        md.copy_(torch.from_numpy(np.roll(mask, 1, axis=0)).to(DEV))
        graph.replay()
        md.copy_(torch.from_numpy(mask).to(DEV))
        graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(labels.cpu().numpy(), eager.cpu().numpy())
