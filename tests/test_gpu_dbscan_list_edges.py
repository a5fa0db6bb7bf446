"""DBSCAN on the list of dynamic pillars (liso_dbscan_components_ws / liso_dbscan_labels_ws, liso_amd/csrc/flow_dbscan.hip) against
the oracle's scikit-learn labels and against the dense passes (liso_dbscan_components / liso_dbscan_labels), on masks built around
the list: none and one listed cell, a one-cell-wide chain across the grid and across the 16 x 32 union tiles, two blobs that share
one border cell (it takes the smaller rank), a blob with more than 20 dynamic cells in a wave of the dense pass (its per-lane path),
a fully dynamic grid (the list names every cell), an empty sample between two others.  Core flags, root flags and labels are
compared in full, bit for bit; a captured replay must equal the eager call.  Every device buffer lies between guard bands
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


def centres(gx, gy):
    from liso_amd.utils.bev_utils import get_metric_voxel_center_coords

    return get_metric_voxel_center_coords(np.float32(gx * PITCH), np.float32(gy * PITCH), np.array([gx, gy], np.int32)).astype(np.float32)


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
    out["a blob denser than 20 cells per wave"] = (m, noise(1))
    out["a fully dynamic grid"] = (np.ones((1, gx, gy), bool), noise(1) * 10)
    m = np.zeros((3, gx, gy), bool)
    m[0] = rng.random((gx, gy)) < 0.35
    m[2, 2, :] = True
    m[2, gx - 3:, gy - 4:] = True
    out["batch 3 with an empty middle sample"] = (m, noise(3) * 5)
    return out


def device_labels(mask, flow, xy):
    from liso_amd.networks.flow_cluster_detector.flow_cluster_detector import cluster_dynamic_pillars

    xs, ys = torch.from_numpy(xy[:, 0, 0].copy()).to(DEV), torch.from_numpy(xy[0, :, 1].copy()).to(DEV)
    return cluster_dynamic_pillars(torch.from_numpy(mask).to(DEV), torch.from_numpy(flow).to(DEV), xs, ys, pitch=PITCH)


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


def _dense_and_list(mask, flow, xy):
    """core, is_root, labels of both pairs of entry points on the same inputs (poisoned outputs)"""
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
    out = []
    for use_list in (False, True):
        poison = lambda dt: torch.empty((B, gx, gy), dtype=dt, device=DEV).fill_(0x5A)  # noqa: E731
        core, parent, is_root, labels = poison(torch.uint8), poison(torch.int32), poison(torch.int32), poison(torch.int32)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV).fill_(0xA5)  # exactly the bytes asked for
        a = (ctypes.byref(cfg), L.ptr(dyn), L.ptr(xs), L.ptr(ys), L.ptr(fl), L.ptr(core), L.ptr(parent), L.ptr(is_root))
        rc = lib.liso_dbscan_components_ws(*a, L.ptr(ws), nbytes, L.stream_ptr()) if use_list else lib.liso_dbscan_components(*a, L.stream_ptr())
        assert rc == 0
        rank = inclusive_scan_i32(is_root.view(B, -1)).view(B, gx, gy)
        a = (ctypes.byref(cfg), L.ptr(dyn), L.ptr(xs), L.ptr(ys), L.ptr(fl), L.ptr(core), L.ptr(parent), L.ptr(rank), L.ptr(labels))
        rc = lib.liso_dbscan_labels_ws(*a, L.ptr(ws), nbytes, L.stream_ptr()) if use_list else lib.liso_dbscan_labels(*a, L.stream_ptr())
        assert rc == 0
        if use_list:
            assert lib.liso_dbscan_components_ws(*a[:8], L.ptr(ws), nbytes - 1, L.stream_ptr()) == -2  # a short workspace is refused
        out.append({k: v.cpu().numpy() for k, v in dict(core=core, is_root=is_root, labels=labels, non_core_parent=parent * (core == 0)).items()})
    return out


@pytest.mark.parametrize("gx,gy", GRIDS)
def test_list_passes_equal_the_dense_passes_bit_for_bit(gx, gy):
    xy = centres(gx, gy)
    for name, (mask, flow) in cases(gx, gy).items():
        with guarded() as gd:
            dense, listed = _dense_and_list(mask, flow, xy)
            gd.check()
        for k in dense:
            assert dense[k].tobytes() == listed[k].tobytes(), (name, k, int((dense[k] != listed[k]).sum()))


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
