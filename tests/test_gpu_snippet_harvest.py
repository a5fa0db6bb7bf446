"""GPU: the snippet cut kernel (include/liso_snippets.h) against the reference fixture under the criteria of
tests/test_snippet_harvest.py, against the numpy host path on a seeded case, at the exact boundary, with a capacity below the
total between guard bands, on degenerate jobs, as a captured graph, and through `SnippetHarvester` into `BoxAugmenter`."""
import numpy as np
import pytest
import torch

from guarded_alloc import guarded
from liso_amd import _lib as L
from liso_amd.tracker import snippet_harvest as H
from test_snippet_harvest import G, boundary_case, check_against, fixture_boxes, random_case, small_sequence

pytestmark = pytest.mark.gpu
DEV = "cuda"


class _Cfg(dict):
    __getattr__ = dict.__getitem__


def _cfg(d):
    return _Cfg({k: _cfg(v) if isinstance(v, dict) else v for k, v in d.items()})


def make_cfg(G_, R, box_cfg):
    return _cfg({"data": {"bev_range_m": [R, R], "img_grid_size": [G_, G_], "flow_source": "slim_flow", "train_on_box_source": "mined",
                          "limit_pillar_height": False, "augmentation": {"boxes": dict(box_cfg, active=True)}},
                 "network": {"name": "pointpillars"}, "loss": {"supervised": {"centermaps": {"confidence_target": "gaussian"}}}})


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(res):
    return tuple(None if t is None else t.cpu().numpy() for t in res)


def device_cut(c, capacity=None, job_cloud=None):
    return H.cut_box_snippets(dev(c["clouds"]), dev(c["counts"]) if c.get("counts") is not None else None, dev(c["lidar_rows"]),
                              c["job_cloud"] if job_cloud is None else job_cloud, c["boxes7"], capacity=capacity)


@pytest.fixture(scope="module")
def case():
    c = random_case()
    c["host"] = H.cut_box_snippets_host(c["clouds"], c["counts"], c["lidar_rows"], c["job_cloud"], c["boxes7"])
    return c


def test_device_matches_reference():
    got = H.cut_box_snippets(dev(G["cut_clouds"]), dev(G["cut_counts"]), dev(G["cut_lidar_rows"]), G["cut_job_cloud"], fixture_boxes())
    check_against(host(got), G["cut_offsets"], G["cut_points"], G["cut_rows"], G["cut_box_T_sensor"], "device vs reference", 1e-12)


def test_device_matches_host_path_and_repeats_bitwise(case):
    first, second = host(device_cut(case)), host(device_cut(case))
    want = case["host"]
    check_against(first, want[0], want[1], want[2], want[3], "device vs host path", 1e-12)
    for a, b in zip(first, second):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), "two runs differ"


def test_device_exact_boundary():
    clouds, rows, job_cloud, b7, inside = boundary_case()
    offsets, points, got_rows, box_T = host(H.cut_box_snippets(dev(clouds), None, dev(rows), job_cloud, b7))
    assert offsets.tolist() == [0, 3] and np.array_equal(got_rows, inside)
    assert np.array_equal(points, clouds[0, inside])
    assert np.array_equal(box_T[0], np.eye(4))


def test_capacity_below_the_total_writes_nothing_behind_it(case):
    want = case["host"]
    total = int(want[0][-1])
    for capacity in (total - 1, total // 2 + 3, 1):
        with guarded() as g:  # every buffer the wrapper allocates lies between canary bands
            offsets, points, rows, _ = device_cut(case, capacity=capacity)
            assert g.check() >= 4
        assert points.shape == (capacity, 4) and rows.shape == (capacity,)
        assert np.array_equal(offsets.cpu().numpy(), want[0]), "the offsets report the true totals"
        assert np.array_equal(rows.cpu().numpy(), want[2][:capacity])
        assert np.array_equal(points.cpu().numpy()[:, 3], want[1][:capacity, 3])
    full = host(device_cut(case))
    assert np.array_equal(points.cpu().numpy(), full[1][:1])
    # a buffer larger than the total: the rows behind the total are not written
    sentinel = torch.full((total + 64, 4), -7.0, device=DEV)
    offsets = torch.empty(len(want[0]), dtype=torch.int64, device=DEV)
    out_rows = torch.full((total + 64,), -7, dtype=torch.int32, device=DEV)
    clouds, counts, lrows = dev(case["clouds"]), dev(case["counts"]), dev(case["lidar_rows"])
    jc, b7 = dev(case["job_cloud"]), dev(case["boxes7"])
    ws = torch.empty(int(L.lib().liso_snippet_cut_workspace_bytes(3, 5000, 9)), dtype=torch.uint8, device=DEV)
    L.check(L.lib().liso_snippet_cut_f32(3, 5000, 4, L.ptr(clouds), L.ptr(counts), L.ptr(lrows), 9, L.ptr(jc), L.ptr(b7), total + 64, L.ptr(offsets),
                                         L.ptr(sentinel), L.ptr(out_rows), None, L.ptr(ws), ws.numel(), L.stream_ptr()), "snippet_cut")
    assert np.array_equal(sentinel.cpu().numpy()[:total], full[1]) and bool((sentinel[total:] == -7.0).all()) and bool((out_rows[total:] == -7).all())


def test_degenerate_jobs(case):
    clouds, lrows = dev(case["clouds"]), dev(case["lidar_rows"])
    offsets, points, rows, box_T = H.cut_box_snippets(clouds, None, lrows, np.zeros(0, np.int32), np.zeros((0, 7), np.float32))
    assert offsets.cpu().tolist() == [0] and points.shape == (0, 4) and rows.shape == (0,) and box_T.shape == (0, 4, 4)
    # a NaN box row, and sweep indices outside [0, T) handed to the C ABI as they are (a device tensor is not checked on the host)
    b7 = case["boxes7"].copy()
    b7[1, 4] = np.nan
    b7[4, 6] = np.nan
    job_cloud = case["job_cloud"].copy()
    job_cloud[5], job_cloud[6] = 3, -1
    with pytest.raises(AssertionError):
        H.cut_box_snippets(clouds, dev(case["counts"]), lrows, job_cloud, b7)
    with guarded() as g:
        got = host(H.cut_box_snippets(clouds, dev(case["counts"]), lrows, dev(job_cloud), b7))
        g.check()
    sizes, want_sizes = np.diff(got[0]), np.diff(case["host"][0])
    assert sizes[[1, 4, 5, 6]].tolist() == [0, 0, 0, 0]
    others = [0, 2, 3, 7, 8]
    assert np.array_equal(sizes[others], want_sizes[others])
    want_rows = np.concatenate([case["host"][2][case["host"][0][j]:case["host"][0][j + 1]] for j in others])
    assert np.array_equal(got[2], want_rows)


def test_graph_capture_replays_with_refilled_inputs(case):
    from liso_amd.utils import graph_capture

    want = case["host"]
    capacity = int(want[0][-1]) + 100
    clouds, counts, lrows = dev(case["clouds"]), dev(case["counts"]), dev(case["lidar_rows"])
    jc, b7 = dev(case["job_cloud"]), dev(case["boxes7"])
    stream = torch.cuda.Stream()
    graph, res = graph_capture.capture(lambda: H.cut_box_snippets(clouds, counts, lrows, jc, b7, capacity=capacity), stream, warm_ups=1)
    torch.cuda.synchronize()
    # other inputs in the captured buffers: the sweeps swapped and the jobs re-aimed
    other = dict(case)
    other["clouds"] = np.ascontiguousarray(case["clouds"][[1, 0, 2]])
    other["lidar_rows"] = np.ascontiguousarray(case["lidar_rows"][[1, 0, 2]])
    other["counts"] = np.array([4097, 5000, 0], np.int32)
    other["job_cloud"] = np.where(case["job_cloud"] < 2, 1 - case["job_cloud"], 2).astype(np.int32)
    eager = host(device_cut(other, capacity=capacity))
    assert 0 < eager[0][-1] <= capacity
    clouds.copy_(dev(other["clouds"])), lrows.copy_(dev(other["lidar_rows"])), counts.copy_(dev(other["counts"])), jc.copy_(dev(other["job_cloud"]))
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        graph.replay()
    torch.cuda.synchronize()
    replayed = host(res)
    n = int(eager[0][-1])
    assert np.array_equal(replayed[0], eager[0]) and np.array_equal(replayed[3], eager[3])
    assert np.array_equal(replayed[1][:n].view(np.uint32), eager[1][:n].view(np.uint32)) and np.array_equal(replayed[2][:n], eager[2][:n])


@pytest.mark.parametrize("raydrop", [False, True])
def test_chain_device_database_equals_host_database(raydrop):
    """sweeps -> SnippetHarvester -> BoxSnippetDb -> BoxAugmenter: the device-resident database gives bitwise the sample that the
    database cut on the host and loaded through the constructor gives"""
    from liso_amd.datasets.box_augmentation import BoxAugmenter, BoxSnippetDb
    from liso_amd.datasets.torch_dataset_commons import voxelize_sample

    clouds, counts, lidar_rows, sensor, world = small_sequence()
    dbs = []
    for on_device in (True, False):
        h = H.SnippetHarvester(max_augm_db_size_mb=100)
        np.random.seed(6)
        if on_device:
            h.add_tracked_sequence(dev(clouds), dev(counts), dev(lidar_rows), sensor, world, min_track_age=2)
            assert torch.is_tensor(h.points) and h.points.is_cuda
            db = h.to_box_snippet_db()
            assert db.points.data_ptr() == h.points.data_ptr(), "from_device adopts the buffer"
        else:
            h.add_tracked_sequence(clouds, counts, lidar_rows, sensor, world, min_track_age=2)
            db = BoxSnippetDb(h.to_dict(stacked=True), DEV)
        assert len(db) >= 3
        dbs.append(db)
    assert np.array_equal(dbs[0].offsets, dbs[1].offsets) and torch.equal(dbs[0].points, dbs[1].points)
    box_cfg = {"max_num_objs": 4, "min_artificial_obj_velo": 1.0, "max_artificial_obj_velo": 3.0, "max_scale_delta": 0.2,
               "max_points_dropout": 0.25, "use_raydrop_augm": raydrop}
    rs = np.random.default_rng(9)
    pcl = dev(np.concatenate([rs.uniform(-5, 5, (200, 3)), rs.uniform(0, 1, (200, 1))], -1).astype(np.float32))
    sample = {"pcl_ta": {"pcl": pcl, "pillar_coors": voxelize_sample(pcl, (40.0, 40.0), (64, 64))[0]}, "pcl_full_w_ground_ta": pcl,
              "pcl_full_no_ground_ta": pcl, "gt": {}}
    outs = []
    for db in dbs:
        aug = BoxAugmenter(make_cfg(64, 40.0, box_cfg), db, need_flow=False)
        np.random.seed(3)
        torch.manual_seed(3)
        outs.append(aug.create_augmented_sample_from_box_snippet_db(0.1, sample))
    a, b = outs
    assert a["pcl_full_no_ground_ta"].shape[0] > 200
    for key in ("pcl_full_no_ground_ta", "pcl_full_w_ground_ta"):
        assert torch.equal(a[key].view(torch.int32), b[key].view(torch.int32)), key
    assert torch.equal(a["pcl_ta"]["pcl"].view(torch.int32), b["pcl_ta"]["pcl"].view(torch.int32))
    assert torch.equal(a["pcl_ta"]["pillar_coors"], b["pcl_ta"]["pillar_coors"])
    for k in ("pos", "dims", "rot", "probs", "velo"):
        assert torch.equal(getattr(a["gt"]["boxes"], k), getattr(b["gt"]["boxes"], k)), k
