"""GPU: JCP ground removal on the device (liso_amd/csrc/ground_jcp.hip) against the reference fixtures and, at full size, against
the numpy host path: every label identical.  fp64 device arithmetic in the reference's order differs from the host's by a few
ulp, so wherever the recorded decision margins are >= 1e-9 the labels must match bit for bit; the tests assert that condition
on the inputs they use and fail loudly (never skip) if a cloud violates it."""
import os

import numpy as np
import pytest
import torch

from liso_amd.jcp.jcp import JPCGroundRemove, jcp_device, jcp_host, remove_ground_points

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ground_seg_reference.npz")
KITTI = dict(range_img_width=2083, range_img_height=64, sensor_height=1.73, delta_R=1)
AV2 = dict(range_img_width=2000, range_img_height=64, sensor_height=1.8, delta_R=2)
DEV = torch.device("cuda:0")


def load_case(d, name):
    pcl = d["kitti_pcl"][d["shuffled_perm_of_kitti"]] if name == "shuffled" else d[f"{name}_pcl"]
    w, h, sh, dr = d[f"{name}_params"]
    return pcl, dict(range_img_width=int(w), range_img_height=int(h), sensor_height=float(sh), delta_R=float(dr))


def case_names():
    return [str(n) for n in np.load(GOLDEN)["names"]]


def to_dev(pcl64):
    p32 = pcl64.astype(np.float32)
    assert np.array_equal(p32.astype(np.float64), pcl64, equal_nan=True)  # the fixtures are float32 values stored as float64
    return torch.from_numpy(p32).to(DEV)


def full_cloud(seed):
    from liso_amd.datasets.synthetic import make_scene, render

    boxes, _, _ = make_scene(seed, DEV)
    return render(boxes, DEV, seed)[0].contiguous()  # [120000, 4] float32


def host_labels_checked(pcl_np, prm, what):
    labels, info = jcp_host(pcl_np, debug=True, **prm)
    print(f"{what}: candidates {info['candidates'].shape[0]}, exact ties {info['exact_ties']}, min nonzero margin "
          f"{info['min_nonzero_margin']:.3g}, min index distance {info['min_index_frac']:.3g}, ground {int(labels.sum())}")
    assert info["bad_ties"] == 0, f"{what}: an exact score tie that is not 0 vs 0 -- the comparison is not decided by the margin"
    assert info["min_nonzero_margin"] >= 1e-9 and info["min_index_frac"] >= 1e-9, \
        f"{what}: near-tie condition violated (margin {info['min_nonzero_margin']}, index distance {info['min_index_frac']})"
    return labels


@pytest.mark.parametrize("name", case_names())
def test_device_equals_reference_fixture(name):
    d = np.load(GOLDEN)
    pcl, prm = load_case(d, name)
    got = JPCGroundRemove(pcl=to_dev(pcl), **prm)
    assert got.dtype == torch.bool and got.is_cuda and got.shape == (pcl.shape[0],)
    got = got.cpu().numpy()
    want = d[f"{name}_labels"]
    print(name, "labels differing:", int((got != want).sum()), "of", want.size)
    assert np.array_equal(got, want)


def test_batched_call_equals_per_cloud_calls():
    d = np.load(GOLDEN)
    names = ["kitti", "shuffled", "nan_padded", "tilted"]  # one parameter set, four lengths
    clouds = [load_case(d, n)[0].astype(np.float32) for n in names]
    n_max = max(c.shape[0] for c in clouds) + 5
    batch = np.full((len(clouds), n_max, 3), np.nan, np.float32)
    for i, c in enumerate(clouds):
        batch[i, : c.shape[0]] = c
    got = JPCGroundRemove(pcl=torch.from_numpy(batch).to(DEV), **KITTI).cpu().numpy()
    # the same rows with explicit counts and finite garbage behind them
    counts = torch.tensor([c.shape[0] for c in clouds], dtype=torch.int32, device=DEV)
    junk = np.where(np.isnan(batch) & (np.arange(n_max)[None, :, None] >= counts.cpu().numpy()[:, None, None]), np.float32(7.5), batch)
    got_counts = jcp_device(torch.from_numpy(junk).to(DEV), counts=counts, **KITTI).cpu().numpy()
    for i, (n, c) in enumerate(zip(names, clouds)):
        single = JPCGroundRemove(pcl=torch.from_numpy(c).to(DEV), **KITTI).cpu().numpy()
        assert np.array_equal(single, d[f"{n}_labels"]), n
        assert np.array_equal(got[i, : c.shape[0]], single), n
        assert not got[i, c.shape[0]:].any(), n
        assert np.array_equal(got_counts[i], got[i]), n


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("params", ["kitti", "av2"])
def test_full_size_render_equals_host_path(seed, params):
    prm = KITTI if params == "kitti" else AV2
    cloud = full_cloud(seed)[:, :3].contiguous()
    assert cloud.shape == (120000, 3)
    want = host_labels_checked(cloud.cpu().numpy(), prm, f"seed {seed}, {params}")
    got = JPCGroundRemove(pcl=cloud, **prm).cpu().numpy()
    print(f"seed {seed}, {params}: labels differing {int((got != want).sum())} of {want.size}")
    assert np.array_equal(got, want)
    z = cloud[:, 2].cpu().numpy()
    assert want[z < -1.5].mean() > 0.9 and want[z > -1.2].mean() < 0.1  # it is a ground segmentation


def test_remove_ground_points_equals_host_selection():
    from liso_amd.datasets.torch_dataset_commons import infer_ground_label_using_cone

    # every 2nd / 3rd ray of a sweep (the render is ring-major); [N,4]: the intensity column travels along
    clouds = [full_cloud(0)[::2].contiguous(), full_cloud(1)[1::3].contiguous()]
    n_max = 60000
    batch = torch.full((2, n_max, 4), float("nan"), device=DEV)
    for i, c in enumerate(clouds):
        batch[i, : c.shape[0]] = c
    out, counts, is_ground = remove_ground_points(batch, **KITTI)
    assert out.shape == batch.shape and counts.dtype == torch.int32 and is_ground.dtype == torch.bool
    for i, c in enumerate(clouds):
        p = c.cpu().numpy()
        jcp = host_labels_checked(p[:, :3], KITTI, f"removal cloud {i}")
        cone = infer_ground_label_using_cone(p[:, :3].astype(np.float64))
        want = p[~(jcp | cone)]
        n = int(counts[i])
        print(f"removal cloud {i}: kept {n} of {p.shape[0]}, expected {want.shape[0]}")
        assert n == want.shape[0] and 0 < n < p.shape[0]
        assert np.array_equal(is_ground[i, : p.shape[0]].cpu().numpy(), jcp | cone)
        assert np.array_equal(out[i, :n].cpu().numpy(), want)
        assert torch.isnan(out[i, n:]).all()
    # JCP alone, one unbatched cloud
    out1, counts1, g1 = remove_ground_points(clouds[1], cone=None, **KITTI)
    jcp = jcp_host(clouds[1][:, :3].cpu().numpy(), **KITTI)
    assert int(counts1[0]) == int((~jcp).sum()) and np.array_equal(g1.cpu().numpy(), jcp)
    assert np.array_equal(out1[: int(counts1[0])].cpu().numpy(), clouds[1].cpu().numpy()[~jcp])


def test_graph_capture_and_replay_on_a_second_cloud():
    a, b = full_cloud(0)[:, :3].contiguous(), full_cloud(1)[:, :3].contiguous()
    want_a, want_b = (host_labels_checked(c.cpu().numpy(), KITTI, f"graph cloud {i}") for i, c in enumerate((a, b)))
    assert not np.array_equal(want_a, want_b)
    static = a.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        JPCGroundRemove(pcl=static, **KITTI)  # warm-up outside the capture: library load, LDS opt-in
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        labels = JPCGroundRemove(pcl=static, **KITTI)
        kept, counts, _ = remove_ground_points(static, cone=None, **KITTI)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(labels.cpu().numpy(), want_a)
    static.copy_(b)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(labels.cpu().numpy(), want_b)
    assert int(counts[0]) == int((~want_b).sum())
    assert np.array_equal(kept[: int(counts[0])].cpu().numpy(), b.cpu().numpy()[~want_b])


def test_guard_bands_stay_intact():
    from guarded_alloc import guarded

    d = np.load(GOLDEN)
    with guarded() as g:
        for name in ("nuscenes", "tilted"):
            pcl, prm = load_case(d, name)
            rows = np.concatenate([pcl.astype(np.float32), np.ones((pcl.shape[0], 1), np.float32)], -1)
            batch = torch.from_numpy(np.stack([rows, rows[::-1].copy()])).to(DEV)
            out, counts, is_ground = remove_ground_points(batch, **prm)
            assert g.check() >= 5  # labels, workspaces, output, counts
            assert np.array_equal(JPCGroundRemove(pcl=batch[0, :, :3].contiguous(), **prm).cpu().numpy(), d[f"{name}_labels"])
        # a label image too large for LDS takes the global-memory resolve
        big = dict(range_img_width=4096, range_img_height=64, sensor_height=1.73, delta_R=1)
        pcl = load_case(d, "kitti")[0]
        got = JPCGroundRemove(pcl=to_dev(pcl), **big)
        g.check()
    assert np.array_equal(got.cpu().numpy(), host_labels_checked(pcl, big, "4096x64 image"))
