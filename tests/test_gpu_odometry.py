"""Lidar odometry on the device (include/liso_odometry.h; liso_amd/odometry) against the host restatement, on the world-fixed scene
of tests/odometry_scenes.py.

1. preprocess + downsample: point set and order bit-equal to the host, with an all-NaN tail, an empty frame, a frame out of range
2. map update with given poses over 4 frames: per voxel the stored points and their order bit-equal, with room and overflowing
3. registration with given map, guess and sigma: iteration counts equal, poses within the measured tolerance
4. end to end, S = 3 of lengths 6, 4, 1: padded frames identity, a sequence alone bit-equal to itself in the batch, against the host
5. a captured replay equals the eager call bit for bit, twice
6. KissICP on CUDA tensors equals lidar_odometry with S = 1; odom(i, j); the KITTI correction

The pose tolerance is measured, not chosen: the host restatement registers the fixture of (3) once with A and b accumulated first to
last and once last to first; 100 x the largest difference of a pose entry (the margin covers the compounding over iterations, the
device's reduction tree) is the bound, and it has to stay below 1e-8 for the comparison to mean anything.  Measured on a CPU-only
x86-64 host: largest difference 6.2e-16, bound 6.2e-14; on the host of an MI355X 1.5e-15, bound 1.5e-13; the device is 1.4e-15 from
the first-to-last registration and, end to end against the restatement in its canonical order (the kernel's), 0.0.
"""
import functools

import numpy as np
import pytest
import torch

import odometry_scenes as SC
from guarded_alloc import guarded
from liso_amd.odometry import host as H
from liso_amd.odometry.config import resolve_params

pytestmark = pytest.mark.gpu
P = resolve_params(**SC.PARAMS)
MAP_VOXELS = 1 << 14
EYE = np.eye(4)


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()  # (a copy: the scenes' arrays are read-only)


def _workspace(S, F, C=3, map_voxels=MAP_VOXELS):
    from liso_amd.odometry import OdometryWorkspace

    return OdometryWorkspace(S, F, SC.N_MAX, C, "cuda", map_voxels=map_voxels, **SC.PARAMS)


def _host_downsampled(sweep):
    ds = H.voxel_down_sample(H.preprocess(sweep, P["min_range"], P["max_range"]), 0.5 * P["voxel_size"])
    return ds, H.voxel_down_sample(ds, 1.5 * P["voxel_size"])


# ---- 1 -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [3, 4])
def test_preprocess_and_downsample_equal_the_host_bit_for_bit(C):
    clouds_a, counts_a, _ = SC.sequence("a")
    S, F, N = 4, 2, SC.N_MAX
    clouds, counts = np.full((S, F, N, C), np.nan, np.float32), np.zeros((S, F), np.int32)
    rng = np.random.default_rng(5)
    clouds[..., 3:] = 7.0
    clouds[0, 1, :, :3], counts[0, 1] = clouds_a[1], N            # the sweep, then an all-NaN tail inside the count
    clouds[1, 1, :, :3], counts[1, 1] = clouds_a[2], 0            # an empty frame (garbage behind the count)
    far = clouds_a[3].copy()
    far[:counts_a[3] // 2] *= np.float32(40.0)                     # beyond max_range
    far[counts_a[3] // 2:] *= np.float32(0.01)                     # inside min_range
    clouds[2, 1, :, :3], counts[2, 1] = far, counts_a[3]          # a frame entirely out of range
    shuffled = clouds_a[4][rng.permutation(counts_a[4])]
    shuffled[::97] = np.inf
    clouds[3, 1, :counts_a[4], :3], counts[3, 1] = shuffled, counts_a[4] - 100  # another order, infinities, a count that cuts
    clouds[:, 0, :, :3] = clouds_a[0]                             # frame 0 must not be looked at
    counts[:, 0] = N
    n_frames = np.full(S, F, np.int32)
    with guarded():
        ws = _workspace(S, F, C)
        ws.preprocess(1, _dev(clouds), _dev(counts), _dev(n_frames))
        n_source = ws.n_source.cpu().numpy()
        got = [(ws.frame_ds(s), ws.source(s)) for s in range(S)]
    for s in range(S):
        ds, src = _host_downsampled(clouds[s, 1, :counts[s, 1]])
        assert got[s][0].tobytes() == ds.tobytes() and got[s][1].tobytes() == src.tobytes(), s
        assert n_source[s, 1] == len(src) and n_source[s, 0] == 0
    assert len(got[0][1]) > 2000 and len(got[3][0]) > 4000 and len(got[1][0]) == 0 and len(got[2][0]) == 0


# ---- 2 -------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _given_pose_fixture():
    """two sequences of four frames with the true poses relative to their first frame"""
    seqs = [SC.sequence("a"), SC.sequence("b")]
    clouds = np.stack([c[:4] for c, _, _ in seqs])
    counts = np.stack([n[:4] for _, n, _ in seqs])
    poses = np.stack([[np.linalg.inv(t[0]) @ t[f] for f in range(4)] for _, _, t in seqs])
    return clouds, counts, poses


@pytest.mark.parametrize("map_voxels,overflows", [(MAP_VOXELS, False), (4096, True)])
def test_map_update_keeps_the_hosts_points_in_the_hosts_order(map_voxels, overflows):
    clouds, counts, poses = _given_pose_fixture()
    S, F = clouds.shape[:2]
    n_frames = np.full(S, F, np.int32)
    hosts = [H.VoxelMap(P["voxel_size"], 20, P["max_range"], map_voxels) for _ in range(S)]
    d_clouds, d_counts, d_frames, d_poses = _dev(clouds), _dev(counts), _dev(n_frames), _dev(poses)
    with guarded() as g:
        ws = _workspace(S, F, map_voxels=map_voxels)
        for f in range(F):
            ws.preprocess(f, d_clouds, d_counts, d_frames)
            ws.map_update(f, d_frames, d_poses)
            g.check()
            overflow = ws.map_overflow.cpu().numpy()
            for s in range(S):
                hosts[s].update(_host_downsampled(clouds[s, f, :counts[s, f]])[0], poses[s, f])
                got, want = ws.map_voxels_of(s, f), hosts[s].voxels
                assert set(got) == set(want), (f, s, len(got), len(want))
                for key, cell in want.items():
                    assert got[key].tobytes() == np.asarray(cell, np.float32).tobytes(), (f, s, key)
                assert overflow[s] == hosts[s].overflow and int(ws.table("n_map_voxels")[s]) == len(want), (f, s, overflow, hosts[s].overflow)
    full = [sum(len(c) == 20 for c in h.voxels.values()) for h in hosts]
    if overflows:
        assert all(h.overflow > 1000 for h in hosts), [h.overflow for h in hosts]
    else:
        assert all(h.overflow == 0 for h in hosts) and full[0] >= 1, full


# ---- 3 -------------------------------------------------------------------------------------------------------------------------------
REGISTER_CASES = ((1, 2.0), (2, 2.0), (1, 1.0))  # (frame of trajectory "a" registered against the map of frame 0, sigma)


@functools.lru_cache(maxsize=None)
def _register_reference():
    """the host's registrations of REGISTER_CASES, forward and reversed -> (poses forward [3,4,4], iterations, converged, tolerance)"""
    clouds, counts, _ = SC.sequence("a")
    res = {}
    for order in ("forward", "reversed"):
        rows = []
        for frame, sigma in REGISTER_CASES:
            m = H.VoxelMap(P["voxel_size"], 20, P["max_range"], MAP_VOXELS)
            m.update(_host_downsampled(clouds[0, :counts[0]])[0], EYE)
            info = {}
            T, it, conv = H.register(_host_downsampled(clouds[frame, :counts[frame]])[1], m, EYE, 3.0 * sigma, sigma / 3.0,
                                     P["max_num_iterations"], P["convergence_criterion"], order, info)
            # a stop that straddles the criterion could pass as agreement, or fail as disagreement, by luck
            assert abs(info["last_step"] - P["convergence_criterion"]) > 0.01 * P["convergence_criterion"], (frame, sigma, info)
            rows.append((T, it, conv))
        res[order] = rows
    fwd, rev = res["forward"], res["reversed"]
    assert [r[1:] for r in fwd] == [r[1:] for r in rev]
    spread = max(np.abs(a[0] - b[0]).max() for a, b in zip(fwd, rev))
    tol = 100.0 * spread
    print("registration: forward against reversed", spread, "-> tolerance", tol)
    assert 0.0 < tol < 1e-8, tol
    return np.stack([r[0] for r in fwd]), [r[1] for r in fwd], [r[2] for r in fwd], tol


def test_registration_with_given_map_guess_and_sigma_equals_the_host():
    want, want_it, want_conv, tol = _register_reference()
    clouds_a, counts_a, _ = SC.sequence("a")
    S = len(REGISTER_CASES)
    clouds = np.stack([np.stack([clouds_a[0], clouds_a[frame]]) for frame, _ in REGISTER_CASES])
    counts = np.stack([[counts_a[0], counts_a[frame]] for frame, _ in REGISTER_CASES]).astype(np.int32)
    d_clouds, d_counts, d_frames = _dev(clouds), _dev(counts), _dev(np.full(S, 2, np.int32))
    guess, sigma = _dev(np.tile(EYE, (S, 1, 1))), _dev(np.array([s for _, s in REGISTER_CASES]))
    with guarded():
        ws = _workspace(S, 2)
        ws.preprocess(0, d_clouds, d_counts, d_frames)
        ws.map_update(0, d_frames)  # (the object's poses are identities)
        ws.preprocess(1, d_clouds, d_counts, d_frames)
        ws.register(1, d_frames, guess, sigma)
        poses, it, conv, sig = (t.cpu().numpy() for t in (ws.poses, ws.n_iterations, ws.converged, ws.sigma))
        assert float(ws.table("sse").abs().sum()) == 0.0 and int(ws.table("n_err").sum()) == 0  # given guesses leave the sums alone
    print("registration: device against host", np.abs(poses[:, 1] - want).max(), "tolerance", tol, "iterations", it[:, 1], want_it)
    assert list(it[:, 1]) == want_it and list(conv[:, 1]) == want_conv == [1, 1, 1]
    assert list(sig[:, 1]) == [s for _, s in REGISTER_CASES]
    assert np.abs(poses[:, 1] - want).max() <= tol, (np.abs(poses[:, 1] - want).max(), tol)
    assert np.array_equal(poses[:, 0], np.tile(EYE, (S, 1, 1)))


# ---- 4 -------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _host_batch():
    return H.lidar_odometry_host(*SC.batch(), map_voxels=MAP_VOXELS, **SC.PARAMS)


def _fields(r):
    return {k: getattr(r, k).cpu().numpy() for k in ("poses", "sigma", "n_source", "n_iterations", "converged", "map_overflow")}


@functools.lru_cache(maxsize=None)
def _device_batch():
    from liso_amd.odometry import lidar_odometry

    with guarded():
        return _fields(lidar_odometry(*[_dev(a) for a in SC.batch()], map_voxels=MAP_VOXELS, **SC.PARAMS))


def test_sequences_end_to_end_against_the_host():
    got, want = _device_batch(), _host_batch()
    tol = _register_reference()[3] * 6  # (the registration's measured tolerance, scaled by the frame count)
    print("end to end: device against host", np.abs(got["poses"] - want["poses"]).max(), "tolerance", tol)
    for k in ("n_source", "n_iterations", "converged", "map_overflow"):
        assert np.array_equal(got[k], want[k]), (k, got[k], want[k])
    assert np.abs(got["poses"] - want["poses"]).max() <= tol
    pad = np.arange(6)[None, :] >= SC.batch()[2][:, None]
    assert pad.sum() == 7 and np.array_equal(got["poses"][pad], np.tile(EYE, (7, 1, 1))) and (got["sigma"][pad] == 0).all()
    assert np.array_equal(got["poses"][:, 0], np.tile(EYE, (3, 1, 1))) and (got["n_iterations"][~pad][3:] > 1).any()


def test_sigma_equals_the_hosts():
    """The threshold of every frame, equal to the host's to the bit: sigma is sqrt(sse / n) of model errors computed from the poses,
    and host and device form the poses with the same correctly rounded operations in the same order."""
    got, want = _device_batch(), _host_batch()
    print("sigma: device against host, largest difference", np.abs(got["sigma"] - want["sigma"]).max())
    assert np.array_equal(got["sigma"], want["sigma"]), (got["sigma"], want["sigma"])


@pytest.mark.parametrize("s,path", [(0, "a"), (1, "b"), (2, "c")])
def test_a_sequence_alone_equals_itself_in_the_batch(s, path):
    from liso_amd.odometry import lidar_odometry

    clouds, counts, _ = SC.sequence(path)
    k = len(clouds)
    with guarded():
        alone = _fields(lidar_odometry(_dev(clouds[None]), _dev(counts[None]), _dev(np.array([k], np.int32)), map_voxels=MAP_VOXELS, **SC.PARAMS))
    batch = _device_batch()
    for key in ("poses", "sigma", "n_source", "n_iterations", "converged"):
        assert alone[key][0].tobytes() == batch[key][s, :k].tobytes(), (path, key)
    assert alone["map_overflow"][0] == batch["map_overflow"][s] == 0


# ---- 5 -------------------------------------------------------------------------------------------------------------------------------
def test_a_captured_replay_equals_the_eager_call_twice():
    from liso_amd.odometry import lidar_odometry
    from liso_amd.utils.graph_capture import capture

    args = [_dev(a) for a in SC.batch(("b", "c"))]
    body = lambda: lidar_odometry(*args, map_voxels=MAP_VOXELS, **SC.PARAMS)  # noqa: E731
    eager = _fields(body())
    stream = torch.cuda.Stream()
    graph, static = capture(body, stream, warm_ups=1)
    for _ in range(2):
        for t in (static.poses, static.sigma, static.n_source, static.n_iterations, static.converged, static.map_overflow):
            t.fill_(3)  # the call resets its results and its state itself
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            graph.replay()
        torch.cuda.synchronize()
        replay = _fields(static)
        for key in eager:
            assert replay[key].tobytes() == eager[key].tobytes(), key
    assert (eager["n_iterations"][0, 1:4] > 1).all()


# ---- 6 -------------------------------------------------------------------------------------------------------------------------------
def test_kiss_icp_on_cuda_tensors_equals_the_batched_call_and_odom_is_inv_matmul():
    from liso_amd.odometry import KISSConfig, KissICP, LidarOdometry, lidar_odometry

    cfg = KISSConfig()
    cfg.data.max_range, cfg.data.min_range = SC.PARAMS["max_range"], SC.PARAMS["min_range"]
    clouds, counts, _ = SC.sequence("b")
    with guarded():
        odometry = KissICP(config=cfg, max_points=SC.N_MAX, map_voxels=MAP_VOXELS)
        for f in range(len(clouds)):
            odometry.register_frame(_dev(clouds[f, :counts[f]]).double())  # (the builders hand float64 sweeps)
        got = {k: v.cpu().numpy() for k, v in odometry.device_result().items()}
        poses = odometry.poses
    batch = _device_batch()
    for key in ("poses", "sigma", "n_source", "n_iterations", "converged"):
        assert got[key][0].tobytes() == batch[key][1, :4].tobytes(), key
    assert len(poses) == 4 and all(np.array_equal(p, q) for p, q in zip(poses, batch["poses"][1]))
    r = LidarOdometry(*[_dev(batch[k]) for k in ("poses", "sigma", "n_source", "n_iterations", "converged", "map_overflow")], _dev(SC.batch()[2]))
    for i, j in ((0, 1), (1, 3), (3, 1), (2, 2), (0, 5)):
        want = np.stack([np.linalg.inv(batch["poses"][s, i]) @ batch["poses"][s, j] for s in range(3)])
        assert np.abs(r.odom(i, j).cpu().numpy() - want).max() <= 1e-13, (i, j)
    keys = r.kiss_odom_keys(1)
    assert sorted(keys) == ["kiss_odom_t0_t1", "kiss_odom_t0_t2", "kiss_odom_t1_t0", "kiss_odom_t1_t2", "kiss_odom_t2_t0", "kiss_odom_t2_t1"]
    assert np.array_equal(keys["kiss_odom_t0_t2"].cpu().numpy(), r.odom(1, 3).cpu().numpy())
    assert np.abs((keys["kiss_odom_t1_t2"] @ keys["kiss_odom_t2_t1"]).cpu().numpy() - EYE).max() <= 1e-13
    world = r.world_poses()
    assert np.array_equal(world.w_T_sensor.cpu().numpy(), batch["poses"]) and np.array_equal(world.odom[:, 2].cpu().numpy(), r.odom(2, 3).cpu().numpy())
    assert np.array_equal(world.odom[:, 5].cpu().numpy(), np.tile(EYE, (3, 1, 1)))


def test_kitti_correction_on_the_device_equals_the_host():
    from liso_amd.odometry import correct_kitti_scan

    rng = np.random.default_rng(2)
    pts = np.concatenate([rng.uniform(-60, 60, (5000, 3)), [[0.0, 0.0, 2.0], [0.0, 0.0, -3.0], [1e-9, 0.0, 1.0]]])
    with guarded():
        got = correct_kitti_scan(_dev(pts))
        assert isinstance(got, torch.Tensor) and got.is_cuda
        got = got.cpu().numpy()
    assert np.abs(got - H.correct_kitti_scan_host(pts)).max() <= 1e-13 and np.array_equal(got[5000:5002], pts[5000:5002])
