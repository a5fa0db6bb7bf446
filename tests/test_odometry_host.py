"""CPU: the host restatement of the lidar odometry (liso_amd/odometry/host.py), piece by piece and on the world-fixed scene of
tests/odometry_scenes.py.

The two error bounds below were measured with the restatement itself on an x86-64 host (numpy, glibc) and carry a 3x margin for platform
libm differences:
  * self-registration (a sweep against a map of its own moved copy): pose distance 3.99e-9 m, largest entry difference 3.22e-9
  * trajectory "a": the estimated frame-to-frame motions are at most 0.153 m (pose distance at 30 m) from the truth, "b" 0.097 m
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.linalg
from scipy.spatial.transform import Rotation

import odometry_scenes as SC
from liso_amd.odometry import host as H
from liso_amd.odometry.config import KISSConfig, resolve_params

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SELF_REGISTRATION_BOUND = 3 * 3.99e-9
TRAJECTORY_BOUND = {"a": 3 * 0.153, "b": 3 * 0.097}
P = resolve_params(**SC.PARAMS)


# ---- pieces ------------------------------------------------------------------------------------------------------------------------
def test_voxel_down_sample_floors_and_keeps_the_first_comer_in_input_order():
    pts = np.array([[0.9, 0.1, 0.1],     # voxel (0, 0, 0)
                    [-0.1, 0.1, 0.1],    # voxel (-1, 0, 0): truncation would put it with the first
                    [0.2, 0.9, 0.5],     # (0, 0, 0) again: dropped
                    [-0.9, 0.5, 0.5],    # (-1, 0, 0) again: dropped
                    [-1.0, -1.0, -1.0],  # exactly on a boundary: voxel (-1, -1, -1)
                    [-1.0001, -0.5, -0.5],  # (-2, -1, -1)
                    [1.0, 0.0, 0.0],     # (1, 0, 0)
                    [-0.0, 0.5, 0.999]], np.float32)  # (0, 0, 0) again (-0.0 floors to 0)
    assert np.array_equal(H.voxel_keys(pts[[1, 4, 5]], 1.0), [[-1, 0, 0], [-1, -1, -1], [-2, -1, -1]])
    assert np.array_equal(H.voxel_down_sample(pts, 1.0), pts[[0, 1, 4, 5, 6]])
    assert np.array_equal(H.voxel_down_sample(pts[::-1], 1.0), pts[::-1][[0, 1, 2, 3, 4]])  # the first comer changes with the order
    assert np.array_equal(H.voxel_down_sample(pts, 4.0), pts[[0, 1, 4]])  # voxels (0, 0, 0), (-1, 0, 0), (-1, -1, -1)
    assert H.voxel_down_sample(pts[:0], 1.0).shape == (0, 3)
    # the key is floor(p / v) in fp64 of the fp32 value, not the fp32 quotient
    p = np.array([[np.float32(0.3) * 3, 0, 0]], np.float32)
    assert H.voxel_keys(p, 0.3)[0, 0] == int(np.floor(float(p[0, 0]) / 0.3))


def test_preprocess_keeps_finite_rows_strictly_inside_the_range_shell():
    pts = np.array([[3, 4, 0, 9], [0.5, 0.5, 0.5, 9], [np.nan, 1, 1, 9], [1, np.inf, 1, 9], [30, 0, 0, 9], [29.999, 0, 0, 9], [0, 0, 2, 9],
                    [0, -1, 0, 9], [0, 18, 24, 9]], np.float32)  # (norms 1 and 30 exactly: outside)
    assert np.array_equal(H.preprocess(pts, 1.0, 30.0), pts[[0, 5, 6], :3])


@pytest.mark.parametrize("dx", [[0.3, -0.2, 0.1, 0.02, -0.4, 0.7], [1.0, 2.0, 3.0, 0.0, 0.0, 0.0], [0.5, -0.5, 0.25, 3e-11, -2e-11, 1e-11],
                                [0.5, -0.5, 0.25, 3e-9, -2e-9, 1e-9], [0.1, 0.2, 0.3, 1e-5, 2e-5, -1e-5], [0.0, 0.0, 0.0, 0.0, 0.0, 3.0]])
def test_exp_se3_is_the_matrix_exponential_of_the_twist(dx):
    twist = np.zeros((4, 4))
    twist[:3, :3], twist[:3, 3] = H.hat(dx[3:]), dx[:3]
    assert np.allclose(H.exp_se3(np.array(dx)), scipy.linalg.expm(twist), rtol=0, atol=1e-14)


def test_solve_ldlt_solves_and_refuses():
    rng = np.random.default_rng(0)
    M = rng.standard_normal((6, 6))
    A, rhs = M @ M.T + 6 * np.eye(6), rng.standard_normal(6)
    assert np.allclose(H.solve_ldlt(A, rhs), np.linalg.solve(A, rhs), rtol=0, atol=1e-13)
    assert H.solve_ldlt(np.diag([1.0, 1.0, 0.0, 1.0, 1.0, 1.0]), rhs) is None
    assert H.solve_ldlt(-A, rhs) is None and H.solve_ldlt(np.full((6, 6), np.nan), rhs) is None


def test_correct_kitti_scan_rotates_about_the_horizontal_normal():
    rng = np.random.default_rng(1)
    pts = np.concatenate([rng.uniform(-50, 50, (200, 3)), [[0.0, 0.0, 2.5], [0.0, 0.0, -1.0], [3.0, 0.0, 0.0]]])
    got = H.correct_kitti_scan_host(pts)
    axis = np.cross(pts[:200], [0.0, 0.0, 1.0])
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    want = Rotation.from_rotvec(axis * np.deg2rad(0.205)).apply(pts[:200])
    assert np.allclose(got[:200], want, rtol=0, atol=1e-12)
    assert np.array_equal(got[200:202], pts[200:202])  # on the z axis: unchanged
    assert np.allclose(got[202], [3 * np.cos(np.deg2rad(0.205)), 0.0, 3 * np.sin(np.deg2rad(0.205))], rtol=0, atol=1e-14)
    from liso_amd.odometry import correct_kitti_scan

    assert np.array_equal(correct_kitti_scan(pts), got)


def test_threshold_arithmetic():
    shift = lambda x: np.array([[1, 0, 0, x], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]])  # noqa: E731
    assert H.threshold([], 0.0, 0, 2.0, 0.1) == 2.0
    assert H.threshold([shift(0.0), shift(0.4)], 0.32, 2, 2.0, 0.1) == 2.0    # moved 0.4 <= 5 * 0.1
    assert H.threshold([shift(0.0), shift(0.5)], 0.32, 2, 2.0, 0.1) == 2.0    # exactly 0.5: not more
    assert H.threshold([shift(0.0), shift(0.6)], 0.0, 0, 2.0, 0.1) == 2.0     # no model error yet
    assert H.threshold([shift(0.0), shift(0.6)], 0.32, 2, 2.0, 0.1) == np.sqrt(0.16) == 0.4
    assert H.threshold([shift(7.0), shift(7.3)], 0.32, 2, 2.0, 0.1) == 2.0    # the motion counts from the first pose, not the origin
    # the model error: a pure shift of 0.3 and a pure turn of 0.01 rad at 30 m
    assert H.model_error(shift(1.0), shift(1.3), 30.0) == pytest.approx(0.3, abs=1e-15)
    turn = H.exp_se3(np.array([0, 0, 0, 0, 0, 0.01]))
    assert H.model_error(np.eye(4), turn, 30.0) == pytest.approx(2 * 30.0 * np.sin(0.005), abs=1e-12)
    # and through a sequence: frame 1's error 0.3 > 0.1 is accumulated, sigma of frame 3 = sqrt(sse / n)
    odo = H.HostOdometry(**SC.PARAMS)
    odo.poses, odo.sse, odo.n_err = [shift(0.0), shift(0.3), shift(0.7)], 0.3 * 0.3 + 0.1 * 0.1, 2
    assert H.threshold(odo.poses, odo.sse, odo.n_err, 2.0, 0.1) == np.sqrt(0.05)
    assert np.allclose(odo.guess(), shift(1.1), rtol=0, atol=1e-15)  # constant velocity: 0.7 + (0.7 - 0.3)


def test_config_follows_the_builders_usage():
    kiss_config = KISSConfig()
    kiss_config.mapping.voxel_size = 0.01 * kiss_config.data.max_range  # create_kitti_raw.py:74-76
    assert kiss_config.params() == dict(max_range=100.0, min_range=5.0, deskew=False, voxel_size=1.0, max_points_per_voxel=20,
                                        initial_threshold=2.0, min_motion_th=0.1, max_num_iterations=500, convergence_criterion=1e-4)
    assert resolve_params()["voxel_size"] == 1.0 and resolve_params(max_range=30.0)["voxel_size"] == 0.3
    with pytest.raises(NotImplementedError):
        resolve_params(deskew=True)
    with pytest.raises(TypeError):
        resolve_params(voxel=1.0)
    with pytest.raises(ValueError):
        resolve_params(max_points_per_voxel=21)
    from liso_amd.odometry import KissICP

    odo = KissICP(config=kiss_config)
    assert odo.poses == []


# ---- the map -----------------------------------------------------------------------------------------------------------------------
def test_map_caps_voxels_keeps_order_removes_by_first_point_and_counts_overflow():
    m = H.VoxelMap(1.0, 3, 10.0, map_voxels=2)
    pts = np.array([[0.1, 0.1, 0.1], [0.2, 0.2, 0.2], [5.5, 0.5, 0.5], [0.3, 0.3, 0.3], [0.4, 0.4, 0.4], [-3.5, 0.5, 0.5], [5.6, 0.5, 0.5]], np.float32)
    m.update(pts, np.eye(4))
    assert m.overflow == 1 and len(m) == 2  # the third voxel found no slot; the fourth point of voxel 0 is dropped, not overflow
    k0, k5 = (int(H.pack_keys(np.array([k]))[0][0]) for k in ([0, 0, 0], [5, 0, 0]))
    assert np.array_equal(m.voxels[k0], pts[[0, 1, 3]]) and np.array_equal(m.voxels[k5], pts[[2, 6]])
    far = np.eye(4)
    far[0, 3] = -4.6  # 5.5 + 4.6 > 10: the voxel goes by its FIRST point, although the frame's own point lands in it
    m.update(np.array([[10.15, 0.5, 0.5]], np.float32), far)
    assert set(m.voxels) == {k0} and m.overflow == 1


# ---- registration ------------------------------------------------------------------------------------------------------------------
def _downsampled(path, f):
    clouds, counts, _ = SC.sequence(path)
    ds = H.voxel_down_sample(H.preprocess(clouds[f, :counts[f]], P["min_range"], P["max_range"]), 0.5 * P["voxel_size"])
    return ds, H.voxel_down_sample(ds, 1.5 * P["voxel_size"])


def test_registration_recovers_the_motion_of_a_clouds_own_copy():
    ds, src = _downsampled("a", 0)
    truth = H.exp_se3(np.array([0.3, -0.1, 0.02, 0.005, -0.003, np.deg2rad(2.0)]))
    m = H.VoxelMap(P["voxel_size"], 20, P["max_range"])
    m.update(ds, truth)
    T, it, conv = H.register(src, m, np.eye(4), 3 * 2.0, 2.0 / 3, 500, 1e-4)
    print("self-registration: iterations", it, "pose distance", SC.pose_distance(truth, T), "largest entry", np.abs(T - truth).max())
    assert conv == 1 and 1 < it < 50
    assert SC.pose_distance(truth, T) < SELF_REGISTRATION_BOUND
    # nothing to register against, and a source out of the map's reach: the guess comes back, not converged
    G = H.exp_se3(np.array([100.0, 0, 0, 0, 0, 0]))
    T, it, conv = H.register(src, m, G, 6.0, 2.0 / 3, 500, 1e-4)
    assert np.array_equal(T, G) and (it, conv) == (0, 0)
    T, it, conv = H.register(src[:0], m, np.eye(4), 6.0, 2.0 / 3, 500, 1e-4)
    assert np.array_equal(T, np.eye(4)) and (it, conv) == (0, 0)


@pytest.fixture(scope="module")
def runs():
    """the three trajectories, frame by frame, with what happened to the map on the way (computed once, read-only)"""
    out = {}
    for path in SC.PATHS:
        clouds, counts, truth = SC.sequence(path)
        odo, removed, full = H.HostOdometry(**SC.PARAMS), [], []
        for f in range(len(clouds)):
            before = set(odo.map.voxels)
            map_before = H.VoxelMap(P["voxel_size"], 20, P["max_range"])
            map_before.voxels = {k: list(c) for k, c in odo.map.voxels.items()}
            odo.step(clouds[f, :counts[f]])
            removed.append(len(before - set(odo.map.voxels)))
            full.append(sum(len(c) == 20 for c in odo.map.voxels.values()))
        out[path] = dict(odo=odo, removed=removed, full=full, truth=truth, map_before_last=map_before)
    return out


def test_every_path_of_the_pipeline_runs_on_the_fixture(runs):
    a = runs["a"]
    odo = a["odo"]
    assert SC.N_MAX < 6000 and (SC.sequence("a")[1] > 5000).all()
    assert a["full"][-1] >= 5, a["full"]                       # several voxels reached their 20-point cap
    assert sum(a["removed"]) >= 50, a["removed"]               # the map dropped voxels by range
    assert odo.sigma[:3] == [2.0, 2.0, 2.0] and all(s != 2.0 for s in odo.sigma[3:]), odo.sigma  # the threshold left its initial value
    assert odo.n_iterations[0] == 0 and all(1 < it < 500 for it in odo.n_iterations[1:]) and all(odo.converged), odo.n_iterations
    assert all(0 < n < d for n, d in zip(odo.n_source, [5400] * 6))
    # outliers met the robust weight: at the last frame's pose, against the map it was registered to, pairs are kept whose weight is
    # well below that of a perfect pair
    src = odo.source.astype(np.float64)
    q, d2 = H.nearest(a["map_before_last"].search_arrays(), H.transform_points(odo.poses[-1], src), P["voxel_size"])
    kept = np.sqrt(d2) < 3.0 * odo.sigma[-1]
    kappa = odo.sigma[-1] / 3.0
    weight = kappa ** 2 / (kappa + d2[kept]) ** 2  # 1 for a perfect pair
    # (a weight below 0.7 is a residual above sqrt(kappa (1 / sqrt(0.7) - 1)) = 0.31 m, thirty times the range noise: a moved box or
    # a surface seen for the first time, not a noisy inlier)
    assert kappa > 0.5 and kept.sum() > 1000 and (weight < 0.7).sum() >= 5, (kept.sum(), np.sort(weight)[:8])


@pytest.mark.parametrize("path", ["a", "b"])
def test_estimated_motion_beats_identity_and_constant_velocity(runs, path):
    est, truth = SC.relative(runs[path]["odo"].poses), SC.relative(list(runs[path]["truth"]))
    for n in range(len(est)):  # est[n]: the motion from frame n to frame n + 1
        d_est, d_identity = SC.pose_distance(truth[n], est[n]), SC.pose_distance(truth[n], np.eye(4))
        d_constant = SC.pose_distance(truth[n], est[n - 1]) if n >= 1 else np.inf
        print(f"{path}: frame {n + 1}: estimate {d_est:.4f} identity {d_identity:.4f} constant velocity {d_constant:.4f}")
        if n + 1 >= 2:  # from the third frame on
            assert d_est < d_identity and d_est < d_constant, (path, n + 1, d_est, d_identity, d_constant)
        assert d_est < TRAJECTORY_BOUND[path], (path, n + 1, d_est)


def test_sequences_are_padded_with_identity_and_independent(runs):
    clouds, counts, n_frames = SC.batch()
    res = H.lidar_odometry_host(clouds, counts, n_frames, **SC.PARAMS)
    assert list(n_frames) == [6, 4, 1]
    for s, path in enumerate(("a", "b", "c")):
        k, odo = n_frames[s], runs[path]["odo"]
        assert np.array_equal(res["poses"][s, :k], np.stack(odo.poses)) and np.array_equal(res["poses"][s, k:], np.tile(np.eye(4), (6 - k, 1, 1)))
        assert list(res["sigma"][s, :k]) == odo.sigma and (res["sigma"][s, k:] == 0).all()
        assert list(res["n_source"][s, :k]) == odo.n_source and list(res["n_iterations"][s, :k]) == odo.n_iterations
    assert (res["map_overflow"] == 0).all() and np.array_equal(res["poses"][:, 0], np.tile(np.eye(4), (3, 1, 1)))


def test_kiss_icp_interface_takes_numpy_sweeps(runs):
    from liso_amd.odometry import KissICP

    cfg = KISSConfig()
    cfg.data.max_range, cfg.data.min_range = SC.PARAMS["max_range"], SC.PARAMS["min_range"]
    odometry = KissICP(config=cfg)
    clouds, counts, _ = SC.sequence("b")
    for f in range(3):
        odometry.register_frame(clouds[f, :counts[f]].astype(np.float64), timestamps=np.zeros(counts[f]))
    w_Ts_si = odometry.poses
    assert len(w_Ts_si) == 3 and all(np.array_equal(a, b) for a, b in zip(w_Ts_si, runs["b"]["odo"].poses[:3]))
    assert np.linalg.inv(w_Ts_si[0]) @ w_Ts_si[1] == pytest.approx(w_Ts_si[1])


def test_install_as_registers_kiss_icp_only_when_there_is_none(tmp_path):
    code = ("import liso_amd\nliso_amd.install_as('liso')\nfrom kiss_icp.config import KISSConfig\nfrom kiss_icp.kiss_icp import KissICP\n"
            "import liso_amd.odometry as O\nassert KISSConfig is O.KISSConfig and KissICP is O.KissICP\n"
            "from liso.odometry import lidar_odometry\nliso_amd.install_as('liso')\nprint('KISS_OK')\n")
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=str(tmp_path), timeout=300)
    assert r.returncode == 0 and "KISS_OK" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
    (tmp_path / "kiss_icp").mkdir()
    (tmp_path / "kiss_icp" / "__init__.py").write_text("REAL = 1\n")
    code = "import liso_amd\nliso_amd.install_as('liso')\nimport kiss_icp\nassert kiss_icp.REAL == 1\nprint('REAL_KEPT')\n"
    env = dict(os.environ, PYTHONPATH=str(tmp_path) + os.pathsep + ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=str(tmp_path), timeout=300)
    assert r.returncode == 0 and "REAL_KEPT" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
