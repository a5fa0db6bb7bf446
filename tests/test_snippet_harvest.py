"""CPU: the box-snippet harvest (liso_amd/tracker/snippet_harvest.py, include/liso_snippets.h) -- the numpy host path, the draws,
the size cap and the tracking mirrors against tests/golden/snippet_harvest_reference.npz (made by the reference's python, see
tests/golden/make_snippet_harvest_golden.py), the exact boundary of the inside test, the file round trip, and the argument checks
of the C entry point.  tests/test_gpu_snippet_harvest.py runs the same checks on the device and shares the helpers below."""
import ctypes
import os

import numpy as np
import pytest
import torch

from liso_amd.kabsch.shape_utils import Shape
from liso_amd.tracker import snippet_harvest as H

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "snippet_harvest_reference.npz"))
EINVAL, EWORKSPACE = -1, -2


# ---- helpers shared with the device tests ------------------------------------------------------------------------------------------
def ulp_distance(a, b):
    """distance in representable float32 values"""
    def key(v):
        i = np.ascontiguousarray(v, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


def fixture_boxes():
    return Shape(**{k: torch.from_numpy(G[f"cut_{k}"]) for k in ("pos", "dims", "rot", "probs")})


def check_against(got, want_offsets, want_points, want_rows, want_T, what, T_rtol):
    """membership, order and rows identical; coordinates within 1 float32 ulp, intensity untouched; box_T_sensor within T_rtol"""
    offsets, points, rows, box_T = got
    assert offsets.dtype == np.int64 and np.array_equal(offsets, want_offsets), (what, offsets, want_offsets)
    assert points.dtype == np.float32 and points.shape == want_points.shape, (what, points.shape, want_points.shape)
    assert rows.dtype == np.int32 and np.array_equal(rows, want_rows), what  # the LiDAR rows identify the points and their order
    assert np.array_equal(points[:, 3].view(np.uint32), want_points[:, 3].view(np.uint32)), what
    d = ulp_distance(points[:, :3], want_points[:, :3])
    equal = float(np.mean(d == 0)) if d.size else 1.0
    print(f"{what}: {d.size} coordinates, bit-equal share {equal:.6f}, max distance {int(d.max()) if d.size else 0} ulp")
    assert d.size == 0 or d.max() <= 1, f"{what}: max {int(d.max())} ulp, bit-equal share {equal:.6f}"
    scale = np.abs(want_T).max(axis=(1, 2), keepdims=True)
    err = float((np.abs(box_T - want_T) / scale).max())
    print(f"{what}: box_T_sensor max relative error {err:.3e}")
    assert box_T.dtype == np.float64 and err <= T_rtol, (what, err)


def random_case(seed=4):
    """T = 3 sweeps of n_max = 5000 rows with counts (5000, 4097, 0), NaN rows sprinkled in; J = 9 jobs out of cloud order: jobs 0
    and 2 cut sweep 1 with overlapping boxes, job 8's box holds nothing, job 3 names the empty sweep, yaws spread over (-pi, pi).
    Points within 1e-4 m of a bloated box face (fp64, host) are removed (made NaN rows) -> also returns their share."""
    g = np.random.default_rng(seed)
    T, N = 3, 5000
    counts = np.array([5000, 4097, 0], np.int32)
    job_cloud = np.array([1, 0, 1, 2, 0, 1, 0, 1, 0], np.int32)
    pos = np.concatenate([g.uniform(-30, 30, (9, 2)), g.uniform(-1.2, -0.6, (9, 1))], -1).astype(np.float32)
    pos[2] = pos[0] + np.array([0.8, -0.5, 0.1], np.float32)
    pos[8, 2] = 15.0
    dims = np.stack([g.uniform(3.5, 5.0, 9), g.uniform(1.6, 2.2, 9), g.uniform(1.4, 1.9, 9)], -1).astype(np.float32)
    rot = (np.linspace(-3.1, 3.1, 9)[g.permutation(9)]).astype(np.float32)[:, None]
    b7 = np.concatenate([pos, dims, rot], -1)
    clouds = np.concatenate([g.uniform(-35, 35, (T, N, 2)), g.uniform(-3, 2, (T, N, 1)), g.uniform(0, 255, (T, N, 1))], -1).astype(np.float32)
    for j in range(9):  # 200 points in and around every box, spread over its sweep
        t = int(job_cloud[j])
        if counts[t] == 0 or j == 8:
            continue
        local = g.uniform(-0.7, 0.7, (200, 3)) * dims[j]
        c, s = np.cos(rot[j, 0]), np.sin(rot[j, 0])
        at = g.choice(int(counts[t]), 200, replace=False)
        clouds[t, at, 0] = pos[j, 0] + c * local[:, 0] - s * local[:, 1]
        clouds[t, at, 1] = pos[j, 1] + s * local[:, 0] + c * local[:, 1]
        clouds[t, at, 2] = pos[j, 2] + local[:, 2]
    M = H.box_T_sensor_host(b7)
    near = np.zeros((T, N), bool)
    for j in range(9):
        p = np.concatenate([clouds[..., :3].astype(np.float64), np.ones((T, N, 1))], -1)
        q = np.einsum("rc,tnc->tnr", M[j, :3], p)
        near |= (np.abs(np.abs(q) - (H.BLOAT_HALF * dims[j]).astype(np.float64)) < 1e-4).any(-1)
    removed = float(near.mean())
    clouds[near, :3] = np.nan
    clouds[g.uniform(size=(T, N)) < 0.01, g.integers(0, 3)] = np.nan  # the sprinkled NaN rows
    lidar_rows = g.integers(0, 64, (T, N)).astype(np.int32)
    return dict(clouds=clouds, counts=counts, lidar_rows=lidar_rows, job_cloud=job_cloud, boxes7=b7, removed=removed)


def boundary_case():
    """box at the origin, yaw 0, dims (2, 2, 2): the bound is exactly float32(1.1) = 2 * float32(0.55); rows 0, 2, 4 are inside"""
    e = np.float32(1.1)
    out = np.nextafter(e, np.float32(np.inf))
    xyz = np.array([[e, 0, 0], [out, 0, 0], [0, -e, 0], [0, -out, 0], [e, e, -e], [0, 0, out]], np.float32)
    clouds = np.concatenate([xyz, np.arange(6, dtype=np.float32)[:, None]], -1)[None]
    b7 = np.array([[0, 0, 0, 2, 2, 2, 0]], np.float32)
    assert np.float32(2) * H.BLOAT_HALF == e
    return clouds, np.arange(6, dtype=np.int32)[None], np.zeros(1, np.int32), b7, np.array([0, 2, 4], np.int32)


def small_sequence(seed=2):
    """4 sweeps of 3000 points, 3 tracks with refined boxes in sensor and world coordinates (the world is the sensor shifted)"""
    g = np.random.default_rng(seed)
    T, N = 4, 3000
    clouds = np.concatenate([g.uniform(-20, 20, (T, N, 2)), g.uniform(-2.5, 1, (T, N, 1)), g.uniform(0, 255, (T, N, 1))], -1).astype(np.float32)
    counts = np.array([3000, 2900, 3000, 2500], np.int32)
    sensor, world = {}, {}
    for track_id, (start, length, speed) in enumerate([(0, 4, 2.5), (1, 3, 0.2), (2, 2, 6.0)]):
        x0, y0, yaw = g.uniform(-10, 10), g.uniform(-10, 10), g.uniform(-3, 3)
        dims = np.tile(np.array([g.uniform(3.5, 4.8), g.uniform(1.7, 2.1), g.uniform(1.4, 1.8)], np.float32), (length, 1))
        pos = np.stack([x0 + speed * np.arange(length) * np.cos(yaw), y0 + speed * np.arange(length) * np.sin(yaw), np.full(length, -0.9)], -1).astype(np.float32)
        rot = np.full((length, 1), yaw, np.float32)
        for k in range(length):  # 120 returns on the object in every frame of the track
            local = g.uniform(-0.5, 0.5, (120, 3)) * dims[k]
            at = g.choice(int(counts[start + k]), 120, replace=False)
            clouds[start + k, at, 0] = pos[k, 0] + np.cos(yaw) * local[:, 0] - np.sin(yaw) * local[:, 1]
            clouds[start + k, at, 1] = pos[k, 1] + np.sin(yaw) * local[:, 0] + np.cos(yaw) * local[:, 1]
            clouds[start + k, at, 2] = pos[k, 2] + local[:, 2]
        mk = lambda p: Shape(pos=torch.from_numpy(p.copy()), dims=torch.from_numpy(dims.copy()), rot=torch.from_numpy(rot.copy()),  # noqa: E731
                             probs=torch.full((length, 1), 0.5 + 0.1 * track_id))
        sensor[(track_id, start)], world[(track_id, start)] = mk(pos), mk(pos + np.array([100.0, -50.0, 0.0], np.float32))
    lidar_rows = g.integers(0, 64, (T, N)).astype(np.int32)
    return clouds, counts, lidar_rows, sensor, world


# ---- the host path ----------------------------------------------------------------------------------------------------------------
def test_host_path_matches_reference():
    got = H.cut_box_snippets_host(G["cut_clouds"], G["cut_counts"], G["cut_lidar_rows"], G["cut_job_cloud"], fixture_boxes())
    check_against(got, G["cut_offsets"], G["cut_points"], G["cut_rows"], G["cut_box_T_sensor"], "host vs reference", 1e-12)


def test_host_path_exact_boundary():
    clouds, rows, job_cloud, b7, inside = boundary_case()
    offsets, points, got_rows, _ = H.cut_box_snippets_host(clouds, None, rows, job_cloud, b7)
    assert offsets.tolist() == [0, 3] and np.array_equal(got_rows, inside)
    assert np.array_equal(points, clouds[0, inside])  # the identity pose: coordinates and intensity come through untouched


def test_random_case_margin_and_structure():
    """the seeded case of the device test: the margin removes at most 1 % of the points, and the case has what it is meant to have"""
    c = random_case()
    assert c["removed"] <= 0.01, c["removed"]
    offsets, points, rows, _ = H.cut_box_snippets_host(c["clouds"], c["counts"], c["lidar_rows"], c["job_cloud"], c["boxes7"])
    sizes = np.diff(offsets)
    print("random case: removed share", c["removed"], "sizes", sizes.tolist())
    assert sizes[3] == 0 and sizes[8] == 0 and (np.delete(sizes, [3, 8]) > 50).all(), sizes
    a = set(points[offsets[0]:offsets[1], 3].tolist()) & set(points[offsets[2]:offsets[3], 3].tolist())
    assert len(a) > 10, "jobs 0 and 2 are meant to share points"
    assert np.isnan(c["clouds"][..., :3]).any(-1).sum() > 50
    short = H.cut_box_snippets_host(c["clouds"], c["counts"], c["lidar_rows"], c["job_cloud"], c["boxes7"], capacity=100)
    assert np.array_equal(short[0], offsets) and np.array_equal(short[1], points[:100]) and np.array_equal(short[2], rows[:100])


# ---- draws, size cap, mirrors --------------------------------------------------------------------------------------------------------
def test_seeded_draws_match_reference():
    np.random.seed(int(G["draw_track_seed"]))
    picks = [H.draw_track_snippet_times(int(l), int(s), d, int(a)) for l, s, d, a in G["draw_tracks"]]
    assert [len(p) for p in picks] == G["draw_track_sizes"].tolist()
    assert np.array_equal(np.concatenate(picks), G["draw_track_picks"])
    off = np.concatenate([[0], np.cumsum(G["draw_box_sizes"])])
    np.random.seed(int(G["draw_box_seed"]))
    idxs = [H.draw_untracked_box_idxs(G["draw_box_probs"][off[i]:off[i + 1]]) for i in range(len(off) - 1)]
    assert np.array_equal(np.concatenate(idxs), G["draw_box_picks"])
    assert all(len(i) == min(3, n) for i, n in zip(idxs, G["draw_box_sizes"]))


def test_size_cap_matches_reference():
    sizes, probs = G["cap_sizes"], G["cap_probs"]
    h = H.SnippetHarvester(float(G["cap_max_mb"]))
    h.points = np.arange(int(sizes.sum()) * 4, dtype=np.float32).reshape(-1, 4)
    h.rows = np.arange(int(sizes.sum()), dtype=np.int32)
    h.box_T_sensor = np.tile(np.eye(4), (len(sizes), 1, 1)) * np.arange(1, len(sizes) + 1)[:, None, None]
    h.counts = sizes.astype(np.int64)
    h.boxes = [H._host_box(Shape(pos=torch.zeros(3), dims=torch.ones(3), rot=torch.zeros(1), probs=torch.tensor([p]))) for p in probs]
    h.unique_track_id = list(range(len(sizes)))
    before, off = h.points.copy(), h.offsets
    np.random.seed(int(G["cap_seed"]))
    h._apply_size_cap()
    keep = G["cap_keep"]
    assert h.unique_track_id == keep.tolist() and np.array_equal(h.counts, sizes[keep])
    assert np.array_equal(h.points, np.concatenate([before[off[i]:off[i + 1]] for i in keep]))
    assert np.array_equal(h.rows, np.concatenate([np.arange(off[i], off[i + 1]) for i in keep]))
    assert np.array_equal(h.box_T_sensor[:, 0, 0], keep + 1.0)
    assert [float(b.probs) for b in h.boxes] == [float(probs[i]) for i in keep] and h.size_mb() <= float(G["cap_max_mb"])


def _seq(prefix):
    return Shape(**{k: torch.from_numpy(G[f"{prefix}_{k}"].copy()) for k in ("pos", "dims", "rot", "probs")})


def test_world_sensor_updates_match_reference():
    from liso_amd.tracker.tracking import update_sensor_boxes_from_world_boxes, update_world_boxes_from_sensor_boxes

    w_T_s = torch.from_numpy(G["mir_w_T_s"])
    world = update_world_boxes_from_sensor_boxes(box_sequence_sensor=_seq("mir_sensor"), box_sequence_world=_seq("mir_world"), w_T_sensor_ti=w_T_s)
    sensor = update_sensor_boxes_from_world_boxes(box_sequence_world=_seq("mir_world"), box_sequence_sensor=_seq("mir_sensor"), w_T_sensor_ti=list(w_T_s))
    for got, tag in ((world, "mir_to_world"), (sensor, "mir_to_sensor")):
        assert np.abs(got.pos.numpy() - G[f"{tag}_pos"]).max() <= 1e-12 and np.abs(got.rot.numpy() - G[f"{tag}_rot"]).max() <= 1e-12
        assert np.array_equal(got.dims.numpy(), G[f"{tag}_dims"]) and np.array_equal(got.probs.numpy(), G[f"{tag}_probs"])


def test_decide_keep_or_drop_matches_reference():
    from liso_amd.tracker.tracking import decide_keep_or_drop_box

    class Cfg(dict):
        __getattr__ = dict.__getitem__

    for (ti, speed, fcd), keep, dist in zip(G["keep_cases"], G["keep_keep"], G["keep_dist"]):
        trk = G["keep_tracks"][int(ti)]
        box = Shape(pos=torch.from_numpy(trk[:, :3]), dims=torch.ones(8, 3, dtype=torch.float64) * 2.0, rot=torch.from_numpy(trk[:, 3:]),
                    probs=torch.ones(8, 1, dtype=torch.float64))
        got_keep, got_dist = decide_keep_or_drop_box(tracking_cfg=Cfg(flow_cluster_detector_min_travel_dist_filter_m=1.5),
                                                     box_sequence_world_for_specific_track_id=box, min_track_obj_speed_mps=float(speed), track_id=int(ti),
                                                     time_between_frames_s=0.1, verbose=False, is_flow_cluster_detector=bool(fcd))
        assert bool(got_keep) == bool(keep) and abs(got_dist - dist) <= 1e-12, (ti, speed, fcd)


def test_reference_names_through_install_as():
    import liso_amd

    liso_amd.install_as("liso")
    from liso.tracker.tracking import decide_keep_or_drop_box, update_sensor_boxes_from_world_boxes, update_world_boxes_from_sensor_boxes  # noqa: F401
    from liso.datasets.box_augmentation import BoxSnippetDb

    assert hasattr(BoxSnippetDb, "from_device")


# ---- the harvester through the host path, and the file round trip ----------------------------------------------------------------------
def test_harvester_file_round_trip(tmp_path):
    from liso_amd.tracker.augm_box_db_utils import load_sanitize_box_augmentation_database, save_augmentation_database

    clouds, counts, lidar_rows, sensor, world = small_sequence()
    h = H.SnippetHarvester(max_augm_db_size_mb=100)
    np.random.seed(1)
    h.add_tracked_sequence(clouds, counts, lidar_rows, sensor, world, min_track_age=2)
    boxes_per_time = [_boxes_at(sensor, t) for t in range(4)]
    h.add_untracked_sequence(clouds, counts, lidar_rows, boxes_per_time, [np.arange(b.shape[0]) + 40 for b in boxes_per_time])
    M = len(h)
    assert M >= 6 and h.max_track_id == 3 and (h.counts > 0).all() and h.points.shape == (h.counts.sum(), 4)
    assert sorted(set(h.unique_track_id) - {0, 1, 2}) and set(h.unique_track_id) >= {0, 1, 2}
    # every stored snippet is what a single cut of its own box gives
    db = h.to_dict()
    assert len(db["pcl_in_box_cosy"]) == len(db["boxes"]) == len(db["box_T_sensor"]) == len(db["lidar_rows"]) == len(db["unique_track_id"]) == M
    name, _ = save_augmentation_database(db, tmp_path, 3)
    loaded = load_sanitize_box_augmentation_database(name, 0.0)
    keep = np.flatnonzero(h.counts > 10)
    assert len(loaded["pcl_in_box_cosy"]) == len(keep) > 0
    for k, i in enumerate(keep):
        assert np.array_equal(loaded["pcl_in_box_cosy"][k], db["pcl_in_box_cosy"][i]) and np.array_equal(loaded["lidar_rows"][k], db["lidar_rows"][i])
        assert np.array_equal(loaded["box_T_sensor"][k].numpy(), db["box_T_sensor"][i])
        for a in ("pos", "dims", "rot", "probs"):
            assert np.array_equal(getattr(loaded["boxes"], a)[k].numpy(), getattr(db["boxes"][i], a).numpy()), a
    raw = np.load(name, allow_pickle=True).item()
    assert raw["unique_track_id"].dtype == np.uint32 and raw["unique_track_id"].tolist() == h.unique_track_id
    stacked = h.to_dict(stacked=True)
    assert np.array_equal(stacked["box_T_sensor"], raw["box_T_sensor"]) and np.array_equal(stacked["boxes"]["pos"], raw["boxes"]["pos"])


def _boxes_at(sensor, t):
    """the boxes of all tracks alive in frame t, as one Shape [K]"""
    alive = [s[t - st] for (_, st), s in sensor.items() if st <= t < st + s.shape[0]]
    return Shape(**{k: torch.stack([getattr(b, k) for b in alive]) for k in Shape._keys})


def test_harvester_drops_empty_snippets_and_numbers_tracks():
    clouds, counts, lidar_rows, sensor, world = small_sequence()
    far = sensor[(1, 1)].clone()
    far.pos = far.pos + torch.tensor([0.0, 0.0, 30.0])  # a track whose boxes hold no point: nothing of it is stored, its id is used up
    sensor[(1, 1)] = far
    h = H.SnippetHarvester(max_augm_db_size_mb=100)
    np.random.seed(0)
    h.add_tracked_sequence(clouds, counts, lidar_rows, sensor, world, min_track_age=2)
    assert set(h.unique_track_id) == {0, 2} and h.max_track_id == 3 and (h.counts >= 100).all()
    h.add_tracked_sequence(clouds, counts, lidar_rows, sensor, world, min_track_age=2)
    assert set(h.unique_track_id) == {0, 2, 3, 5} and h.max_track_id == 6


# ---- the C entry point refuses bad arguments before it launches --------------------------------------------------------------------------
def test_entry_point_refuses_bad_arguments():
    from liso_amd import _lib

    lib = _lib.lib()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 63) // 64 * 64)  # host memory, aligned like a device buffer; nothing is launched
    need = lib.liso_snippet_cut_workspace_bytes(2, 1000, 5)
    assert need > 0 and lib.liso_snippet_cut_workspace_bytes(2, 1000, -1) == 0 and lib.liso_snippet_cut_workspace_bytes(-1, 1000, 5) == 0

    def call(T=2, N=1000, stride=4, clouds=p, rows=p, J=5, job_cloud=p, boxes=p, cap=10, offsets=p, points=p, out_rows=p, ws=p, ws_bytes=need):
        return lib.liso_snippet_cut_f32(T, N, stride, clouds, None, rows, J, job_cloud, boxes, cap, offsets, points, out_rows, None, ws, ws_bytes, None)

    assert call(clouds=None) == EINVAL
    assert call(stride=3) == EINVAL
    assert call(J=-1) == EINVAL
    assert call(out_rows=None) == EINVAL  # lidar_rows without out_rows
    assert call(rows=None) == EINVAL  # and the other way round
    assert call(offsets=None) == EINVAL and call(points=None) == EINVAL and call(cap=-1) == EINVAL and call(ws=None) == EINVAL
    assert call(job_cloud=None) == EINVAL and call(boxes=None) == EINVAL and call(T=70000) == EINVAL
    assert call(ws_bytes=need - 1) == EWORKSPACE and call(ws_bytes=0) == EWORKSPACE
