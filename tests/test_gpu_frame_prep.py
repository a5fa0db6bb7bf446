"""Frame preparation on the device (include/liso_frame_prep.h; liso_amd/tracker/frame_prep.py) on the sequences of
tests/frame_prep_cases.py.

1. against `prepare_tracker_frames_host` given the device's mean flows: integer tables, `src`, `in_fov`, drop counts and `overflow`
   identical, fp32 columns taken from the input bitwise, fp64 fields within 1e-9; the mean flows against the restatement's own within 5e-6
2. against the reference fixture, with the bounds of tests/test_frame_prep_host.py
3. against the per-frame path: counts and means bitwise those of `mean_flow_per_box`, the kept set that of
   `drop_boxes_with_too_few_points`, the propagated poses those of `propagate_boxes_forward_using_flow` within 1e-9
4. the chain: `TrackerFrames.track` gives `DeviceFlowBasedBoxTracker`'s ids on the per-frame path's frames, and mining its result runs
5. bitwise: a batch against its single calls, two runs, permuted points, a captured replay
6. capacities between guard bands, a `cap` below the need, garbage behind the counts
7. refused sizes"""
import functools

import numpy as np
import pytest
import torch

import frame_prep_cases as FC
from test_frame_prep_host import assert_matches_reference, reference

pytestmark = pytest.mark.gpu
F64 = dict(rtol=0, atol=1e-9)
FLOW_TOL = 5e-6
CASES = [(b, c) for b in ("AB_empty", "W") for c in FC.CONFIGS]


def _device(arrays):
    return [torch.from_numpy(np.array(a)).cuda() for a in arrays]  # (a copy: the cases' arrays are read-only)


@functools.lru_cache(maxsize=None)
def _inputs(batch):
    """the device tensors of one batch, made once (read-only)"""
    return tuple(_device(FC.args_of(FC.batch(batch))))


def _prepare(batch, cfg="filter", cap=None, args=None, fov=True):
    from liso_amd.tracker.frame_prep import prepare_tracker_frames

    args = list(_inputs(batch) if args is None else args)
    if not fov:
        args = args[:9]
    return prepare_tracker_frames(*args, cap=FC.SHAPES[FC.BATCHES[batch][0]][1] if cap is None else cap, **FC.config(cfg))


def _fields(frames):
    from liso_amd.tracker.frame_prep import FIELDS

    return {k: getattr(frames, k).cpu().numpy() for k in FIELDS}


def _host(batch, cfg, cap=None, **more):
    from liso_amd.tracker.frame_prep import prepare_tracker_frames_host

    return prepare_tracker_frames_host(*FC.args_of(FC.batch(batch)), cap=FC.SHAPES[FC.BATCHES[batch][0]][1] if cap is None else cap,
                                       **FC.config(cfg), **more)


def _assert_matches_host(got, want, what):
    for k in ("n_det", "src", "in_fov", "n_points", "dropped_bev", "dropped_points", "overflow"):
        assert np.array_equal(got[k], want[k]), (what, k)
    for k in ("conf", "mean_flow"):  # (the means were handed to the restatement)
        assert got[k].tobytes() == want[k].tobytes(), (what, k)
    assert got["boxes"][..., :6].tobytes() == want["boxes"][..., :6].tobytes(), what
    for k in ("rot", "velo", "into_prev", "into_next"):
        assert got[k].dtype == np.float64 and np.allclose(got[k], want[k], **F64), (what, k)
    assert np.array_equal(got["boxes"][..., 6], got["rot"].astype(np.float32)), what  # the table carries the heading rounded to fp32


def _assert_bitwise(a, b, what):
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


@pytest.mark.parametrize("batch,cfg", CASES)
def test_device_equals_the_host_restatement(batch, cfg):
    got = _fields(_prepare(batch, cfg))
    _assert_matches_host(got, _host(batch, cfg, mean_flow=got["mean_flow"]), (batch, cfg))
    own = _host(batch, cfg)
    assert np.abs(got["mean_flow"] - own["mean_flow"]).max() <= FLOW_TOL
    assert got["n_det"].sum() > 0 and (got["n_det"][-1] == 0).all() == (batch == "AB_empty")


@pytest.mark.parametrize("cfg", ["filter", "keep_all"])
def test_more_boxes_than_a_tile_and_a_round_hold(cfg):
    """300 boxes in one frame: three tiles of the point pass, two rounds of the compaction"""
    got = _fields(_prepare("X", cfg))
    want = _host("X", cfg, mean_flow=got["mean_flow"], **FC.MARGINS)
    _assert_matches_host(got, want, ("X", cfg))
    assert np.abs(got["mean_flow"] - _host("X", cfg)["mean_flow"]).max() <= FLOW_TOL
    n = int(got["n_det"][0, 0])
    assert n == (300 if cfg == "keep_all" else 80) and got["src"][0, 0, n - 1] > 256  # (kept boxes in both rounds of the compaction)
    assert (got["dropped_bev"][0, 0], got["dropped_points"][0, 0]) == ((0, 0) if cfg == "keep_all" else (118, 102))


def test_without_a_field_of_view_cloud_every_box_is_flagged():
    got, with_fov = _fields(_prepare("AB_empty", fov=False)), _fields(_prepare("AB_empty"))
    rows = np.arange(FC.P)[None, None] < got["n_det"][..., None]
    assert np.array_equal(got["in_fov"], rows.astype(np.uint8)) and not with_fov["in_fov"][rows].all()
    _assert_bitwise({k: v for k, v in got.items() if k != "in_fov"}, {k: v for k, v in with_fov.items() if k != "in_fov"}, "no fov")


@pytest.mark.parametrize("batch,cfg", CASES)
def test_device_equals_the_reference(batch, cfg):
    frames = _prepare(batch, cfg)
    got = _fields(frames)
    for i, name in enumerate(FC.BATCHES[batch]):
        if name != "empty":
            assert_matches_reference({k: v[i] for k, v in got.items()}, reference(name, cfg), (name, cfg))
    # the raw-box database: the in-FOV rows as they were detected
    names = [[f"{n}_{t}" for t in range(got["n_det"].shape[1])] for n in FC.BATCHES[batch]]
    db = frames.to_raw_boxes_db(names)
    for i, name in enumerate(FC.BATCHES[batch]):
        for t in range(got["n_det"].shape[1]):
            want = reference(name, cfg) if name != "empty" else None
            keep = want["in_fov"][t, :want["n_det"][t]] != 0 if want is not None else np.zeros(0, bool)
            assert (f"{name}_{t}" in db) == bool(keep.any())
            if keep.any():
                entry = db[f"{name}_{t}"]
                assert np.array_equal(entry["raw_box"]["rot"][:, 0], want["raw_yaw"][t, :len(keep)][keep])
                assert np.array_equal(entry["raw_box"]["pos"], want["boxes"][t, :len(keep), :3][keep])
                assert np.array_equal(entry["raw_box"]["probs"][:, 0], want["conf"][t, :len(keep)][keep])
                assert np.allclose(entry["lidar_T_box"][:, :3, 3], entry["raw_box"]["pos"], **F64) and entry["lidar_T_box"].dtype == np.float64


def _per_frame(name, t, cfg):
    """frame t of a scene through the per-frame mirrors -> None without a kept box, else (kept Shape [k] before the alignment, src,
    count, mean, into_next, into_prev, in-FOV count, the aligned Shape)"""
    from liso_amd.eval.eval_ours import count_box_points_in_kitti_annotated_fov
    from liso_amd.kabsch.shape_utils import Shape, is_boxes_clearly_in_bev_range, soft_align_box_flip_orientation_with_motion_trafo
    from liso_amd.tracker.tracking import drop_boxes_with_too_few_points, mean_flow_per_box, propagate_boxes_forward_using_flow

    sc = FC.scene(name)
    nb, n, m = int(sc["n_box"][t]), int(sc["counts"][t]), int(sc["fov_counts"][t])
    if nb == 0:
        return None
    b, conf, pcl, valid, flow, full, odom = _device([sc["boxes"][t, :nb], sc["conf"][t, :nb], sc["clouds"][t, :n], sc["point_valid"][t, :n],
                                                     sc["flow"][t, :n], sc["fov_clouds"][t, :m], sc["odom"][t]])
    boxes = Shape(pos=b[:, :3], dims=b[:, 3:6], rot=b[:, 6:7], probs=conf[:, None], class_id=torch.arange(nb, device="cuda", dtype=torch.int32)[:, None])
    if cfg["drop_boxes_on_bev_boundaries"]:
        boxes.valid = is_boxes_clearly_in_bev_range(boxes, torch.tensor(cfg["bev_range_m"], device="cuda"))
        boxes = boxes.drop_padding_boxes()
    if boxes.shape[0] == 0:
        return None
    kept = drop_boxes_with_too_few_points(boxes, pcl, cfg["min_points_in_box"])
    if kept.shape[0] == 0:
        return None
    mean, count = mean_flow_per_box(kept[None], pcl[None, :, :3], valid[None], flow[None])
    fg, _, bg, _, into_next = propagate_boxes_forward_using_flow(kept[None], pcl[None, :, :3], valid[None], flow[None], odom, "cuda", mean_flow=mean)
    _, _, _, _, into_prev = propagate_boxes_forward_using_flow(kept[None], pcl[None, :, :3], valid[None], -1.0 * flow[None], torch.linalg.inv(odom),
                                                               "cuda", mean_flow=-mean)
    fov_count = count_box_points_in_kitti_annotated_fov(kept.clone(), full)
    aligned = soft_align_box_flip_orientation_with_motion_trafo(kept.clone()[None], fg, bg)[0]
    return kept, kept.class_id[:, 0], count[0], mean[0], into_next[0], into_prev[0], fov_count, aligned


@pytest.mark.parametrize("name", ["A", "B", "W"])
def test_device_equals_the_per_frame_path(name):
    cfg = FC.config("filter")
    frames = _prepare(name)
    got = _fields(frames)
    for t in range(FC.SHAPES[name][0]):
        n = int(got["n_det"][0, t])
        per = _per_frame(name, t, cfg) if t < FC.scene(name)["n_frames"] else None
        if per is None:
            assert n == 0, t
            continue
        kept, src, count, mean, into_next, into_prev, fov_count, aligned = per
        assert np.array_equal(got["src"][0, t, :n], src.cpu().numpy()), t  # the kept set
        assert got["n_points"][0, t, :n].tobytes() == count.cpu().numpy().tobytes() and got["mean_flow"][0, t, :n].tobytes() == mean.cpu().numpy().tobytes(), t
        assert np.allclose(got["into_next"][0, t, :n], into_next.cpu().numpy(), **F64) and np.allclose(got["into_prev"][0, t, :n], into_prev.cpu().numpy(), **F64), t
        assert np.array_equal(got["in_fov"][0, t, :n], (fov_count >= FC.MIN_POINTS).cpu().numpy().astype(np.uint8)), t
        assert np.allclose(got["rot"][0, t, :n], aligned.rot[:, 0].cpu().numpy(), **F64) and np.allclose(got["velo"][0, t, :n], aligned.velo.cpu().numpy(), **F64), t


def test_the_chain_tracks_like_the_per_frame_path_and_its_result_is_mined():
    from liso_amd.tracker.device_tracker import DeviceFlowBasedBoxTracker
    from liso_amd.tracker.track_mining import mine_tracked_sequences

    cfg, sc = FC.config("filter"), FC.scene("A")
    tracker = DeviceFlowBasedBoxTracker(use_propagated_boxes=True, box_matching_threshold_m=5.0)
    for t in range(sc["n_frames"]):
        per = _per_frame("A", t, cfg)
        odom = torch.from_numpy(sc["odom"][t].copy()).cuda()
        if per is None:
            from liso_amd.kabsch.shape_utils import Shape

            none = torch.zeros((0, 3), device="cuda")
            empty = Shape(pos=none, dims=none.clone(), rot=none[:, :1].double(), probs=none[:, :1].clone(), velo=none.double())
            tracker.update(empty, torch.zeros((0, 4, 4), dtype=torch.float64, device="cuda"), torch.zeros((0, 4, 4), dtype=torch.float64, device="cuda"), odom)
        else:
            tracker.update(per[7], per[4], per[5], odom)
    tracker.run_tracker()
    frames = _prepare("A")
    tracked = frames.track(5.0, tracker._cap)
    n_out, want_n = tracked.n_out.cpu().numpy()[0], tracker.result.n_out.cpu().numpy()[0]
    assert np.array_equal(n_out, want_n) and n_out.sum() > 0
    assert np.array_equal(tracked.track_ids.cpu().numpy()[0], tracker.result.track_ids.cpu().numpy()[0])
    assert int(tracked.overflow.sum()) == 0 and int(tracked.id_counter[0]) == int(tracker.result.id_counter[0])
    clouds, counts = _inputs("A")[5], _inputs("A")[6]
    mined = mine_tracked_sequences(tracked, frames.boxes, frames.conf, clouds, counts, max_tracks=32, cap_out=8, min_track_age=2,
                                   confidence_threshold_mined_boxes=0.3, min_track_obj_speed_mps=0.0, time_between_frames_s=0.1,
                                   is_flow_cluster_detector=False, flow_cluster_detector_min_travel_dist_filter_m=3.0, fit_rot=False, fit_pos=False,
                                   fitting_dims_bloat_factor=1.2, use_track_smoothing=False, in_annotated_fov=frames.in_fov,
                                   export_only_in_annotated_fov=True)
    assert int(mined.overflow.sum()) == 0 and mined.frames.n_boxes.shape == (1, FC.T)


def test_a_batch_equals_its_single_calls_bitwise():
    together = _fields(_prepare("AB_empty"))
    for i, name in enumerate(("A", "B")):
        alone = _fields(_prepare(name))
        for k in alone:
            assert alone[k][0].tobytes() == together[k][i].tobytes(), (name, k)
    for k, v in together.items():  # the sequence without a frame: blank rows
        assert not v[2].any() if k != "src" else (v[2] == -1).all(), k


def test_two_runs_are_bitwise_equal():
    _assert_bitwise(_fields(_prepare("AB_empty")), _fields(_prepare("AB_empty")), "two runs")


def test_permuted_points_change_nothing_bitwise():
    b = {k: v.copy() for k, v in FC.batch("AB_empty").items()}
    rng = np.random.default_rng(5)
    for s in range(len(b["n_frames"])):
        for t in range(FC.T):
            n, m = int(b["counts"][s, t]), int(b["fov_counts"][s, t])
            order, fov_order = rng.permutation(n), rng.permutation(m)
            for k in ("clouds", "point_valid", "flow"):
                b[k][s, t, :n] = b[k][s, t, :n][order]
            b["fov_clouds"][s, t, :m] = b["fov_clouds"][s, t, :m][fov_order]
    assert not np.array_equal(b["flow"], FC.batch("AB_empty")["flow"])
    _assert_bitwise(_fields(_prepare("AB_empty")), _fields(_prepare("AB_empty", args=_device(FC.args_of(b)))), "permuted")


def test_a_captured_replay_equals_the_eager_call_bitwise():
    from liso_amd.tracker.frame_prep import FIELDS
    from liso_amd.utils.graph_capture import capture

    eager = _fields(_prepare("AB_empty"))
    stream = torch.cuda.Stream()
    graph, out = capture(lambda: _prepare("AB_empty"), stream, warm_ups=2)
    for k in FIELDS:
        getattr(out, k).fill_(7)  # (the replay, not the capture, fills the tables)
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        graph.replay()
    stream.synchronize()
    _assert_bitwise(eager, _fields(out), "replay")


def test_exact_capacities_between_guard_bands():
    """`cap` at its exact need, P across two wavefronts: every table and the workspace lie between guard bands, nothing is written outside"""
    from tests.guarded_alloc import guarded

    want = _host("W", "filter")
    need = int(want["n_det"].max())
    assert need == 47
    with guarded() as g:
        frames = _prepare("W", cap=need)
        assert g.check() > 0
    got = _fields(frames)
    assert not got["overflow"].any() and np.array_equal(got["n_det"], want["n_det"]) and np.array_equal(got["src"], want["src"][:, :, :need])
    with guarded() as g:
        frames = _prepare("AB_empty", "keep_all")
        assert g.check() > 0
    assert _fields(frames)["n_det"].max() == FC.P


def test_a_cap_below_the_need():
    roomy = _fields(_prepare("W"))
    need = int(roomy["n_det"].max())
    tight = _fields(_prepare("W", cap=need - 1))
    assert tight["overflow"].tolist() == [1] and tight["n_det"].tolist() == [[need - 1]]
    for k in tight:
        if k not in ("n_det", "overflow"):
            assert tight[k].tobytes() == np.ascontiguousarray(roomy[k][:, :, :need - 1] if roomy[k].ndim > 2 else roomy[k]).tobytes(), k
    tight = _fields(_prepare("AB_empty", cap=5))
    roomy = _fields(_prepare("AB_empty"))
    assert np.array_equal(tight["overflow"], np.maximum(roomy["n_det"] - 5, 0).sum(axis=1)) and tight["overflow"].tolist() == [4, 2, 0]
    assert np.array_equal(tight["src"], roomy["src"][:, :, :5]) and tight["into_next"].tobytes() == np.ascontiguousarray(roomy["into_next"][:, :, :5]).tobytes()


def test_garbage_behind_the_counts_changes_nothing_bitwise():
    clean = FC.batch("AB_empty")
    b = {k: v.copy() for k, v in clean.items()}
    for s in range(len(b["n_frames"])):
        for t in range(FC.T):
            if t >= b["n_frames"][s]:
                b["n_box"][s, t], b["counts"][s, t], b["fov_counts"][s, t] = 7, 2000, 2500
                nb = n = m = 0
                b["odom"][s, t] = np.nan
            else:
                nb, n, m = int(b["n_box"][s, t]), int(b["counts"][s, t]), int(b["fov_counts"][s, t])
            b["boxes"][s, t, nb:], b["conf"][s, t, nb:] = np.nan, np.nan
            b["clouds"][s, t, n:], b["flow"][s, t, n:], b["point_valid"][s, t, n:] = np.nan, np.nan, 255
            b["fov_clouds"][s, t, m:] = np.nan
    # finite garbage too: a box around the sensor and points inside it, where a kernel that read them would count them
    b["boxes"][0, 1, 6:], b["conf"][0, 1, 6:] = b["boxes"][0, 1, 0], 0.99  # (frame 1 of A has six boxes)
    b["clouds"][1, 0, int(b["counts"][1, 0]):, :3] = b["boxes"][1, 0, 0, :3]
    b["flow"][1, 0, int(b["counts"][1, 0]):] = 3.0
    b["boxes"][1, 1] = b["boxes"][1, 0]  # (the frame without boxes)
    _assert_bitwise(_fields(_prepare("AB_empty")), _fields(_prepare("AB_empty", args=_device(FC.args_of(b)))), "garbage")


def test_refused_sizes_raise_and_an_empty_batch_gives_empty_tables():
    from liso_amd._lib import LisoHipError
    from liso_amd.tracker.frame_prep import FIELDS, prepare_tracker_frames

    args = list(_inputs("A"))
    with pytest.raises(LisoHipError, match="sizes refused"):
        prepare_tracker_frames(*args, cap=0, **FC.config("filter"))
    wide = list(args)
    wide[2], wide[3] = torch.zeros((1, FC.T, 1025, 7), device="cuda"), torch.zeros((1, FC.T, 1025), device="cuda")
    with pytest.raises(LisoHipError, match="sizes refused"):
        prepare_tracker_frames(*wide, cap=8, **FC.config("filter"))
    narrow = list(args)
    narrow[5] = args[5][..., :2].contiguous()
    with pytest.raises(LisoHipError, match="sizes refused"):
        prepare_tracker_frames(*narrow, cap=8, **FC.config("filter"))
    with pytest.raises(LisoHipError):
        prepare_tracker_frames(*[a.cpu() for a in args], cap=8, **FC.config("filter"))
    empty = prepare_tracker_frames(*[a[:0] for a in args], cap=8, **FC.config("filter"))
    assert all(getattr(empty, k).shape[0] == 0 for k in FIELDS) and empty.into_next.shape == (0, FC.T, 8, 4, 4)
    wide_ok = list(args)
    wide_ok[2], wide_ok[3] = torch.zeros((1, FC.T, 512, 7), device="cuda"), torch.zeros((1, FC.T, 512), device="cuda")
    wide_ok[2][:, :, :FC.P], wide_ok[3][:, :, :FC.P] = args[2], args[3]
    got, want = _fields(prepare_tracker_frames(*wide_ok, cap=8, **FC.config("filter"))), _fields(_prepare("A"))
    _assert_bitwise(got, want, "P = 512")
