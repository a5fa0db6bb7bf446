"""Track mining on the device (include/liso_track_mining.h; liso_amd/tracker/track_mining.py) on the sequences of
tests/track_mining_cases.py.

* every stage against `mine_tracked_sequences_host` (checked against a literal per-track loop in tests/test_track_mining_host.py):
  ages, starts, verdicts, ids, counts and the median confidence identical; fp64 fields within 1e-9 (fp64 products in another order),
  fp32 fields within 1e-6.  `refined_dims` within 4 fp32 ulps of the fp64 interpolation: the kernel rounds the fraction, the difference
  of the two neighbours, its product with the fraction and the sum -- on positive values of one magnitude each costs at most one ulp
  of the result.
* with the rectangle fit on, the refined sensor boxes against `perform_local_box_refinement` track by track on the same device, and the
  whole stage against the host restatement given the device's fits.
* "jerk": the SMOOTHED tracks' world boxes are exactly what `smooth_track_jerk` makes of the tables `smoothing_tables` hands to it, the
  other tracks are untouched.  "none": the positions are the float32 tables the smoothing is given (the reference stores a smoothed
  track's positions as it gets them from the smoother, in float32: the table, and with it the refined position to float32 rounding) and
  `velo` is `batched_displacement_from_pos` of them.
* a batch against its single-sequence calls, two runs, a captured replay against the eager call: bitwise.
* one run between guard bands with cap_out and max_tracks at their exact need; a cap_out below the need; refused sizes."""
import functools

import numpy as np
import pytest
import torch

import track_mining_cases as C
import tracker_scenes as TS

pytestmark = pytest.mark.gpu

F64, F32 = dict(rtol=0, atol=1e-9), dict(rtol=0, atol=1e-6)
PER_TRACK_EXACT = ("age", "start", "verdict", "median_conf")
SHAPES = {"world": "world_refined", "sensor": "sensor_refined", "world_raw": "world_raw", "sensor_raw": "sensor_raw"}
FRAME_EXACT = ("n_boxes", "track_id", "valid", "max_confidence")
FULL = dict(fit_rot=True, fit_pos=True, track_smoothing_method="jerk")


@functools.lru_cache(maxsize=None)
def _inputs(batch):
    """device tensors of one batch and the tracker's result on them, made once (read-only)"""
    from liso_amd.tracker.device_tracker import track_sequences

    arrays, extra, _ = C.batch(batch)
    dev = {k: torch.from_numpy(v).cuda() for k, v in {**arrays, **extra}.items()}
    tracked = track_sequences(**{k: dev[k] for k in arrays}, threshold=TS.THRESHOLD, cap=C.tracked_host(batch)[1])
    return dev, tracked


@functools.lru_cache(maxsize=None)
def _host(batch, cfg, cap_out=6):
    from liso_amd.tracker.track_mining import mine_tracked_sequences_host

    arrays, extra, _ = C.batch(batch)
    return mine_tracked_sequences_host(C.tracked_host(batch)[0], arrays["boxes"], arrays["conf"], max_tracks=C.needed_tracks(batch), cap_out=cap_out,
                                       in_annotated_fov=extra["in_fov"], margin=1e-6, **C.config(cfg))


def _mine(batch, cfg="network", cap_out=6, max_tracks=None, **more):
    from liso_amd.tracker.track_mining import mine_tracked_sequences

    dev, tracked = _inputs(batch)
    return mine_tracked_sequences(tracked, dev["boxes"], dev["conf"], dev["clouds"], dev["counts"], max_tracks=max_tracks or C.needed_tracks(batch),
                                  cap_out=cap_out, in_annotated_fov=dev["in_fov"], **C.config(cfg, **more))


SELECT_KEYS = ("min_track_age", "confidence_threshold_mined_boxes", "min_track_obj_speed_mps", "time_between_frames_s", "is_flow_cluster_detector",
               "flow_cluster_detector_min_travel_dist_filter_m", "min_dist_for_track_smoothing", "use_track_smoothing")


def _select_refine(batch, conf, fit):
    """the first two stages on their own -> (SelectedTracks, RefinedTracks)"""
    from liso_amd.tracker.track_mining import refine_tracks, select_tracks

    dev, tracked = _inputs(batch)
    sel = select_tracks(tracked, dev["boxes"], dev["conf"], max_tracks=C.needed_tracks(batch), **{k: conf[k] for k in SELECT_KEYS})
    return sel, refine_tracks(sel, tracked, dev["clouds"], dev["counts"], fit_rot=fit, fit_pos=fit, fitting_dims_bloat_factor=1.2, time_between_frames_s=C.DT)


def _fields(mined):
    """every tensor of a MinedTracks under the names of the host restatement"""
    out = {k: getattr(mined, k) for k in ("n_tracks", "overflow", "age", "start", "median_conf", "dist_covered_m", "verdict", "refined_dims")}
    for key, attr in SHAPES.items():
        out[key + "_pos"], out[key + "_rot"] = getattr(mined, attr).pos, getattr(mined, attr).rot
    out.update(dims=mined.world_refined.dims, probs=mined.world_refined.probs, velo=mined.velo, raw_dims=mined.world_raw.dims,
               raw_probs=mined.world_raw.probs)
    out.update({"frame_" + k: getattr(mined.frames, k) for k in ("n_boxes", "pos", "rot", "dims", "probs", "velo", "track_id", "lidar_T_box",
                                                                 "max_confidence", "valid")})
    return {k: v.cpu().numpy() for k, v in out.items()}


def _assert_matches_host(got, want, what):
    for k in PER_TRACK_EXACT + ("n_tracks", "overflow") + tuple("frame_" + f for f in FRAME_EXACT):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (what, k, got[k], want[k])
    err = np.abs(got["refined_dims"].astype(np.float64) - want["refined_dims_f64"])
    assert (err <= 4 * np.spacing(np.abs(want["refined_dims_f64"]).astype(np.float32))).all(), (what, "refined_dims", err.max())
    for k, v in got.items():
        if v.dtype == np.float64:
            assert v.shape == want[k].shape and np.allclose(v, want[k], **F64), (what, k, np.abs(v - want[k]).max())
        elif v.dtype == np.float32 and k not in ("median_conf", "frame_max_confidence"):
            assert v.shape == want[k].shape and np.allclose(v, want[k], **F32), (what, k, np.abs(v - want[k]).max())


@pytest.mark.parametrize("batch,cfg", [(b, c) for b in ("AB", "A_empty", "empty_A") for c in C.CONFIGS])
def test_device_equals_the_host_restatement(batch, cfg):
    want = _host(batch, cfg)
    # stage by stage: the selection, the refinement (before any smoothing), the whole
    sel, ref = _select_refine(batch, C.config(cfg), False)
    for k in PER_TRACK_EXACT:
        assert np.array_equal(getattr(sel, k).cpu().numpy(), want[k]), (k, getattr(sel, k), want[k])
    assert np.allclose(sel.dist_covered_m.cpu().numpy(), want["dist_covered_m"], **F64)
    for kind, box in (("sensor_raw", sel.sensor_raw), ("world_raw", sel.world_raw)):
        assert np.allclose(box.pos.cpu().numpy(), want[kind + "_pos"], **F64) and np.allclose(box.rot.cpu().numpy(), want[kind + "_rot"], **F64), kind
        assert np.array_equal(box.dims.cpu().numpy(), want["raw_dims"]) and np.array_equal(box.probs.cpu().numpy(), want["raw_probs"]), kind
    assert np.allclose(ref.sensor.pos.cpu().numpy(), want["refined_sensor_pos"], **F64)
    assert np.allclose(ref.sensor.rot.cpu().numpy(), want["refined_sensor_rot"], **F64)
    _assert_matches_host(_fields(_mine(batch, cfg)), want, (batch, cfg))


def test_refinement_equals_the_per_track_path_and_the_host_given_the_fits():
    from liso_amd.networks.flow_cluster_detector.flow_cluster_detector import FlowClusterDetector
    from liso_amd.tracker.track_mining import KEPT, mine_tracked_sequences_host
    from liso_amd.tracker.tracking import perform_local_box_refinement
    from liso_amd.utils.config import to_attr

    dev, _ = _inputs("AB")
    arrays, extra, _ = C.batch("AB")
    counts = extra["counts"]
    for cfg_name in ("network", "flow_cluster"):
        conf = C.config(cfg_name, fit_rot=True, fit_pos=True)
        sel, ref = _select_refine("AB", conf, True)
        ref_cfg = to_attr({"data": {"tracking_cfg": {"fit_box_to_points": {"fit_rot": True, "fit_pos": True, "fitting_dims_bloat_factor": 1.2}}}})
        predictor = object.__new__(FlowClusterDetector) if conf["is_flow_cluster_detector"] else object()
        age, start, verdict = sel.age.cpu().numpy(), sel.start.cpu().numpy(), sel.verdict.cpu().numpy()
        fit_count = ref.fit_count.cpu().numpy()
        moved = 0
        for s, m in zip(*np.where(verdict & KEPT)):
            n, first = int(age[s, m]), int(start[s, m])
            clouds = [dev["clouds"][s, t, :int(counts[s, t])] for t in range(C.T)]
            seq = perform_local_box_refinement(ref_cfg, predictor, clouds, sel.sensor_raw[s, m, :n].clone(), n, first)
            got = ref.sensor[s, m, :n]
            assert np.allclose(got.pos.cpu().numpy(), seq.pos.cpu().numpy(), **F64) and np.allclose(got.rot.cpu().numpy(), seq.rot.cpu().numpy(), **F64), (s, m)
            assert np.allclose(got.dims.cpu().numpy(), seq.dims.cpu().numpy(), **F32), (s, m)
            moved += int((fit_count[s, first:first + n, m] > 0).sum())
        planted = sum(len(C.PLANTED[name]) for name in ("A", "B"))
        # every planted object's track holds points in some frame, no other kept track does (track 4 of A is the object without points)
        assert moved > 0 and (fit_count[0, :, 3] == 0).all() and (fit_count > 0).any(axis=1).sum() == planted
        want = mine_tracked_sequences_host(C.tracked_host("AB")[0], arrays["boxes"], arrays["conf"], max_tracks=C.needed_tracks("AB"), cap_out=6,
                                           in_annotated_fov=extra["in_fov"], margin=1e-6, fits=(fit_count, ref.fit.cpu().numpy()), **conf)
        assert not np.allclose(want["refined_sensor_pos"], _host("AB", cfg_name)["refined_sensor_pos"], rtol=0, atol=1e-3)  # the fit moves boxes
        _assert_matches_host(_fields(_mine("AB", cfg_name, fit_rot=True, fit_pos=True)), want, cfg_name)


def test_jerk_smoothing_is_the_smoother_on_the_stage_tables_and_leaves_the_other_tracks_alone():
    from liso_amd.tracker.track_mining import SMOOTHED, smooth_tracks, smoothing_tables
    from liso_amd.tracker.track_smoothing import smooth_track_jerk

    sel, ref = _select_refine("AB", C.config("network"), True)
    before = {k: getattr(ref.world, k).clone() for k in ("pos", "rot", "velo")}
    tables = [tuple(v.clone() for v in smoothing_tables(sel, ref, s)) for s in range(2)]
    smooth_tracks(sel, ref, track_smoothing_method="jerk", time_between_frames_s=C.DT)
    rows = sel.row_valid(SMOOTHED)
    assert rows.any(dim=2).sum() >= 4
    for s, (pos, yaw, valid) in enumerate(tables):
        assert torch.equal(valid, rows[s])
        want = smooth_track_jerk(batched_observed_pos_m=pos, batched_observed_yaw_angle_rad=yaw, batched_valid_mask=valid, time_between_frames_s=C.DT)
        for k, w in zip(("pos", "rot", "velo"), want):
            got = getattr(ref.world, k)[s]
            assert torch.equal(got[valid], w[valid].to(got.dtype)), (s, k)
            assert torch.equal(got[~valid], before[k][s][~valid]), (s, k)
        assert not torch.equal(ref.world.pos[s][valid], before["pos"][s][valid])  # (the smoother moved something)


def test_bike_model_smoothing_is_the_smoother_on_the_smoothed_tracks():
    """the bicycle model's L-BFGS needs every row of its batch valid somewhere: the stage hands it the SMOOTHED tracks only"""
    from liso_amd.tracker.track_mining import SMOOTHED, smooth_tracks, smoothing_tables
    from liso_amd.tracker.track_smoothing import smooth_track_bike_model

    sel, ref = _select_refine("A", C.config("network"), False)
    before = {k: getattr(ref.world, k).clone() for k in ("pos", "rot", "velo")}
    pos, yaw, valid = (v.clone() for v in smoothing_tables(sel, ref, 0))
    smooth_tracks(sel, ref, track_smoothing_method="bike_model", time_between_frames_s=C.DT)
    picked = torch.nonzero(valid[:, 0])[:, 0]
    assert picked.numel() == 3 and torch.equal(valid, sel.row_valid(SMOOTHED)[0])
    want = smooth_track_bike_model(batched_observed_pos_m=pos[picked], batched_observed_yaw_angle_rad=yaw[picked], batched_valid_mask=valid[picked],
                                   batched_vehicle_length_m=sel.refined_dims[0, picked, 0], time_between_frames_s=C.DT)
    for k, w in zip(("pos", "rot", "velo"), want):
        got = getattr(ref.world, k)[0]
        assert torch.isfinite(got).all() and torch.equal(got[picked][valid[picked]], w.detach()[valid[picked]].to(got.dtype)), k
        assert torch.equal(got[~valid], before[k][0][~valid]), k


def test_no_smoothing_method_keeps_the_positions_and_gives_the_displacements():
    from liso_amd.tracker.track_mining import SMOOTHED
    from liso_amd.tracker.track_smoothing import batched_displacement_from_pos

    plain, none = _mine("AB", "no_smoothing"), _mine("AB", "network")  # (the base configuration smooths with "none")
    rows = ((none.verdict & SMOOTHED) != 0)[..., None] & none.world_refined.valid
    assert rows.any() and not (plain.verdict & SMOOTHED).any()
    refined = plain.world_refined.pos  # the same tracks without the smoothing branch: the refined positions
    table = (refined * rows[..., None]).float()
    assert torch.equal(none.world_refined.pos[rows], table[rows].double())
    assert ((none.world_refined.pos - refined).abs()[rows] <= torch.finfo(torch.float32).eps * refined.abs()[rows]).all()
    assert torch.equal(none.world_refined.pos[~rows], refined[~rows]) and torch.equal(none.world_refined.rot[~rows], plain.world_refined.rot[~rows])
    for s in range(2):
        assert torch.equal(none.velo[s][rows[s]], batched_displacement_from_pos(table[s])[..., None][rows[s]])
    assert torch.equal(none.velo[~rows], plain.velo[~rows])


def _assert_bitwise(a, b, what, pick=lambda k, v: v):
    for k in a:
        assert pick(k, a[k]).tobytes() == pick(k, b[k]).tobytes(), (what, k)


def test_a_batch_equals_its_single_calls_bitwise():
    M = C.needed_tracks("AB")
    together = _fields(_mine("AB", **FULL))
    for i, name in enumerate(("A", "B")):
        alone = _fields(_mine(name, max_tracks=M, **FULL))
        for k in alone:
            assert alone[k][0].tobytes() == together[k][i].tobytes(), (name, k)
    assert (together["verdict"] & 8).any() and together["frame_n_boxes"].sum() > 0


def test_two_runs_are_bitwise_equal():
    _assert_bitwise(_fields(_mine("AB", "fov", **FULL)), _fields(_mine("AB", "fov", **FULL)), "two runs")


def test_a_captured_replay_equals_the_eager_call_bitwise():
    from liso_amd.utils.graph_capture import capture

    eager = _fields(_mine("AB", "fov", **FULL))
    stream = torch.cuda.Stream()
    graph, out = capture(lambda: _mine("AB", "fov", **FULL), stream, warm_ups=2)
    for t in (out.verdict, out.overflow, out.frames.n_boxes, out.frames.pos, out.world_refined.pos, out.sensor_refined.pos, out.frames.track_id):
        t.fill_(7)  # (the replay, not the capture, fills the tables)
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        graph.replay()
    stream.synchronize()
    _assert_bitwise(eager, _fields(out), "replay")


def test_exact_capacities_between_guard_bands():
    """cap_out and max_tracks at their exact need: every table of the call lies between guard bands, nothing is written outside"""
    from tests.guarded_alloc import guarded

    want = _host("AB", "no_speed_filter")
    need = int(want["frame_n_boxes"].max())
    assert int(want["n_tracks"].max()) == C.needed_tracks("AB")
    with guarded() as g:
        mined = _mine("AB", "no_speed_filter", cap_out=need, **FULL)
        assert g.check() > 0
    got = _fields(mined)
    assert not got["overflow"].any() and np.array_equal(got["frame_n_boxes"], want["frame_n_boxes"]) and int(got["frame_n_boxes"].max()) == need
    assert np.array_equal(got["frame_track_id"], want["frame_track_id"][:, :, :need]) and np.array_equal(got["verdict"], want["verdict"])


def test_a_cap_out_below_the_need():
    roomy = _host("AB", "network")
    need = int(roomy["frame_n_boxes"].max())
    got = _fields(_mine("AB", "network", cap_out=need - 1))
    _assert_matches_host(got, _host("AB", "network", need - 1), "tight")
    surplus = np.maximum(roomy["frame_n_boxes"] - (need - 1), 0).sum(axis=1)
    assert surplus.max() > 0 and np.array_equal(got["overflow"], surplus)
    assert np.array_equal(got["frame_track_id"], roomy["frame_track_id"][:, :, :need - 1])
    assert np.allclose(got["frame_pos"], roomy["frame_pos"][:, :, :need - 1], **F64)


def test_more_tracks_than_max_tracks_are_reported_not_written():
    got = _fields(_mine("AB", "network", max_tracks=3))
    want = _host("AB", "network")
    assert got["n_tracks"].tolist() == want["n_tracks"].tolist() and got["age"].shape == (2, 3)
    assert np.array_equal(got["verdict"], want["verdict"][:, :3]) and (got["frame_track_id"] <= 3).all()


def test_sizes_the_lds_plans_cannot_hold_are_refused():
    import dataclasses

    from liso_amd._lib import LisoHipError
    from liso_amd.tracker.track_mining import select_tracks

    dev, tracked = _inputs("A")
    rest = dict(min_track_age=4, confidence_threshold_mined_boxes=0.5, min_track_obj_speed_mps=1.0, time_between_frames_s=0.1,
                is_flow_cluster_detector=False, flow_cluster_detector_min_travel_dist_filter_m=3.0)
    with pytest.raises(LisoHipError, match="sizes refused"):
        select_tracks(tracked, dev["boxes"], dev["conf"], max_tracks=8193, **rest)
    long = dataclasses.replace(tracked, track_ids=torch.zeros((1, 1025, 2), dtype=torch.int64, device="cuda"))
    with pytest.raises(LisoHipError, match="sizes refused"):
        select_tracks(long, torch.zeros((1, 1025, 1, 7), device="cuda"), torch.zeros((1, 1025, 1), device="cuda"), max_tracks=4, **rest)
    with pytest.raises(LisoHipError, match="cap_out"):
        _mine("A", cap_out=0)
