"""The sequence tracker on the device (include/liso_tracking.h: liso_track_sequences; liso_amd/tracker/device_tracker.py).

* `DeviceFlowBasedBoxTracker` on the golden sequences a, b, d of tests/golden/tracker_reference.npz: the assertions of
  tests/test_tracker_sequence.py with its tolerances (case c's golden ids hang on torch.argsort's order of equal confidences).
* `track_sequences` against `track_sequences_host` (checked against the host class in tests/test_device_tracker_host.py) on all
  four golden sequences and on the generated ones of tests/tracker_scenes.py: n_out, ids, src, is_fill, id counter, overflow exactly;
  world boxes and sensor poses within 1e-9 (fp64 products in another order).  The generated inputs keep every fp64 distance 1e-3 m
  away from a decision (asserted by the host run): at 500 m the fp32 spacing is 3e-5 m and the distance carries a few of those.
* batching, run-to-run and captured-replay results bitwise; a capacity below the need; the smoothing tables.
"""
import functools

import numpy as np
import pytest
import torch

import tracker_scenes as TS

pytestmark = pytest.mark.gpu

CASES = [str(c) for c in TS.G["cases"]]
EXACT = ("n_out", "track_ids", "src", "is_fill", "id_counter", "overflow")
CLOSE = ("pos_world", "rot_world", "w_T_sensor")
ATTRS = ("pos", "dims", "rot", "probs")


@functools.lru_cache(maxsize=None)
def _scenes():
    return TS.generated_scenes()


@functools.lru_cache(maxsize=None)
def _scene(name):
    return TS.golden_scene(name) if name in CASES else _scenes()[name]


def _cap(scene):
    from liso_amd.tracker.device_tracker import needed_capacity

    return needed_capacity(scene["n_det"])


@functools.lru_cache(maxsize=None)
def _host(name, cap=None):
    """the yardstick of one sequence, computed once (read-only)"""
    from liso_amd.tracker.device_tracker import track_sequences_host

    scene = _scene(name)
    return track_sequences_host(**TS.batch([scene]), threshold=TS.THRESHOLD, cap=cap or _cap(scene), margin=None if name in CASES else 1e-3)


def _device(arrays, cap):
    from liso_amd.tracker.device_tracker import track_sequences

    return track_sequences(**{k: torch.from_numpy(v).cuda() for k, v in arrays.items()}, threshold=TS.THRESHOLD, cap=cap)


def _np(res):
    return {k: getattr(res, k).cpu().numpy() for k in EXACT + CLOSE}


def _assert_equal(got, want, what):
    for k in EXACT:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (what, k, got[k], want[k])
    for k in CLOSE:
        assert got[k].dtype == want[k].dtype and np.allclose(got[k], want[k], rtol=0, atol=1e-9), (what, k, np.abs(got[k] - want[k]).max())


@pytest.mark.parametrize("tag", ["a", "b", "d"])
def test_device_class_reproduces_the_golden_sequences(tag):
    from liso_amd.tracker.device_tracker import DeviceFlowBasedBoxTracker

    tr = DeviceFlowBasedBoxTracker(use_propagated_boxes=True, box_matching_threshold_m=2.0)
    tr.test_device = "cuda"
    scene = _scene(tag)
    TS.run_host_class(scene, tr)
    key, G = f"{tag}_flow", TS.G
    world, sensor = tr.get_boxes_in_world_coordinates(), tr.get_boxes_in_sensor_coordinates_at_each_timestamp()
    ids = TS.golden_frames(key, "ids")
    assert len(tr.track_ids) == len(ids)
    for t, want in enumerate(ids):
        assert np.array_equal(tr.track_ids[t].cpu().numpy(), want), (t, tr.track_ids[t], want)
    for view, boxes in (("world", world), ("sensor", sensor)):
        for a in ATTRS:
            for t, want in enumerate(TS.golden_frames(key, f"{view}_{a}")):
                got = getattr(boxes[t], a).cpu().numpy()
                assert got.shape == want.shape and got.dtype == want.dtype, (view, a, t, got.shape, want.shape, got.dtype, want.dtype)
                assert np.allclose(got, want, rtol=0, atol=1e-9 if want.dtype == np.float64 else 1e-6), (view, a, t)
    # (the scenes number their attribute entries 1000 * frame + slot; the golden ones carry the fixture's uid of the same detection)
    uid = [u.tolist() for u in TS.golden_frames(tag, "in_attr")]
    for t, want in enumerate(TS.golden_frames(key, "attrs")):
        got = [uid[d["uid"] // 1000][d["uid"] % 1000] for d in tr.get_extra_attributes_at_each_timestamp()[t]]
        assert got == want.tolist(), t
    tids, lens = tr.get_ids_lengths_of_longest_tracks()
    assert np.array_equal(lens.cpu().numpy(), G[key + "_longest_lens"]) and np.array_equal(np.sort(tids.cpu().numpy()), G[key + "_id_set"])
    lo, hi = tr.get_min_max_track_id()
    assert [int(lo), int(hi)] == G[key + "_min_max"].tolist() and int(tr.max_track_id_counter) == int(G[key + "_counter"])
    rows = TS.golden_frames(key, "probe_rows")
    for i, tid in enumerate(G[key + "_probe_ids"]):
        box_idxs, start = tr.get_box_indices_start_time_for_track_id(int(tid))
        assert np.array_equal(box_idxs.cpu().numpy(), rows[i]) and int(start) == int(G[key + "_probe_start"][i])


@pytest.mark.parametrize("name", CASES + sorted(TS.generated_scenes()))
def test_device_equals_the_host_restatement(name):
    scene = _scene(name)
    _assert_equal(_np(_device(TS.batch([scene]), _cap(scene))), _host(name), name)


FIVE = ("T1", "T2", "T3_all_lost", "story", "T25")


def test_a_batch_equals_its_single_calls_bitwise():
    cap = max(_cap(_scene(n)) for n in FIVE)
    together = _np(_device(TS.batch([_scene(n) for n in FIVE]), cap))
    for i, name in enumerate(FIVE):
        alone, T = _np(_device(TS.batch([_scene(name)]), cap)), len(_scene(name)["n_det"])
        _assert_equal(alone, _host(name, cap), name)
        for k in EXACT + CLOSE:
            a, b = alone[k][0], together[k][i]
            assert a.tobytes() == (b if k in ("id_counter", "overflow") else b[:T]).tobytes(), (name, k)
        # frames behind the sequence are blank
        assert (together["track_ids"][i, T:] == -1).all() and (together["src"][i, T:] == -1).all() and not together["n_out"][i, T:].any()
        assert np.array_equal(together["w_T_sensor"][i, T:], np.tile(np.eye(4), (together["w_T_sensor"].shape[1] - T, 1, 1)))


def test_two_runs_are_bitwise_equal():
    arrays = TS.batch([_scene("story"), _scene("T6_counts")])
    cap = _cap(_scene("T6_counts"))
    first, second = _np(_device(arrays, cap)), _np(_device(arrays, cap))
    for k in EXACT + CLOSE:
        assert first[k].tobytes() == second[k].tobytes(), k


def test_a_captured_replay_equals_the_eager_call_bitwise():
    from liso_amd.tracker.device_tracker import track_sequences
    from liso_amd.utils.graph_capture import capture

    arrays = TS.batch([_scene("story"), _scene("T25")])
    cap = max(_cap(_scene("story")), _cap(_scene("T25")))
    static = {k: torch.from_numpy(v).cuda() for k, v in arrays.items()}
    eager = _np(track_sequences(**static, threshold=TS.THRESHOLD, cap=cap))
    stream = torch.cuda.Stream()
    graph, out = capture(lambda: track_sequences(**static, threshold=TS.THRESHOLD, cap=cap), stream, warm_ups=2)
    for k in EXACT + CLOSE:
        getattr(out, k).fill_(7)  # (the replay, not the capture, fills the tables)
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        graph.replay()
    stream.synchronize()
    replayed = _np(out)
    for k in EXACT + CLOSE:
        assert eager[k].tobytes() == replayed[k].tobytes(), k
    assert np.array_equal(out.boxes.valid.cpu().numpy(), np.arange(cap)[None, None] < eager["n_out"][..., None])


@pytest.mark.parametrize("name,cap", [("story", 23), ("story", 22), ("T6_counts", 70), ("T6_counts", 10)])
def test_a_capacity_below_the_need(name, cap):
    """`overflow` is the exact surplus -- the rows of every frame of the result with room beyond `cap`, summed; the rows that fit are
    the first rows of the result with room, in every frame; the id counter is that of the result with room; nothing is written outside
    the tables (every table of the call lies between guard bands)"""
    from tests.guarded_alloc import guarded

    scene = _scene(name)
    with guarded() as g:
        res = _device(TS.batch([scene]), cap)
        assert g.check() > 0
    got, roomy = _np(res), _host(name)
    _assert_equal(got, _host(name, cap), (name, cap))
    surplus = int(np.maximum(roomy["n_out"][0].astype(np.int64) - cap, 0).sum())
    assert surplus > 0 and int(got["overflow"][0]) == surplus
    assert int(got["id_counter"][0]) == int(roomy["id_counter"][0])
    for t in range(len(scene["n_det"])):
        n = min(int(roomy["n_out"][0, t]), cap)
        assert int(got["n_out"][0, t]) == n, t
        for k, blank in (("track_ids", -1), ("src", -1), ("is_fill", 0)):
            assert np.array_equal(got[k][0, t, :n], roomy[k][0, t, :n]) and (got[k][0, t, n:] == blank).all(), (t, k)
        for k in ("pos_world", "rot_world"):
            assert np.allclose(got[k][0, t, :n], roomy[k][0, t, :n], rtol=0, atol=1e-9), (t, k)


def test_getters_raise_on_overflow_with_the_needed_capacity():
    from liso_amd._lib import LisoHipError
    from liso_amd.tracker.device_tracker import DeviceFlowBasedBoxTracker

    tr = DeviceFlowBasedBoxTracker(use_propagated_boxes=True, box_matching_threshold_m=2.0, capacity=23)
    tr.test_device = "cuda"
    TS.run_host_class(_scene("story"), tr)
    with pytest.raises(LisoHipError, match=f"capacity {_cap(_scene('story'))} always suffices"):
        tr.get_boxes_in_world_coordinates()


def test_frames_without_attributes_list_none_per_box():
    from liso_amd.tracker.device_tracker import DeviceFlowBasedBoxTracker

    tr = DeviceFlowBasedBoxTracker(use_propagated_boxes=True, box_matching_threshold_m=2.0)
    tr.test_device = "cuda"
    TS.run_host_class(_scene("T3_all_lost"), tr, attributes=False)
    listed = tr.get_extra_attributes_at_each_timestamp()
    assert [len(a) for a in listed] == [3, 6, 6] and all(v is None for a in listed for v in a)  # detections + the boxes carried into frame 1


def test_sizes_the_lds_plan_cannot_hold_are_refused():
    from liso_amd._lib import LisoHipError

    with pytest.raises(LisoHipError, match="sizes refused"):
        _device(TS.batch([_scene("T1")]), 1025)


def test_smoothing_tables_equal_those_built_from_the_host_getters():
    from liso_amd.tracker.global_box_tracker import FlowBasedBoxTracker

    scene = _scene("story")
    tr = TS.run_host_class(scene, FlowBasedBoxTracker(use_propagated_boxes=True, box_matching_threshold_m=TS.THRESHOLD, tie_order="stable"))
    world, T, M = tr.get_boxes_in_world_coordinates(), len(scene["n_det"]), 32
    want_ids, want_lens = tr.get_all_unique_track_ids_and_lengths()
    res = _device(TS.batch([scene]), _cap(scene))
    ids, lens, rows, n_tracks = (v[0].cpu().numpy() for v in res.track_table(M))
    pos, yaw, valid, start = (v[0].cpu().numpy() for v in res.observed_for_smoothing(M))
    n = len(want_ids)
    assert int(n_tracks) == n <= M and np.array_equal(ids[:n], want_ids.numpy()) and (ids[n:] == -1).all()
    assert np.array_equal(lens[:n], want_lens.numpy()) and not lens[n:].any() and not valid[n:].any()
    for i, tid in enumerate(want_ids.tolist()):
        box_idxs, first = tr.get_box_indices_start_time_for_track_id(tid)
        first, length = int(first), len(box_idxs)
        assert int(start[i]) == first and np.array_equal(rows[i, first:first + length], box_idxs.numpy())
        assert (rows[i, :first] == -1).all() and (rows[i, first + length:] == -1).all()
        assert valid[i, :length].all() and not valid[i, length:].any() and not pos[i, length:].any() and not yaw[i, length:].any()
        for c, k in enumerate(box_idxs.tolist()):
            assert np.allclose(pos[i, c], world[first + c].pos[k].numpy(), rtol=0, atol=1e-9)
            assert np.allclose(yaw[i, c], world[first + c].rot[k].numpy(), rtol=0, atol=1e-9)
