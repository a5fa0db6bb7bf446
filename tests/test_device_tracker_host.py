"""`track_sequences_host` (liso_amd/tracker/device_tracker.py), the numpy yardstick of the device tracker, against the host class it
restates: `FlowBasedBoxTracker(tie_order="stable")` on the four golden sequences and on generated ones -- track ids, id counter and
hole-filling rows exactly, world boxes within the tolerances of tests/test_tracker_sequence.py (1e-9 for fp64, 1e-6 for fp32).  And
the option itself: with the stable order the golden ids of cases a, b, d come out (at most 9 boxes per frame); `tie_order=None` is
still the old call (case c, whose golden ids depend on torch.argsort's order of equal confidences, still reproduces).  No GPU."""
import numpy as np
import pytest
import torch

import tracker_scenes as TS

CASES = [str(c) for c in TS.G["cases"]]
SCENES = TS.generated_scenes()


def _scene(name):
    return TS.golden_scene(name) if name in CASES else SCENES[name]


def _host_class(scene, tie_order):
    from liso_amd.tracker.global_box_tracker import FlowBasedBoxTracker

    return TS.run_host_class(scene, FlowBasedBoxTracker(use_propagated_boxes=True, box_matching_threshold_m=TS.THRESHOLD, tie_order=tie_order))


@pytest.mark.parametrize("name", CASES + sorted(SCENES))
def test_host_restatement_equals_the_host_class_with_the_stable_order(name):
    from liso_amd.tracker.device_tracker import needed_capacity, track_sequences_host

    scene = _scene(name)
    tr = _host_class(scene, "stable")
    cap = needed_capacity(scene["n_det"])
    got = track_sequences_host(**TS.batch([scene]), threshold=TS.THRESHOLD, cap=cap, margin=None if name in CASES else 1e-3)
    assert int(got["overflow"][0]) == 0 and int(got["id_counter"][0]) == int(tr.max_track_id_counter)
    world = tr.get_boxes_in_world_coordinates()
    for t, ids in enumerate(tr.track_ids):
        n, n_det = len(ids), int(scene["n_det"][t])
        assert int(got["n_out"][0, t]) == n, (t, got["n_out"][0, t], n)
        assert np.array_equal(got["track_ids"][0, t, :n], ids.numpy()) and (got["track_ids"][0, t, n:] == -1).all(), t
        assert np.array_equal(got["is_fill"][0, t, :n], (np.arange(n) >= n_det).astype(np.uint8)), t
        assert world[t].pos.dtype == torch.float64 and world[t].rot.dtype == torch.float64
        assert np.allclose(got["pos_world"][0, t, :n], world[t].pos.numpy(), rtol=0, atol=1e-9), t
        assert np.allclose(got["rot_world"][0, t, :n], world[t].rot.numpy()[:, 0], rtol=0, atol=1e-9), t
        # `src` names the detection whose attributes the row carries (the host class lists the attributes of a frame's detections and
        # then those of EVERY box carried into the frame, hole-filling or not)
        src = got["src"][0, t, :n]
        uids, listed = [1000 * int(a) + int(k) for a, k in src], [d["uid"] for d in tr.get_extra_attributes_at_each_timestamp()[t]]
        assert uids[:n_det] == listed[:n_det] and set(uids[n_det:]) <= set(listed[n_det:]), t
        assert np.allclose(scene["boxes"][src[:, 0], src[:, 1], 3:6], world[t].dims.numpy(), rtol=0, atol=1e-6), t
        assert np.allclose(scene["conf"][src[:, 0], src[:, 1]], world[t].probs.numpy()[:, 0], rtol=0, atol=1e-6), t
    assert np.allclose(got["w_T_sensor"][0], tr.w_Ts_sti.numpy()[:len(tr.track_ids)], rtol=0, atol=1e-9)


@pytest.mark.parametrize("tag", ["a", "b", "d"])
def test_stable_order_reproduces_the_golden_ids(tag):
    tr = _host_class(TS.golden_scene(tag), "stable")
    for t, want in enumerate(TS.golden_frames(f"{tag}_flow", "ids")):
        assert np.array_equal(tr.track_ids[t].numpy(), want), (t, tr.track_ids[t], want)
    assert int(tr.max_track_id_counter) == int(TS.G[f"{tag}_flow_counter"])


def test_default_tie_order_is_the_old_call(monkeypatch):
    """case c through the default: the ids are the golden ones, and the order came from the call the reference makes -- torch.argsort
    without `stable`"""
    calls = []
    real = torch.argsort

    def spy(*args, **kwargs):
        calls.append(kwargs)
        return real(*args, **kwargs)

    monkeypatch.setattr(torch, "argsort", spy)
    tr = _host_class(TS.golden_scene("c"), None)
    monkeypatch.undo()
    assert calls and all(kw == {"descending": True} for kw in calls), calls[:3]
    for t, want in enumerate(TS.golden_frames("c_flow", "ids")):
        assert np.array_equal(tr.track_ids[t].numpy(), want), t
    calls.clear()
    monkeypatch.setattr(torch, "argsort", spy)
    _host_class(TS.golden_scene("a"), "stable")
    assert calls and all(kw == {"descending": True, "stable": True} for kw in calls)


def test_story_scene_tells_its_stories():
    """the generated `story` sequence holds what its description promises, so that the device tests that use it test those cases"""
    from liso_amd.tracker.device_tracker import needed_capacity, track_sequences_host

    scene = SCENES["story"]
    got = track_sequences_host(**TS.batch([scene]), threshold=TS.THRESHOLD, cap=needed_capacity(scene["n_det"]), margin=1e-3)
    fills = [(t, int(i)) for t in range(8) for i in got["track_ids"][0, t][got["is_fill"][0, t] == 1]]
    assert len(fills) >= 3 and any(t == 1 for t, _ in fills)  # object 17's hole, and the loser of each pair competition
    ids_per_frame = [set(got["track_ids"][0, t, :got["n_out"][0, t]].tolist()) for t in range(8)]
    born_late = set.union(*ids_per_frame[1:]) - ids_per_frame[0]
    assert len(born_late) == 2  # object 18 under a new id and object 19; the pairs swap or keep their ids but found no track
    assert min(int(n) for n in scene["n_det"]) >= 17  # at least 17 alive rows of confidence 1 in every frame


def test_kernel_constants_are_those_of_the_host_tracker():
    """the kernel takes its propagation time and confidences from include/liso_tracking.h; they must be the host module's"""
    import os
    import re

    from liso_amd.tracker import device_tracker as D, global_box_tracker as H

    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "liso_tracking.h")).read()
    value = lambda name: float(re.search(rf"#define {name} ([0-9.]+)f?\n", header).group(1))  # noqa: E731
    assert value("LISO_TRACK_MAX_PROPAGATION_TIME") == H.MAX_PROPAGATION_TIME
    assert value("LISO_TRACK_INITIAL_CONF") == H.INITIAL_TRACK_CONF and value("LISO_TRACK_MIN_ALIVE_CONF") == H.MIN_ALIVE_TRACK_CONF
    assert value("LISO_TRACK_MAX_CAP") == D.MAX_CAP


def test_sizes_the_kernel_cannot_hold_are_einval_before_anything_is_launched():
    from liso_amd import _lib
    from liso_amd.tracker.device_tracker import MAX_CAP

    lib = _lib.lib()
    args = lambda cap: (1, 2, 3, cap) + (None,) * 7 + (2.0,) + (None,) * 10 + (0, None)  # noqa: E731
    assert lib.liso_track_sequences(*args(MAX_CAP + 1)) == -1 and lib.liso_track_sequences_workspace_bytes(1, 2, 3, MAX_CAP + 1) == 0
    assert lib.liso_track_sequences(*args(0)) == -1 and lib.liso_track_sequences_workspace_bytes(1, 2, 3, 0) == 0
    assert lib.liso_track_sequences(*args(MAX_CAP)) == -1  # (null tables: refused as well, nothing launched)
    assert lib.liso_track_sequences_workspace_bytes(1, 2, 3, MAX_CAP) > 0
    assert lib.liso_track_sequences_workspace_bytes(1 << 20, 1 << 10, 1 << 10, 8) == 0  # more detections than the grid can index


def test_device_class_refuses_what_it_cannot_run():
    from liso_amd.tracker.device_tracker import DeviceFlowBasedBoxTracker

    with pytest.raises(ValueError, match="use_propagated_boxes=True"):
        DeviceFlowBasedBoxTracker(use_propagated_boxes=False)
    with pytest.raises(ValueError, match="no frame"):
        DeviceFlowBasedBoxTracker(use_propagated_boxes=True).run_tracker()
