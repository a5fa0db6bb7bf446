"""CPU: pins the host restatements of the box-mining steps (oracle/flow_cluster.py: boxes_from_regions, mine_filter_compact,
box_motion, nms_prepare, nms_finish) on cases worked out by hand.  tests/test_gpu_box_mining.py compares every kernel of
liso_amd/csrc/box_mining.hip with them."""
import math

import numpy as np

from oracle import flow_cluster as OF


def test_boxes_from_regions_truncates_clips_by_the_smaller_extent_and_divides():
    rows = np.arange(6, dtype=np.float32) * 2 - 5   # gx = 6
    cols = np.arange(4, dtype=np.float32) * 3 + 100  # gy = 4: both indices are clipped to 3
    props = np.array([[2.9, 1.2, 0.3, 8.0, 2.0], [-0.5, 7.0, -1.0, 1.0, 0.5], [5.0, 3.5, 0.0, 0.0, 0.0]])
    center, dims, rot, dims32, rot32 = OF.boxes_from_regions(props, rows, cols, np.array([4.0, 2.0], np.float32))
    assert center.dtype == np.float32 and dims.dtype == np.float64 and dims32.dtype == np.float32 and rot32.dtype == np.float32
    assert center.tolist() == [[-1.0, 103.0], [-5.0, 109.0], [1.0, 109.0]]  # pillars (2, 1), (0, 3), (3 <- 5, 3)
    assert dims.tolist() == [[2.0, 1.0], [0.25, 0.25], [0.0, 0.0]] and rot.tolist() == [0.3, -1.0, 0.0]


def test_filter_three_boxes_one_failing_each_of_two_rules():
    """box 0 passes; box 1 is 8 m long (aspect 4 is allowed, the length is not); box 2 has a footprint of exactly the minimum
    (the rule is strict).  The survivor moves to slot 0, the other slots take the padding values."""
    center = np.array([[[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]]], np.float32)
    dims2 = np.array([[[4.0, 2.0], [8.0, 2.0], [0.5, 0.5]]])
    rot = np.array([[0.1, 0.2, 0.3]])
    cfg = dict(min_points=10, aspect_ratio_max=4.0, max_box_len_m=7.0, min_box_area_m2=0.25, min_box_volume_m3=0.25)
    args = ([3], center, dims2, rot, np.array([[10, 50, 50]]), np.array([[0.5, 0.6, 0.7]], np.float32), np.array([[1.5, 1.5, 1.5]], np.float32))
    o = OF.mine_filter_compact(*args, **cfg)
    assert o["counts"].tolist() == [1] and o["valid"].tolist() == [[1, 0, 0]]
    assert o["pos"][0].tolist() == [[1.0, 2.0, 0.5], [0, 0, 0], [0, 0, 0]] and o["dims"][0].tolist() == [[4.0, 2.0, 1.5], [0, 0, 0], [0, 0, 0]]
    assert o["rot"][0, :, 0].tolist() == [0.1, 0, 0] and o["probs"][0, :, 0].tolist() == [1, 0, 0] and not o["velo"].any()
    assert o["class_id"][0, :, 0].tolist() == [2**31 - 1, 2**31 - 2, 2**31 - 2] and o["difficulty"][0, :, 0].tolist() == [1, 2**31 - 2, 2**31 - 2]
    assert o["kabsch_pos"][0].tolist() == o["pos"][0].tolist() and o["kabsch_dims"][0, 0].tolist() == [4.0, 2.0, 1.5]
    assert {k: v.dtype.name for k, v in o.items()} == dict(
        pos="float32", dims="float64", rot="float64", probs="float64", velo="float64", valid="uint8", class_id="int32", difficulty="int32",
        counts="int32", kabsch_pos="float32", kabsch_dims="float32", kabsch_rot="float32")
    # each failing rule alone decides: lift it and the box survives, in label order behind box 0
    assert OF.mine_filter_compact(*args, **{**cfg, "max_box_len_m": 8.0})["valid"].tolist() == [[1, 1, 0]]
    o2 = OF.mine_filter_compact(*args, **{**cfg, "min_box_area_m2": np.nextafter(0.25, 0.0)}, park_invalid=True)
    assert o2["valid"].tolist() == [[1, 1, 0]] and o2["pos"][0, 1].tolist() == [5.0, 6.0, np.float32(0.7)]
    assert o2["kabsch_pos"][0, 2].tolist() == [1e6, 1e6, 1e6] and o2["pos"][0, 2].tolist() == [0, 0, 0]
    # a region that does not exist (label > num_labels) and one point too few
    assert OF.mine_filter_compact([0], *args[1:], **cfg)["counts"].tolist() == [0]
    assert OF.mine_filter_compact(*args, **{**cfg, "min_points": 11})["counts"].tolist() == [0]


def test_box_motion_of_a_pure_translation_in_closed_form():
    """background moves by (1, 0, 0), the box's points by (4, 4, 0): in the box frame, yaw 0.7, the motion is R(-0.7) (3, 4, 0) --
    speed 5, direction atan2(4, 3) - 0.7, so the new heading is atan2(4, 3) wherever the box stands"""
    T = np.tile(np.eye(4), (1, 3, 1, 1))
    T[0, 0, :3, 3] = [4.0, 4.0, 0.0]
    T[0, 1] = T[0, 2]                  # a box that moves with the background
    T[0, 1, :3, 3] = T[0, 2, :3, 3] = [1.0, 0.0, 0.0]
    rot, velo = OF.box_motion(T, np.array([[[20.0, -30.0, 1.0], [5.0, 5.0, 0.0]]], np.float32), np.array([[[0.7], [-2.0]]]))
    assert abs(float(rot[0, 0, 0]) - math.atan2(4.0, 3.0)) < 1e-13 and abs(float(velo[0, 0, 0]) - 5.0) < 1e-13
    assert float(velo[0, 1, 0]) < 1e-13 and rot.shape == (1, 2, 1) and velo.shape == (1, 2, 1)


def test_nms_prepare_orders_stably_with_nan_and_invalid_last():
    """confidences [1, 1, nan, 0.5, 1] with slot 1 invalid: keys [1, -inf, -inf, 0.5, 1] -> order [0, 4, 3, 1, 2]"""
    K = 5
    a = {"pos": np.arange(K * 3, dtype=np.float32).reshape(1, K, 3), "dims": np.arange(K * 3, dtype=np.float64).reshape(1, K, 3) + 0.5,
         "rot": np.arange(K, dtype=np.float64).reshape(1, K, 1) / 10, "probs": np.array([1.0, 1.0, np.nan, 0.5, 1.0]).reshape(1, K, 1),
         "velo": np.arange(K, dtype=np.float64).reshape(1, K, 1), "valid": np.array([[1, 0, 1, 1, 1]], np.uint8),
         "class_id": np.arange(K, dtype=np.int32).reshape(1, K, 1), "difficulty": np.arange(K, dtype=np.int32).reshape(1, K, 1) + 10}
    out, enters, dense = OF.nms_prepare(a, 2)
    assert out["class_id"][0, :, 0].tolist() == [0, 4, 3, 1, 2] and out["valid"].tolist() == [[1, 1, 1, 0, 1]]
    assert out["pos"][0, 1].tolist() == [12.0, 13.0, 14.0] and np.isnan(out["probs"][0, 4, 0])
    assert enters.tolist() == [[1, 1, 0, 0, 0]]  # the cut counts ranks: the NaN slot is valid but ranks behind the cut
    assert dense[0, 1].tolist() == [12.0, 13.0, 14.0, 12.5, 13.5, 14.5, np.float32(0.4)]
    assert dense[0, 3].tolist() == [1e6 + 30, 1e6, 0, np.float32(1e-3), np.float32(1e-3), np.float32(1e-3), 0]
    assert OF.nms_prepare(a, 0)[1].tolist() == [[1, 1, 1, 0, 1]] and OF.nms_prepare(a, 9)[1].tolist() == [[1, 1, 1, 0, 1]]
    # fp64 confidences closer than fp32 resolution are still sorted apart
    a["probs"] = np.array([0.5, 0.5 + 1e-12, 0.5, 0.5 + 2e-12, 0.5]).reshape(1, K, 1)
    a["valid"][:] = 1
    assert OF.nms_prepare(a, 0)[0]["class_id"][0, :, 0].tolist() == [3, 1, 0, 2, 4]


def test_nms_finish_keeps_the_first_max_boxes_survivors_of_one_sample():
    K = 4
    a = {"pos": np.ones((2, K, 3), np.float32), "dims": np.full((2, K, 3), 1e-4), "rot": np.full((2, K, 1), 0.5), "probs": np.ones((2, K, 1)),
         "velo": np.ones((2, K, 1)), "valid": np.array([[1, 1, 1, 1], [1, 1, 0, 1]], np.uint8),
         "class_id": np.zeros((2, K, 1), np.int32), "difficulty": np.zeros((2, K, 1), np.int32)}
    enters = np.array([[1, 1, 1, 1], [1, 0, 1, 1]], np.uint8)
    t = (np.full((2, K, 3), 7, np.float32), np.full((2, K, 3), 7, np.float32), np.full((2, K), 7, np.float32), np.full((2, K), 7, np.uint8))
    # kept indices: 3, a duplicate of it, -1, K (ignored), 1 (valid, did not enter), 2 (entered, invalid), 0 -- cut off by num = 6
    out, (t_pos, t_dims, t_rot, t_valid) = OF.nms_finish(1, a, enters, [3, 3, -1, K, 1, 2, 0], 6, 5, t)
    assert out["valid"].tolist() == [[1, 1, 1, 1], [0, 0, 0, 1]] and t_valid.tolist() == [[7] * 4, [0, 0, 0, 1]]
    assert out["class_id"][1, :, 0].tolist() == [2**31 - 2] * 3 + [0] and out["probs"][1, :, 0].tolist() == [0, 0, 0, 1]
    assert t_dims[1].tolist() == [[np.float32(1e-3)] * 3] * 4 and t_rot[1].tolist() == [0, 0, 0, 0.5] and t_pos[1, 3].tolist() == [1, 1, 1]
    assert (t_pos[0] == 7).all() and (out["dims"][0] == 1e-4).all()
    assert OF.nms_finish(1, a, enters, [3, 0, 0, 0], 4, 1, t)[0]["valid"][1].tolist() == [1, 0, 0, 0]  # slot order, not keep order
    for num in (0, -3):
        assert not OF.nms_finish(1, a, enters, [3, 0, 0, 0], num, 5, t)[0]["valid"][1].any()
    assert OF.nms_finish(1, a, enters, [3, 0, 0, 0], K + 5, 5, t)[0]["valid"][1].tolist() == [1, 0, 0, 1]
