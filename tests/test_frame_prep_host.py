"""CPU: `prepare_tracker_frames_host` (liso_amd/tracker/frame_prep.py), the yardstick of tests/test_gpu_frame_prep.py, against
tests/golden/frame_prep_reference.npz -- the reference's own functions run frame by frame on the sequences of tests/frame_prep_cases.py
(tests/golden/make_frame_prep_golden.py).

Integer tables and decisions identical; fp32 columns copied from the input bitwise; mean flow within 5e-6 m (the project's bound for fp32
sums against another order of summation, tests/test_gpu_tracking.py); pose translations within the same 5e-6, rotation entries within
1e-9; the aligned heading within 1e-4 rad: |d angle| <= |d t| / |t| with |d t| <= sqrt(3) * 5e-6 m and |t| > 0.1 m wherever the alignment
ratio is not zero.  The displacement in `velo` inherits the translation's bound.  The restatement runs with the margins of
frame_prep_cases.MARGINS: no quantity decides within them.

Also: the two torch mirrors of liso/kabsch/shape_utils.py on the CPU against the same fixture, and their names under `install_as`."""
import functools
import os

import numpy as np
import pytest
import torch

import frame_prep_cases as FC

GOLD = os.path.join(os.path.dirname(__file__), "golden", "frame_prep_reference.npz")
CASES = [(s, c) for s in ("A", "B", "W") for c in FC.CONFIGS]
EXACT = ("n_det", "src", "in_fov", "n_points", "dropped_bev", "dropped_points")
FLOW_TOL, ROT_ENTRY_TOL, HEADING_TOL = 5e-6, 1e-9, 1e-4


@functools.lru_cache(maxsize=None)
def gold():
    g = np.load(GOLD)
    return {k: g[k] for k in g.files}


def reference(name, cfg):
    return {k[len(f"{name}_{cfg}_"):]: v for k, v in gold().items() if k.startswith(f"{name}_{cfg}_")}


@functools.lru_cache(maxsize=None)
def host(name, cfg):
    from liso_amd.tracker.frame_prep import prepare_tracker_frames_host

    return prepare_tracker_frames_host(*FC.args_of(FC.batch(name)), cap=FC.SHAPES[name][1], **FC.config(cfg), **FC.MARGINS)


def assert_matches_reference(got, want, what):
    """`got`: the tables of one sequence (no leading S) from the restatement or the device; `want`: the fixture's"""
    for k in EXACT:
        assert np.array_equal(got[k], want[k]), (what, k)
    assert got["boxes"][..., :6].tobytes() == want["boxes"][..., :6].tobytes() and got["conf"].tobytes() == want["conf"].tobytes(), what
    assert np.abs(got["mean_flow"] - want["mean_flow"]).max() <= FLOW_TOL, what
    for k in ("into_prev", "into_next"):
        assert np.abs(got[k][..., :3, 3] - want[k][..., :3, 3]).max() <= FLOW_TOL, (what, k)
        assert np.abs(got[k][..., :3, :3] - want[k][..., :3, :3]).max() <= ROT_ENTRY_TOL, (what, k)
        assert np.array_equal(got[k][..., 3, :], want[k][..., 3, :]), (what, k)
    assert np.abs(got["rot"] - want["rot"]).max() <= HEADING_TOL and got["rot"].dtype == np.float64, what
    assert np.abs(got["boxes"][..., 6].astype(np.float64) - want["boxes"][..., 6]).max() <= HEADING_TOL, what
    assert np.abs(got["velo"] - want["velo"]).max() <= 2 * FLOW_TOL, what


def test_the_fixture_was_generated_on_these_inputs():
    for name in ("A", "B", "W"):
        assert FC.checksum(name) == float(gold()[f"{name}_checksum"]), name


@pytest.mark.parametrize("name,cfg", CASES)
def test_host_restatement_equals_the_reference(name, cfg):
    got = {k: v[0] for k, v in host(name, cfg).items()}
    assert got["overflow"] == 0
    assert_matches_reference(got, reference(name, cfg), (name, cfg))


def test_the_planted_cases_decide_as_described():
    f, k = reference("A", "filter"), reference("A", "keep_all")
    assert f["src"][0].tolist() == [0, 1, 3, 6, 7, -1, -1, -1] and f["dropped_bev"][0] == 1 and f["dropped_points"][0] == 2
    assert f["in_fov"][0].tolist() == [1, 1, 1, 1, 0, 0, 0, 0]  # the box behind the sensor is kept, outside the field of view
    assert f["n_points"][0].tolist()[:5] == [12, 5, 9, 12, 12] and not f["mean_flow"][0, 3].any()  # all of its points are invalid
    assert k["n_det"].tolist() == [8, 6, 8, 4, 3] and k["n_points"][0, 5] == 0  # the box without a point: its propagated poses are its pose
    assert np.array_equal(k["into_next"][0, 5], k["into_prev"][0, 5]) and not k["mean_flow"][0, 5].any()
    assert f["n_det"].tolist() == [5, 6, 8, 0, 3] and f["dropped_points"][3] == 4  # the sweep without a point
    disp = f["velo"][1, :4, 0]
    assert np.allclose(disp, [0.05, 0.2, 0.5, 0.2], atol=5e-3)
    turned = f["rot"][1, :4] - f["raw_yaw"][1, :4].astype(np.float64)
    assert turned[0] == 0.0 and abs(abs(turned[3]) - np.pi) < 0.1 and np.abs(turned[1:3]).max() < 0.1
    w = reference("W", "filter")
    assert w["n_det"][0] == 47 and w["src"][0, 46] == 69 and reference("B", "filter")["n_det"].tolist() == [4, 0, 7, 0, 0]
    assert not reference("A", "flow_cluster")["velo"].any()


def test_margins_raise_and_device_means_are_taken_as_given():
    from liso_amd.tracker.frame_prep import prepare_tracker_frames_host

    args, cfg = FC.args_of(FC.batch("A")), FC.config("filter")
    with pytest.raises(AssertionError, match="displacement within the margin"):
        prepare_tracker_frames_host(*args, cap=8, **cfg, margin=0.2)  # (0.2 m and 0.5 m are planted: both within 0.2 of 0.3)
    with pytest.raises(AssertionError, match="box face"):
        prepare_tracker_frames_host(*args, cap=8, **cfg, face_margin=0.2)
    given = np.full((1, FC.T, 8, 3), 0.25, np.float32)
    got = prepare_tracker_frames_host(*args, cap=8, **cfg, mean_flow=given)
    n = int(got["n_det"][0, 1])
    assert (got["mean_flow"][0, 1, :n] == 0.25).all() and not got["mean_flow"][0, 1, n:].any()
    assert np.array_equal(got["into_next"][0, 1, :n, :3, 3], got["boxes"][0, 1, :n, :3].astype(np.float64) + 0.25)
    tight = prepare_tracker_frames_host(*args, cap=4, **cfg)
    roomy = host("A", "filter")
    assert tight["overflow"].tolist() == [int(np.maximum(roomy["n_det"][0] - 4, 0).sum())] and tight["n_det"].max() == 4
    assert np.array_equal(tight["src"], roomy["src"][:, :, :4])


@pytest.mark.parametrize("name", ["A", "B", "W"])
def test_torch_mirrors_on_the_cpu_equal_the_reference(name):
    """extract_motion_in_pred_box_coordinates and soft_align_box_flip_orientation_with_motion_trafo on the fixture's kept boxes with the
    reference's own mean flows: the translation within 1e-9, the heading within 1e-9 (the same arithmetic in the same library), the
    heading's type float64"""
    from liso_amd.kabsch.shape_utils import Shape, extract_motion_in_pred_box_coordinates, soft_align_box_flip_orientation_with_motion_trafo

    want, sc = reference(name, "filter"), FC.scene(name)
    for t in range(sc["n_frames"]):
        n = int(want["n_det"][t])
        if n == 0:
            continue
        b = torch.from_numpy(want["boxes"][t, :n].copy())
        boxes = Shape(pos=b[:, :3], dims=b[:, 3:6], rot=torch.from_numpy(want["raw_yaw"][t, :n, None].copy()),
                      probs=torch.from_numpy(want["conf"][t, :n, None].copy()))[None]
        fg = torch.eye(4, dtype=torch.float64).repeat(1, n, 1, 1)
        fg[0, :, :3, 3] = torch.from_numpy(want["mean_flow"][t, :n]).double()
        bg = torch.linalg.inv(torch.from_numpy(sc["odom"][t].copy()))[None, None]
        trans, _ = extract_motion_in_pred_box_coordinates(boxes, fg, bg)
        assert np.abs(trans[0].numpy() - want["box_translation"][t, :n]).max() <= 1e-9
        out = soft_align_box_flip_orientation_with_motion_trafo(boxes, fg, bg)
        assert out.rot.dtype == torch.float64 and np.abs(out.rot[0, :, 0].numpy() - want["rot"][t, :n]).max() <= 1e-9
        assert np.abs(out.velo[0].numpy() - want["velo"][t, :n]).max() <= 1e-9


def test_the_mirrors_are_reachable_under_the_reference_names():
    import liso_amd

    liso_amd.install_as("liso")
    from liso.eval.eval_ours import count_box_points_in_kitti_annotated_fov  # noqa: F401
    from liso.kabsch.shape_utils import extract_motion_in_pred_box_coordinates, soft_align_box_flip_orientation_with_motion_trafo  # noqa: F401
    from liso.tracker.frame_prep import prepare_tracker_frames  # noqa: F401
