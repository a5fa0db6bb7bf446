"""CPU: the numpy restatement of the detector validation matching (liso_amd/eval/det_validation.py) on the library's host pair
matrices reproduces the reference fixture, each case as ONE padded batch, with the assertions of tests/test_gpu_od_metrics.py.

The fixture's decisions have room (measured on the CPU oracle): no IoU closer than 1.3e-3 to a threshold, no two candidates of a
prediction closer than 4e-2, no radius or coordinate closer than 2.7e-2 m to a bin or area edge, distinct scores -- last-bit
differences between pair implementations cannot flip one."""
import numpy as np
import pytest

from tests.det_val_cases import assert_fixture, fixture_batch, fixture_validator, pad_batch, scene


@pytest.mark.parametrize("tag", ["bev", "i3d"])
def test_host_path_reproduces_reference_fixture(golden_dir, tag):
    g = np.load(f"{golden_dir}/od_metrics_reference.npz")
    gt, pred = fixture_batch(g, tag)
    sizes = [(int(a), int(b)) for a, b in zip(gt.valid.sum(1), pred.valid.sum(1))]
    if tag == "bev":
        assert (5, 0) in sizes and (0, 7) in sizes
    v = fixture_validator(tag)
    v.update_batch_host(gt, None, pred)
    assert_fixture(v, g, tag)


def test_host_restatement_conventions():
    """slots, padding, match order, stable ties and the class transfer of `match_detections_host` on a hand-made frame"""
    from liso_amd.eval.det_validation import FilterSet, JobTable, match_detections_host, pack_boxes

    def box(x, y, cls=0, score=1.0):
        return dict(pos=np.float32([[x, y, 0]]), dims=np.float32([[4, 2, 1.5]]), rot=np.float32([[0]]), probs=np.float32([[score]]),
                    velo=np.zeros((1, 1), np.float32), class_id=np.int64([[cls]]), valid=np.ones(1, bool))

    cat = lambda bs: {k: np.concatenate([b[k] for b in bs]) for k in bs[0]}  # noqa: E731
    gt = pad_batch([cat([box(10, 0, 1), box(20, 0, 2), box(30, 0, 1)])])
    # two predictions of EQUAL score on the first box (the lower slot is visited first and takes it), one on the box at (20, 0)
    pred = pad_batch([cat([box(20.2, 0, 0, 0.5), box(10.4, 0, 0, 0.9), box(10.2, 0, 0, 0.9), box(50, 5, 0, 0.99)])])
    t = JobTable()
    f_all, f_near, f_mid, f_c2 = (t.add_filter(FilterSet()), t.add_filter(FilterSet(range=(0, 20))), t.add_filter(FilterSet(range=(20, 40))),
                                  t.add_filter(FilterSet(class_id=2)))
    jobs = [t.add_job(f_all, "iou_bev", 0.5), t.add_job(f_near, "iou_bev", 0.5), t.add_job(f_mid, "dist", 1.0), t.add_job(f_c2, "iou_3d", 0.25)]
    pk = lambda s: {k: v.numpy() for k, v in pack_boxes(s).items()}  # noqa: E731
    o = match_detections_host(pk(gt), pk(pred), t, class_draws=np.zeros((1, 4), np.int64))
    assert o["order"][0].tolist() == [3, 1, 2, 0]
    assert o["pred_class"][0].tolist() == [2, 1, 0, 0]  # matched ones take the ground truth's class, the others their draw
    assert o["count"][0].tolist() == [2, 1, 1, 1]
    assert o["pairs"][0, jobs[0]].tolist() == [[0, 1], [1, 0], [-1, -1]]
    assert o["pairs"][0, jobs[1]].tolist() == [[0, 1], [-1, -1], [-1, -1]]
    assert o["gt_in"][0, f_near].tolist() == [1, 0, 0] and o["gt_in"][0, f_mid].tolist() == [0, 1, 1]  # r = 20 belongs to 20-40 m
    assert o["pairs"][0, jobs[2], 0].tolist() == [1, 0] and o["pairs"][0, jobs[3], 0].tolist() == [1, 0]
    assert o["pred_in"][0, f_c2].tolist() == [1, 0, 0, 0]
    ate = np.float32(20.2) - np.float32(20)
    assert o["sums"][0, jobs[2]].tolist() == [float(np.sqrt(ate * ate)), 0.0, 0.0]


def test_validator_rejects_what_it_cannot_match():
    from liso_amd.eval.det_validation import Collection, DetectionValidator

    with pytest.raises(NotImplementedError):
        DetectionValidator.for_run_val("nuscenes")
    with pytest.raises(ValueError):
        DetectionValidator([Collection("", "other", dict(moving_velocity_thresh=0.1))])
    v = DetectionValidator.for_run_val("kitti", ("car", "ped"), (0, 1))
    assert len(v.collections) == 25 and len(v.tables["gt"].jobs) == 32 + 32 + 8 and len(v.tables["benchmark"].jobs) == 32
    s = scene(np.random.default_rng(0), 3, 4, 2)
    with pytest.raises(ValueError):
        v.update_batch_host(pad_batch([s[0]]), None, pad_batch([s[1]]))
