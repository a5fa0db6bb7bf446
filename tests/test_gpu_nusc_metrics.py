"""The per-frame part of the nuScenes detection metrics on the device (include/liso_nusc_metrics.h: liso_det_val_nusc_f32): bitwise
agreement with the numpy restatement from empty sets to 1024 x 1000 boxes, the devkit fixture through `update_batch` -> `compute()`,
run_val with the flag against the per-frame `update()` path, graph capture and bounds."""
import numpy as np
import pytest
import torch

from tests.nusc_metrics_cases import assert_fixture, fixture_metric, fixture_shapes, kernel_batch, kernel_host

pytestmark = pytest.mark.gpu

SHAPES = ((0, 5), (5, 0), (1, 1), (17, 70), (64, 65), (130, 129), (1024, 1000))
OUT = ("count", "pairs", "err", "gt_in", "pred_in")


def _device(b, as_one, thresholds=(0.5, 1.0, 2.0, 4.0)):
    from liso_amd import det_nms as D
    from liso_amd.eval.nuscenes_metrics import nusc_match_packed

    t = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    g = {"rows": t(b["gt"]), "valid": t(b["gv"]), "cls": t(b["gc"])}
    p = {"rows": t(b["pred"]), "valid": t(b["pv"]), "cls": t(b["pc"])}
    F, P = b["pv"].shape
    order = D.order(t(b["score"]), None, p["valid"], None)[1] if F and P else torch.zeros((F, P), dtype=torch.int32, device="cuda")
    return (g, p, order, t(b["radius"])), nusc_match_packed(g, p, order, t(b["radius"]), as_one, thresholds)


def _same(dev, host, what):
    for k in OUT:
        d = dev[k].cpu().numpy()
        assert d.shape == host[k].shape and d.dtype == host[k].dtype, (what, k, d.shape, host[k].shape, d.dtype, host[k].dtype)
        assert d.tobytes() == host[k].tobytes(), (what, k)


@pytest.mark.parametrize("as_one", [True, False])
@pytest.mark.parametrize("G,P", SHAPES)
def test_device_equals_the_restatement_bitwise(G, P, as_one):
    b = kernel_batch(100 + G + P, 3, G, P)
    (_, _, order, _), dev = _device(b, as_one)
    torch.cuda.synchronize()
    host_order, host = kernel_host(b, as_one)
    if G and P:
        assert np.array_equal(order.cpu().numpy(), host_order)
    _same(dev, host, (G, P, as_one))
    cnt = host["count"]
    assert cnt.shape == (3, 4) and (np.diff(cnt, axis=1) >= 0).all()  # a wider threshold never matches fewer
    if min(G, P) >= 17:
        assert cnt[:, 0].sum() > 0 and cnt[:, 3].max() > cnt[:, 0].max() and host["gt_in"].sum() < b["gv"].sum()  # the radii cut some
        assert not host["gt_in"][0, 1] and not host["pred_in"][0, 1]  # the NaN centres
        assert as_one or not (host["gt_in"][0, 2] or host["pred_in"][0, 2])  # class ids outside the table
    if (G, P) == (1024, 1000):
        assert cnt[:, 3].min() > 100 and (host["pairs"][:, 3, :, 0].max(axis=1) > 960).all()  # all 16 slots of a lane take part


@pytest.mark.parametrize("as_one", [True, False])
def test_fixture_through_update_batch_and_compute(golden_dir, as_one):
    from liso_amd.eval.det_validation import Collection, DetectionValidator

    g = np.load(f"{golden_dir}/nusc_metrics.npz")
    gt, pred = fixture_shapes(g)
    m = fixture_metric(g, as_one)
    kw = dict(eval_movable_classes_as_one=as_one, class_names=m.class_names, class_ranges=m.class_ranges)
    # The devkit was fed the HOST's fp32 sigmoid of the logits (the generator says so).  torch.sigmoid on the device may differ from it
    # in the last bit, and the confidence curve is compared exactly: the probabilities go in as the host computed them ...
    logits = pred.probs
    pred.probs = torch.sigmoid(logits)
    v = DetectionValidator([Collection("nusc/", "gt", dict(kw, sigmoid_scores=False), "nusc")])
    v.update_batch(gt[:7].to("cuda"), None, pred[:7].to("cuda"))
    v.update_batch(gt[7:].to("cuda"), None, pred[7:].to("cuda"))
    assert all(torch.is_tensor(t) and t.is_cuda for r in v._pending for t in r["gt"].values())  # nothing read back yet
    res = v.compute("val/")
    r = assert_fixture(v.metrics[0], g, as_one)
    assert res["val/nusc/mAP"] == r["mean_ap"] and res["val/nusc/NDS"] == r["nd_score"]
    # ... and the collection's own sigmoid, applied on the device, gives what the host path gives on the device's probabilities
    dev_probs = torch.sigmoid(logits.to("cuda")).cpu()
    pred.probs = logits
    s = DetectionValidator([Collection("nusc/", "gt", dict(kw, sigmoid_scores=True), "nusc")])
    s.update_batch(gt.to("cuda"), None, pred.to("cuda"))
    got = s.compute("val/")
    pred.probs = dev_probs
    host = DetectionValidator([Collection("nusc/", "gt", dict(kw, sigmoid_scores=False), "nusc")])
    host.update_batch_host(gt, None, pred)
    want = host.compute("val/")
    assert set(want) == set(got) and all(got[k] == want[k] for k in want), {k: (got[k], want[k]) for k in want}


@pytest.mark.parametrize("kind", ["kitti", "nuscenes"])
def test_run_val_with_the_flag_equals_the_per_frame_path(kind):
    from liso_amd.eval.det_validation import DetectionValidator
    from liso_amd.eval.eval_ours import run_val
    from liso_amd.eval.nuscenes_metrics import NuscenesObjectDetectionMetrics
    from tests.det_val_cases import pad_batch, shape_of
    from tests.test_gpu_det_val import SEED, _transfer_host, val_set

    gts, bms, preds, _ = val_set(SEED)
    names = ("car", "pedestrian", "bicycle")
    batch = {"pcls": None, "gt_boxes": pad_batch(gts).to("cuda"), "benchmark_gt_boxes": pad_batch(bms).to("cuda")}
    pred = pad_batch(preds).to("cuda")

    class Predictor:
        def predict_boxes(self, _, pcls, logit_threshold):
            return pred.clone(), None, None
    sig = kind == "nuscenes"
    gen = lambda: torch.Generator(device="cuda").manual_seed(11)  # noqa: E731
    got = run_val({}, [batch], Predictor(), "val/", dataset_kind=kind, movable_class_names=names, generator=gen(), nuscenes_metrics=True,
                  sigmoid_scores=sig)
    draws = torch.randint(0, 3, tuple(pred.valid.shape), device="cuda", generator=gen(), dtype=torch.int32).cpu()  # the validator's own draw
    tags = {"final_result/NUSC_OFFICIAL/detection_metrics/": NuscenesObjectDetectionMetrics(True, sigmoid_scores=sig)}
    if kind == "nuscenes":
        tags["final_result/NUSC_OFFICIAL/per_class/detection_metrics/"] = NuscenesObjectDetectionMetrics(False, class_names=names, sigmoid_scores=sig)
    for f in range(len(preds)):
        gt = shape_of(gts[f]).to("cuda")
        p = _transfer_host(gt, shape_of(preds[f]).to("cuda"), draws[f, : len(preds[f]["valid"])])
        for m in tags.values():
            m.update(non_batched_gt_boxes=gt, non_batched_pred_boxes=p, sample_token=str(f))
    want = {}
    for tag, m in tags.items():
        want.update(m.compute("val/" + tag))
    assert len(want) == (13 if kind == "kitti" else 13 + 7 + 3 * 6)
    assert {k for k in got if "NUSC_OFFICIAL" in k} == set(want) and all(got[k] == w for k, w in want.items()), {k: (got[k], w) for k, w in want.items()}
    assert got["val/final_result/NUSC_OFFICIAL/detection_metrics/mAP"] > 0.1 and 0 < got["val/final_result/NUSC_OFFICIAL/detection_metrics/mATE"] < 1
    if kind == "kitti":  # the other collections' results are what they are without the flag
        off = run_val({}, [batch], Predictor(), "val/", dataset_kind=kind, movable_class_names=names, generator=gen())
        same = lambda a, b: a == b or (np.isnan(a) and np.isnan(b))  # noqa: E731
        assert set(got) - set(off) == set(want) and all(same(got[k], x) for k, x in off.items())
    else:
        assert got["val/final_result/NUSC_OFFICIAL/per_class/detection_metrics/car/AP"] > 0.05
        v = DetectionValidator.for_run_val(kind, names, (0, 1, 2), nuscenes_metrics=True)
        assert sum(c.kind == "nusc" for c in v.collections) == 2


@pytest.fixture(scope="module")
def mid():
    b = kernel_batch(7, 3, 130, 129)
    args, dev = _device(b, False)
    torch.cuda.synchronize()
    return b, args, {k: v.cpu().numpy() for k, v in dev.items()}


def test_captured_replay_equals_the_eager_call(mid):
    """(a capture also shows there is no host sync and no allocation outside the graph's pool)"""
    from liso_amd.eval.nuscenes_metrics import nusc_match_packed
    from liso_amd.utils.graph_capture import capture

    _, (g, p, order, radius), eager = mid
    stream = torch.cuda.Stream()
    graph, out = capture(lambda: nusc_match_packed(g, p, order, radius, False), stream, warm_ups=2)
    for k in OUT:
        out[k].fill_(7)  # (the replay, not the capture, fills the tables)
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        graph.replay()
    stream.synchronize()
    _same(out, eager, "replay")


def test_nothing_is_written_outside_the_outputs(mid):
    from liso_amd.eval.nuscenes_metrics import nusc_match_packed
    from tests.guarded_alloc import guarded

    _, (g, p, order, radius), eager = mid
    with guarded() as guard:
        out = nusc_match_packed(g, p, order, radius, False)  # every output at its exact size between guard bands
        assert guard.check() == 5
    _same(out, eager, "guarded")
    for G, P in ((0, 3), (3, 0), (1, 1), (64, 65), (129, 64), (1024, 1000)):
        b = kernel_batch(G + P, 2, G, P)
        with guarded() as guard:
            _, o = _device(b, True, thresholds=(0.5, 1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0))  # the largest threshold table
            guard.check()
        assert o["pairs"].shape == (2, 8, min(G, P), 2) and int(o["count"].max()) <= min(G, P)
