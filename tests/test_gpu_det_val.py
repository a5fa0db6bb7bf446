"""Detector validation matching on the device (include/liso_det_val.h, liso_amd/eval/det_validation.py): the reference fixture,
bitwise agreement with the numpy restatement at the edges, the pair matrices, reproducibility, bounds, and the full run_val
collection set against the per-frame ObjectDetectionMetrics.update path."""
import numpy as np
import pytest
import torch

from tests.det_val_cases import assert_fixture, fixture_batch, fixture_validator, pad_batch, punch_holes, scene

pytestmark = pytest.mark.gpu

OUT = ("count", "pairs", "sums", "gt_in", "pred_in", "pred_class", "order")
MATS = ("iou_bev", "iou_3d", "dist")


def _np(o):
    return {k: v.cpu().numpy() for k, v in o.items()}


def _same(a, b, keys, what=""):
    for k in keys:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, (what, k, a[k].shape, b[k].shape, a[k].dtype, b[k].dtype)
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


def _table():
    from liso_amd.eval.det_validation import FilterSet, JobTable

    t = JobTable()
    sets = [FilterSet(), FilterSet(range=(0, 20)), FilterSet(range=(20, 40)), FilterSet(area=(-50, -20, 50, 20), range=(0, 1000)),
            FilterSet(class_id=1), FilterSet(area=(-50, -20, 50, 20), range=(40, 60), class_id=2), FilterSet(range=(2000, 3000))]
    for i, s in enumerate(sets):
        f = t.add_filter(s)
        for crit, thrs in (("iou_bev", (0.25, 0.5)), ("iou_3d", (0.3, 0.7)), ("dist", (0.5, 2.0))):
            for thr in thrs[: 2 if i < 4 else 1]:
                t.add_job(f, crit, thr)
    return t


def _one(x, y, score=0.5, cls=0, dims=(4.0, 2.0, 1.5), yaw=0.3):
    return dict(pos=np.float32([[x, y, -1.0]]), dims=np.float32([dims]), rot=np.float32([[yaw]]), probs=np.float32([[score]]),
                velo=np.zeros((1, 1), np.float32), class_id=np.int64([[cls]]), valid=np.ones(1, bool))


def _cat(bs):
    return {k: np.concatenate([b[k] for b in bs]) for k in bs[0]}


def _edge_frames():
    g = np.random.default_rng(11)
    frames = [scene(g, 0, 7, 3), scene(g, 5, 0, 3), scene(g, 0, 0, 3),
              scene(g, 65, 130, 3, spread=14.0)]  # crosses the wavefront in both directions, crowded: many candidates per row
    far = scene(g, 9, 12, 3)
    for side in far:
        side["pos"][:, 0] += 400.0  # outside every range bin and the area: everything filtered out of those sets
    frames.append(far)
    ties = scene(g, 20, 40, 3, spread=20.0)
    ties[1]["probs"] = np.round(ties[1]["probs"], 1)  # equal scores
    ties[1]["probs"][0] = 2.0  # (prediction 0 is visited first: both copies of the box are still free)
    ties[0]["pos"][1], ties[0]["dims"][1], ties[0]["rot"][1] = ties[0]["pos"][0], ties[0]["dims"][0], ties[0]["rot"][0]  # equal IoUs in a row
    ties[1]["pos"][0], ties[1]["dims"][0], ties[1]["rot"][0] = ties[0]["pos"][0], ties[0]["dims"][0], ties[0]["rot"][0]
    frames.append(ties)
    nan = scene(g, 10, 16, 3, spread=15.0)
    nan[0]["pos"][3, 0] = np.nan  # a NaN box, valid
    nan[1]["pos"][2, 2] = np.nan  # its 3-D IoUs are NaN; its BEV IoUs and distances are not
    frames.append(nan)
    # a box at (20, 0): r = 20 belongs to 20-40 m and not 0-20 m; boxes on the inclusive area bounds (50, -20) and just outside
    gt = _cat([_one(20.0, 0.0, cls=1), _one(50.0, -20.0, cls=2), _one(np.nextafter(np.float32(50), np.float32(60)), 0.0, cls=2), _one(0.0, 40.0, cls=1)])
    pr = _cat([_one(20.0, 0.0, 0.9, 1), _one(50.0, -20.0, 0.8, 2), _one(np.nextafter(np.float32(50), np.float32(60)), 0.1, 0.7, 2), _one(0.2, 40.0, 0.6, 1)])
    frames.append((gt, pr))
    return frames


@pytest.fixture(scope="module")
def edge():
    """the edge scenes as one padded batch with holes in both valid masks; the device result and its inputs, computed once"""
    from liso_amd.eval.det_validation import match_detections, pack_boxes

    frames = _edge_frames()
    g = np.random.default_rng(12)
    gt, pred = punch_holes(pad_batch([f[0] for f in frames]), g, 0.85), punch_holes(pad_batch([f[1] for f in frames]), g, 0.85)
    gt.valid[7, 0] = pred.valid[7, 0] = True  # (the box at (20, 0) stays)
    assert gt.valid.shape == (8, 65) and pred.valid.shape == (8, 130)
    draws = torch.from_numpy(g.integers(0, 3, (8, 130)).astype(np.int32))
    table = _table()
    dev = match_detections(gt.clone().to("cuda"), pred.clone().to("cuda"), table, draws.cuda())
    torch.cuda.synchronize()
    pk = lambda s: {k: v.numpy() for k, v in pack_boxes(s).items()}  # noqa: E731
    return dict(gt=gt, pred=pred, draws=draws, table=table, dev=_np(dev), pgt=pk(gt), ppred=pk(pred))


@pytest.mark.parametrize("tag", ["bev", "i3d"])
def test_device_path_reproduces_reference_fixture(golden_dir, tag):
    g = np.load(f"{golden_dir}/od_metrics_reference.npz")
    gt, pred = fixture_batch(g, tag)
    v = fixture_validator(tag)
    v.update_batch(gt.to("cuda"), None, pred.to("cuda"))
    assert_fixture(v, g, tag)


def test_device_equals_host_restatement_bitwise_at_the_edges(edge):
    from liso_amd.eval.det_validation import match_detections_host

    d = edge["dev"]
    host = match_detections_host(edge["pgt"], edge["ppred"], edge["table"], edge["draws"].numpy(), pairs={k: d[k] for k in MATS})
    _same(d, host, OUT)
    t = edge["table"]
    job = lambda f, c, thr: t.jobs.index((f, c, float(np.float32(thr))))  # noqa: E731
    cnt = d["count"]
    assert cnt[0].sum() == cnt[1].sum() == cnt[2].sum() == 0 and cnt[3, job(0, "iou_bev", 0.25)] > 20  # G = 0, P = 0, both; 65 x 130
    far_sets = [j for j, b in enumerate(t.jobs) if b.filter != 0 and b.filter != 4]
    assert cnt[4, far_sets].sum() == 0 and cnt[4, job(0, "dist", 2.0)] > 0 and not d["gt_in"][4, 1:4].any()  # everything filtered out
    assert cnt[:, [j for j, b in enumerate(t.jobs) if b.filter == 6]].sum() == 0
    # the box at (20, 0): in 20-40 m, not in 0-20 m; (50, -20) lies on the inclusive area bound, the next float after 50 outside
    assert d["gt_in"][7, 1, 0] == 0 and d["gt_in"][7, 2, 0] == 1 and d["pred_in"][7, 2, 0] == 1
    assert d["gt_in"][7, 3, :4].tolist() == [1, int(edge["gt"].valid[7, 1]), 0, 0]
    assert d["pairs"][7, job(2, "iou_bev", 0.5), 0].tolist() == [0, 0]
    # equal IoUs in one prediction's row: the lowest ground-truth slot wins
    assert edge["gt"].valid[5, 0] and edge["gt"].valid[5, 1] and edge["pred"].valid[5, 0]  # (the holes spare the three boxes)
    row = d["iou_bev"][5, 0]
    assert row[0] == row[1] > 0.99
    pr = d["pairs"][5, job(0, "iou_bev", 0.5), : cnt[5, job(0, "iou_bev", 0.5)]]
    assert pr[pr[:, 1] == 0, 0].tolist() == [0]
    # the NaN boxes are never matched where their NaN enters the value
    j = job(0, "dist", 2.0)
    assert 3 not in d["pairs"][6, j, : cnt[6, j], 0].tolist()
    assert np.isfinite(d["sums"][:, [job(0, "dist", 2.0), job(0, "dist", 0.5)], 0]).all()


def test_default_host_order_equals_the_device_order(edge):
    from liso_amd.eval.det_validation import stable_order_host

    assert np.array_equal(stable_order_host(edge["ppred"]["score"], edge["ppred"]["valid"]), edge["dev"]["order"])


def test_pair_matrices(edge):
    from liso_amd.utils.nms_iou import box_iou_matrix, boxes_iou_bev

    d, gt, pred = edge["dev"], edge["gt"], edge["pred"]
    rows_g, rows_p = torch.from_numpy(edge["pgt"]["rows"]).cuda(), torch.from_numpy(edge["ppred"]["rows"]).cuda()
    checked = 0
    for f in (3, 4, 5, 7):  # (frame 6 holds the NaN boxes)
        gv, pv = gt.valid[f].numpy(), pred.valid[f].numpy()
        want = boxes_iou_bev(rows_g[f].contiguous(), rows_p[f].contiguous()).cpu().numpy().T  # liso_iou3d_iou_bev_f32, [P,G]
        got = d["iou_bev"][f]
        assert np.array_equal(got[np.ix_(pv, gv)].view(np.uint32), np.ascontiguousarray(want[np.ix_(pv, gv)]).view(np.uint32)), f
        assert not got[~pv].any() and not got[:, ~gv].any()
        g1, p1 = gt[f].drop_padding_boxes().to("cuda"), pred[f].drop_padding_boxes().to("cuda")
        i3d = box_iou_matrix(g1, p1, "iou_3d").cpu().numpy().T
        assert np.allclose(d["iou_3d"][f][np.ix_(pv, gv)], i3d, rtol=1e-6, atol=0), f
        dist = torch.cdist(p1.pos[:, :2].float(), g1.pos[:, :2].float(), compute_mode="donot_use_mm_for_euclid_dist").cpu().numpy()
        assert np.allclose(d["dist"][f][np.ix_(pv, gv)], dist, rtol=1e-6, atol=0), f
        checked += int((i3d > 0).sum())
    assert checked > 100


def test_batch_equals_single_frames_and_two_runs_are_equal(edge):
    from liso_amd.eval.det_validation import match_detections

    gt, pred, draws = edge["gt"].clone().to("cuda"), edge["pred"].clone().to("cuda"), edge["draws"].cuda()
    again = _np(match_detections(gt, pred, edge["table"], draws))
    _same(edge["dev"], again, OUT + MATS, "second run")
    for f in range(gt.valid.shape[0]):
        one = _np(match_detections(gt[f:f + 1], pred[f:f + 1], edge["table"], draws[f:f + 1]))
        _same({k: edge["dev"][k][f:f + 1] for k in OUT + MATS}, one, OUT + MATS, f"frame {f}")


def test_garbage_in_invalid_slots_changes_nothing(edge):
    from liso_amd.eval.det_validation import match_detections

    g = np.random.default_rng(13)
    gt, pred = edge["gt"].clone(), edge["pred"].clone()
    for s in (gt, pred):
        bad = ~s.valid
        for k in ("pos", "dims", "rot", "probs"):
            v = getattr(s, k)
            junk = torch.from_numpy(g.normal(0, 30, tuple(v.shape)).astype(np.float32))
            junk[::2] = float("nan")
            setattr(s, k, torch.where(bad[..., None], junk, v))
        s.class_id = torch.where(bad[..., None], torch.from_numpy(g.integers(0, 3, tuple(s.class_id.shape))), s.class_id)
    draws = torch.where(pred.valid, edge["draws"], torch.from_numpy(g.integers(-5, 50, tuple(edge["draws"].shape)).astype(np.int32)))
    got = _np(match_detections(gt.to("cuda"), pred.to("cuda"), edge["table"], draws.cuda()))
    _same(edge["dev"], got, OUT + MATS)


def test_captured_replay_equals_the_eager_call(edge):
    """(a capture also shows there is no host sync and no allocation outside the graph's pool)"""
    from liso_amd.eval.det_validation import match_detections
    from liso_amd.utils.graph_capture import capture

    gt, pred, draws = edge["gt"].clone().to("cuda"), edge["pred"].clone().to("cuda"), edge["draws"].cuda()
    stream = torch.cuda.Stream()
    graph, out = capture(lambda: match_detections(gt, pred, edge["table"], draws), stream, warm_ups=2)
    for k in OUT + MATS:
        out[k].fill_(7)  # (the replay, not the capture, fills the tables)
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        graph.replay()
    stream.synchronize()
    _same(edge["dev"], _np(out), OUT + MATS)


def test_nothing_is_written_outside_the_outputs(edge):
    from liso_amd.eval.det_validation import match_detections
    from tests.guarded_alloc import guarded

    gt, pred, draws = edge["gt"].clone().to("cuda"), edge["pred"].clone().to("cuda"), edge["draws"].cuda()
    with guarded() as g:
        out = match_detections(gt, pred, edge["table"], draws)  # every output at its exact size between guard bands
        assert g.check() > 8
    _same(edge["dev"], _np(out), OUT + MATS)
    for F, G, P in ((1, 1, 1), (2, 0, 3), (2, 3, 0), (1, 64, 65), (1, 129, 64)):
        fr = [scene(np.random.default_rng(F + G + P), G, P, 3, spread=8.0) for _ in range(F)]
        with guarded() as g:
            match_detections(pad_batch([f[0] for f in fr]).to("cuda"), pad_batch([f[1] for f in fr]).to("cuda"), edge["table"],
                             torch.zeros((F, P), dtype=torch.int32, device="cuda"))
            g.check()


# ---- the full run_val collection set ----------------------------------------------------------------------------------------
SEED, CLASS_NAMES, CLASS_IDXS = 0, ("car", "ped", "cyc"), (0, 1, 2)
SIZES = ((30, 45), (40, 60), (12, 9), (0, 14), (25, 0), (33, 52))


def val_set(seed):
    """6 frames: visible ground truth, the benchmark's (a subset of it plus a few boxes of its own), predictions, class draws"""
    g = np.random.default_rng(seed)
    gts, bms, preds = [], [], []
    for n_gt, n_pred in SIZES:
        gt, pred = scene(g, n_gt, n_pred, 3, spread=55.0)
        extra, _ = scene(g, 4, 0, 3, spread=55.0)
        keep = g.uniform(size=n_gt) < 0.7
        bms.append(_cat([{k: v[keep] for k, v in gt.items()}, extra]))
        gts.append(gt), preds.append(pred)
    return gts, bms, preds, g.integers(0, 3, (len(SIZES), max(p for _, p in SIZES))).astype(np.int32)


def _quad(b):
    c, s = np.cos(b[6]), np.sin(b[6])
    return np.array([[b[0] + sx * b[3] / 2 * c - sy * b[4] / 2 * s, b[1] + sx * b[3] / 2 * s + sy * b[4] / 2 * c] for sx, sy in ((-1, -1), (1, -1), (1, 1), (-1, 1))])


def _overlap64(a, b):
    """area of the intersection of two rotated rectangles in fp64 (Sutherland-Hodgman)"""
    poly, clip = _quad(a), _quad(b)
    for i in range(4):
        p0, p1 = clip[i], clip[(i + 1) % 4]
        side = lambda q: (p1[0] - p0[0]) * (q[1] - p0[1]) - (p1[1] - p0[1]) * (q[0] - p0[0])  # noqa: E731
        out = []
        for k in range(len(poly)):
            q0, q1 = poly[k], poly[(k + 1) % len(poly)]
            s0, s1 = side(q0), side(q1)
            if s0 >= 0:
                out.append(q0)
            if (s0 > 0 > s1) or (s0 < 0 < s1):
                out.append(q0 + (q1 - q0) * (s0 / (s0 - s1)))
        poly = out
        if len(poly) < 3:
            return 0.0
    x, y = np.array(poly).T
    return 0.5 * abs(np.dot(x, np.roll(y, -1)) - np.dot(y, np.roll(x, -1)))


def assert_no_decision_on_an_edge(gts, bms, preds):
    """in fp64: no IoU or distance within 1e-4 of a threshold, no radius or coordinate within 1e-3 m of an edge, distinct scores"""
    thr = np.array([0.25, 0.3, 0.4, 0.5, 0.7])
    rows = lambda d: np.concatenate([d["pos"], d["dims"], d["rot"]], -1).astype(np.float64)  # noqa: E731
    for f in range(len(preds)):
        p = rows(preds[f])
        assert len(np.unique(preds[f]["probs"])) == len(p), f
        for boxes in (rows(gts[f]), rows(bms[f]), p):
            r = np.hypot(boxes[:, 0], boxes[:, 1])
            assert (np.abs(r[:, None] - np.array([20.0, 40.0, 60.0, 1000.0])) > 1e-3).all() and (r > 1e-3).all(), f
            assert (np.abs(np.abs(boxes[:, 0]) - 50.0) > 1e-3).all() and (np.abs(np.abs(boxes[:, 1]) - 20.0) > 1e-3).all(), f
        for g in (rows(gts[f]), rows(bms[f])):
            for a in g:
                d = np.hypot(p[:, 0] - a[0], p[:, 1] - a[1])
                assert (np.abs(d - 3.0) > 1e-4).all(), f
                for b in p[d < 12.0]:
                    ov = _overlap64(a, b)
                    if ov == 0.0:
                        continue
                    bev = ov / (a[3] * a[4] + b[3] * b[4] - ov)
                    h = min(a[2] + a[5] / 2, b[2] + b[5] / 2) - max(a[2] - a[5] / 2, b[2] - b[5] / 2)
                    inter = ov * h if h > 0 else 0.0
                    i3d = inter / (a[3] * a[4] * a[5] + b[3] * b[4] * b[5] - inter)
                    assert (np.abs(bev - thr) > 1e-4).all() and (np.abs(i3d - thr) > 1e-4).all(), (f, bev, i3d)


def test_seeded_set_has_no_decision_on_an_edge():
    gts, bms, preds, _ = val_set(SEED)
    assert_no_decision_on_an_edge(gts, bms, preds)


def _transfer_host(gt, pred, draws):
    """run_val :406-447 with the given draws, on unbatched device Shapes"""
    from liso_amd.kabsch.box_groundtruth_matching import slow_greedy_match_boxes_by_desending_confidence_by_dist

    idx_gt, idx_pred, _, _, _ = slow_greedy_match_boxes_by_desending_confidence_by_dist(
        gt.pos, pred.pos, non_batched_pred_confidence=torch.squeeze(pred.probs, dim=-1), matching_threshold=3.0, match_in_nd=2)
    pred.class_id = draws.to(pred.class_id.device).to(pred.class_id.dtype)[:, None].clone()
    pred.class_id[torch.from_numpy(idx_pred).to(pred.class_id.device)] = gt.class_id[torch.from_numpy(idx_gt).to(pred.class_id.device)].to(pred.class_id.dtype)
    return pred


def test_run_val_collections_equal_the_per_frame_path():
    from liso_amd.eval.det_validation import DetectionValidator
    from tests.det_val_cases import shape_of

    gts, bms, preds, draws = val_set(SEED)
    assert_no_decision_on_an_edge(gts, bms, preds)  # the equality below holds only where no decision sits on an edge
    v = DetectionValidator.for_run_val("kitti", CLASS_NAMES, CLASS_IDXS, moving_velocity_thresh=0.5)
    ref = DetectionValidator.for_run_val("kitti", CLASS_NAMES, CLASS_IDXS, moving_velocity_thresh=0.5)  # (its collections only)
    v.update_batch(pad_batch(gts).to("cuda"), pad_batch(bms).to("cuda"), pad_batch(preds).to("cuda"), class_draws=torch.from_numpy(draws).cuda())
    got = v.compute("val/")
    want = {}
    for f in range(len(preds)):
        gt, bm, pred = shape_of(gts[f]).to("cuda"), shape_of(bms[f]).to("cuda"), shape_of(preds[f]).to("cuda")
        pred = _transfer_host(gt, pred, torch.from_numpy(draws[f, : len(preds[f]["valid"])]))
        for c, m in zip(ref.collections, ref.metrics):
            m.update(non_batched_gt_boxes=bm if c.gt_set == "benchmark" else gt, non_batched_pred_boxes=pred)
    n_lists = 0
    for c, m, mine in zip(ref.collections, ref.metrics, v.metrics):
        want.update(m.compute("val/" + c.tag))
        for cn in m.class_names:
            for thr in m.matching_thresholds:
                for cat in m.CATEGORIES:
                    for a, b in zip(m.collected(cn, thr, cat), mine.collected(cn, thr, cat)):
                        assert np.array_equal(a, b), (c.tag, m.box_matching_criterion, cn, thr, cat)
                    n_lists += 1
                assert m.tp_errors[cn][thr]["tps"] == mine.tp_errors[cn][thr]["tps"]
    assert n_lists == (24 * 4 + 3 * 4) * 3 and set(got) == set(want)
    assert "val/final_result/visible/detection_metrics/0_20m/iou_bev/overall/AP@0.5iou_bev" in got
    assert "val/final_result/KITTI/per_class/detection_metrics/iou_bev/ped/AP@0.3iou_bev" in got
    n_ap = 0
    for k, w in want.items():
        g_ = got[k]
        if "AP@" in k:
            assert (np.isnan(g_) and np.isnan(w)) or abs(g_ - w) <= 1e-9, (k, g_, w)
            n_ap += 1
        elif k.endswith(("num_objs", "tps")):
            assert g_ == w, k
        else:
            assert abs(g_ - w) <= 1e-4 * max(abs(w), 1.0), (k, g_, w)  # ATE / ASE / AOE: summed in fp32 there, in fp64 here
    assert n_ap > 300 and got["val/final_result/visible/detection_metrics/0_1000m/iou_bev/overall/AP@0.5iou_bev"] > 0.1


# ---- run_val on a small detector ------------------------------------------------------------------------------------------------
class _DistinctScores:
    """the detector's `predict_boxes` with a slot-dependent offset on the probs: an untrained network gives many boxes the same
    logit, and the per-frame path leaves the visiting order of equal scores to torch.argsort"""

    def __init__(self, net):
        self.net = net

    def predict_boxes(self, *args, **kwargs):
        boxes, keep, counts = self.net.predict_boxes(*args, **kwargs)
        P = boxes.valid.shape[1]
        boxes.probs = torch.where(boxes.valid[..., None], boxes.probs + 1e-3 * torch.arange(P, device=boxes.probs.device)[None, :, None], boxes.probs)
        return boxes, keep, counts


def test_run_val_on_a_small_detector_and_eval_model():
    from liso_amd.datasets.synthetic import detector_batch
    from liso_amd.eval.det_validation import DetectionValidator
    from liso_amd.eval.eval_ours import kitti_annotated_fov_mask, run_val
    from liso_amd.trainer import DetectorTrainer
    from liso_amd.utils.config import default_cfg

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    tr = DetectorTrainer(default_cfg(grid=64, bev_range_m=40.0), dev, total_steps=4)
    pcls, _ = detector_batch(3, 2, dev, n_points=4000, grid=64, bev_range_m=40.0)
    g = np.random.default_rng(21)
    gts = [scene(g, n, 0, 3, spread=18.0)[0] for n in (14, 9)]
    bms = [{k: v[: len(v) // 2] for k, v in gt.items()} for gt in gts]
    batch = dict(pcls=pcls, gt_boxes=pad_batch(gts).to("cuda"), benchmark_gt_boxes=pad_batch(bms).to("cuda"),
                 pcl_full_w_ground=torch.stack([p[:, :3] for p in pcls]))
    names, seed = ("car", "ped", "cyc"), 5
    tr.net.eval()
    predictor = _DistinctScores(tr.net)
    plain = {k: v for k, v in batch.items() if k != "pcl_full_w_ground"}  # (no KITTI rule: every post-NMS box is evaluated)
    got = run_val(tr.cfg, [batch, plain], predictor, "val/", movable_class_names=names, generator=torch.Generator(device=dev).manual_seed(seed))

    # the same predict_boxes output through the per-frame path
    gen = torch.Generator(device=dev).manual_seed(seed)
    ref = DetectionValidator.for_run_val("kitti", names, (0, 1, 2), moving_velocity_thresh=0.1)
    for b in (batch, plain):
        pred, _, _ = predictor.predict_boxes(None, pcls, logit_threshold=-1.0e32)
        if "pcl_full_w_ground" in b:
            n_all = int(pred.valid.sum())
            pred.valid = pred.valid & kitti_annotated_fov_mask(pred, b["pcl_full_w_ground"])
            assert 0 < int(pred.valid.sum()) < n_all
        else:
            assert int(pred.valid.sum()) > 50
        draws = torch.randint(0, 3, tuple(pred.valid.shape), device=dev, generator=gen, dtype=torch.int32)
        for f in range(2):
            p1 = _transfer_host(b["gt_boxes"][f].drop_padding_boxes(), pred[f].drop_padding_boxes(), draws[f][pred.valid[f]])
            for c, m in zip(ref.collections, ref.metrics):
                m.update(non_batched_gt_boxes=(b["benchmark_gt_boxes"] if c.gt_set == "benchmark" else b["gt_boxes"])[f].drop_padding_boxes(),
                         non_batched_pred_boxes=p1)
    want = {}
    for c, m in zip(ref.collections, ref.metrics):
        want.update(m.compute("val/" + c.tag))
    assert set(got) == set(want) and len(got) > 1000
    for k, w in want.items():
        if "AP@" in k:
            assert (np.isnan(got[k]) and np.isnan(w)) or abs(got[k] - w) <= 1e-9, (k, got[k], w)
        elif k.endswith(("num_objs", "tps")):
            assert got[k] == w, k
        else:
            assert abs(got[k] - w) <= 1e-4 * max(abs(w), 1.0), (k, got[k], w)

    # eval_model: eval mode inside, the previous mode and every parameter and buffer afterwards
    tr.net.train()
    before = {k: v.detach().clone() for k, v in tr.net.state_dict().items()}
    seen = []

    def batches():
        seen.append(tr.net.training)
        yield batch
    res = tr.eval_model(batches(), movable_class_names=names)
    assert seen == [False] and tr.net.training and set(res) == {k[len("val/"):] for k in want}
    after = tr.net.state_dict()
    assert set(after) == set(before) and all(torch.equal(before[k], after[k]) for k in before)
