"""Detector inference NMS on the device (include/liso_det_nms.h): dense [B,N] maps -> the first P survivors of the reference's
greedy rotated NMS, per sample, with no host sync.

Yardsticks: the reference's CPU greedy pass (oracle.iou3d.nms) and, bit for bit, the existing full-mask device NMS
(nms_gpu_device) composed with torch.sort(stable=True) and indexing -- the same predicate over the same order."""
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _D():
    from liso_amd import det_nms

    return det_nms


def _yardstick(dense, scores, participate, thresh, pre, post):
    """per sample: stable descending sort of the participating slots, pre cut, full-mask nms_gpu_device, first `post` -> slots"""
    from liso_amd import iou3d_nms_cuda as M

    out = []
    for b in range(dense.shape[0]):
        slots = torch.nonzero(participate[b]).reshape(-1)
        order = slots[torch.sort(scores[b, slots], stable=True, descending=True)[1]]
        if pre is not None:
            order = order[:pre]
        if order.numel() == 0:
            out.append(order.cpu())
            continue
        kd, nd = M.nms_gpu_device(dense[b, order].contiguous(), thresh)
        out.append(order[kd[: int(nd.item())]][:post].cpu())
    return out


def _run(dense, scores, thresh, pre, post, valid=None, gate=None, logit_threshold=None):
    D = _D()
    keys, idx = D.order(scores, gate, valid, logit_threshold)
    keep, counts = D.select(dense, keys, idx, thresh, pre, post)
    return keep, counts


def _check_against(keep, counts, expected, post):
    keep, counts = keep.cpu(), counts.cpu()
    for b, e in enumerate(expected):
        n = int(counts[b])
        assert n == len(e), (b, n, len(e))
        assert torch.equal(keep[b, :n], e.to(torch.int64)), b
        assert bool((keep[b, n:] == -1).all()), b
        assert n <= post


# ---------------------------------------------------------------------------------------------------------- 1. vs the oracle
@pytest.mark.parametrize("n", [64, 1000, 4096])
@pytest.mark.parametrize("thresh", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("post", [1, 83, 500])
def test_keep_lists_equal_reference_greedy(n, thresh, post):
    from oracle import iou3d as O

    b, s = O.random_boxes(n, 7 + n, 50.0)
    order = np.argsort(-s, kind="stable")
    ref = order[O.nms(b[order], thresh)][:post]
    dense = torch.from_numpy(b)[None].to(DEV)
    keep, counts = _run(dense, torch.from_numpy(s)[None].to(DEV), thresh, None, post)
    got = keep[0, : int(counts[0])].cpu().numpy()
    if not np.array_equal(got, ref):
        # device sin/cos/atan2 may differ from glibc by 1 ulp (tests/test_gpu_iou3d.py): only a pair within that of `thresh`
        # may decide differently, and then the device's own full-mask pass is the yardstick
        iou = O.boxes_iou_bev(b, b)
        assert np.any(np.abs(iou - thresh) <= 1e-5), (n, thresh, post)
        exp = _yardstick(dense, torch.from_numpy(s)[None].to(DEV), torch.ones(1, n, dtype=torch.bool, device=DEV), thresh, None, post)
        _check_against(keep, counts, exp, post)
    assert bool((keep[0, len(got):] == -1).all())


# --------------------------------------------------------------------------------- 2. bitwise vs the full-mask device pass
_NETS = {}


def _untrained_detector_map(grid, batch=1, seed=3):
    key = (grid, batch, seed)
    if key not in _NETS:
        _NETS[key] = _make_untrained_detector_map(grid, batch, seed)
    return _NETS[key]


def _make_untrained_detector_map(grid, batch, seed):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    from keyed_init import keyed_state_dict

    from liso_amd.datasets.synthetic import detector_batch
    from liso_amd.networks.simple_net.simple_net import BoxLearner
    from liso_amd.utils.config import default_cfg

    cfg = default_cfg(grid=grid, bev_range_m=100.0 * grid / 512)
    net = BoxLearner(cfg).to(DEV)
    sd = net.state_dict()
    init = keyed_state_dict({k: (tuple(v.shape), v.dtype) for k, v in sd.items()})
    net.load_state_dict({**sd, **{k: v.to(DEV) for k, v in init.items()}}, strict=True)
    net.eval()
    pcls, _ = detector_batch(seed, batch, DEV, n_points=30000, grid=grid, bev_range_m=100.0 * grid / 512)
    return net, pcls, cfg


def _dense(shape):
    from liso_amd.utils.nms_iou import convert_shapes_to_dense_3d

    return convert_shapes_to_dense_3d(shape).float().contiguous()


def _families(side):
    from liso_amd.datasets.synthetic import detector_map_trained_like

    net, pcls, _ = _untrained_detector_map(side * 4)
    with torch.no_grad():
        untrained = net(None, pcls, train=False)[0]
    return {"untrained": untrained, "trained_like": detector_map_trained_like(11, 1, side, DEV)}


@pytest.mark.parametrize("family", ["untrained", "trained_like"])
@pytest.mark.parametrize("pre,post", [(None, 500), (1000, 100)])
def test_bitwise_equal_full_mask_16k(family, pre, post):
    boxes = _families(128)[family]
    assert boxes.valid.shape == (1, 16384)
    dense = _dense(boxes)
    scores = torch.sigmoid(boxes.probs[..., 0].float()).contiguous()
    keep, counts = _run(dense, scores, 0.1, pre, post)
    _check_against(keep, counts, _yardstick(dense, scores, boxes.valid, 0.1, pre, post), post)


def test_bitwise_equal_full_mask_64k_once():
    from liso_amd.datasets.synthetic import detector_map_trained_like

    boxes = detector_map_trained_like(12, 1, 256, DEV)
    dense = _dense(boxes)
    scores = torch.sigmoid(boxes.probs[..., 0]).contiguous()
    keep, counts = _run(dense, scores, 0.1, None, 500)
    _check_against(keep, counts, _yardstick(dense, scores, boxes.valid, 0.1, None, 500), 500)


# ------------------------------------------------------------------------------------------------------- 3. batches
def _batch_case(seed=5, n=3000):
    from oracle import iou3d as O

    B = 4
    boxes, scores, valid = [], [], []
    for b in range(B):
        bx, s = O.random_boxes(n, seed * 10 + b, 30.0)
        boxes.append(torch.from_numpy(bx))
        scores.append(torch.from_numpy(s))
    dense = torch.stack(boxes).to(DEV)
    logits = (torch.stack(scores) * 20 - 10).to(DEV)
    g = torch.Generator().manual_seed(seed)
    valid = torch.rand(B, n, generator=g).to(DEV) < torch.tensor([[0.9], [0.5], [0.0], [1.0]], device=DEV)  # sample 2: no valid slot
    logits[0, :200] = 3.0                     # ties
    logits[1, :300] = 80.0                    # sigmoid saturates to 1.0f: ties by slot index
    logits[3, 100:400] = torch.round(logits[3, 100:400])  # many small tie groups
    return dense, logits, valid


@pytest.mark.parametrize("pre,post,thr", [(None, 500, None), (1000, 100, None), (250, 1024, -2.0), (None, 37, 1.5)])
def test_batch_of_four_matches_composition(pre, post, thr):
    dense, logits, valid = _batch_case()
    scores = torch.sigmoid(logits)
    keep, counts = _run(dense, scores, 0.1, pre, post, valid=valid, gate=logits, logit_threshold=thr)
    part = valid & ~(logits < (thr if thr is not None else -math.inf))
    _check_against(keep, counts, _yardstick(dense, scores, part, 0.1, pre, post), post)
    assert int(counts[2]) == 0 and bool((keep[2] == -1).all())


def test_order_places_nan_like_stable_torch_sort():
    D = _D()
    v = torch.tensor([0.5, float("nan"), -0.0, 0.0, float("inf"), -float("inf"), 0.5, float("nan"), -1.0, 0.5, 3.0],
                     device=DEV)
    scores = torch.cat([v, v.flip(0), torch.rand(5000, device=DEV).round(decimals=2)])[None].contiguous()
    keys, idx = D.order(scores)
    ref = torch.sort(scores[0], stable=True, descending=True)[1]
    assert torch.equal(idx[0].long(), ref)


def test_gathered_shape_and_padding():
    from liso_amd.kabsch.shape_utils import INVALID_CLASS_ID, Shape
    from liso_amd.utils.nms_iou import iou_based_nms_batched

    dense, logits, valid = _batch_case(seed=8, n=700)
    B, N = valid.shape
    g = torch.Generator().manual_seed(1)
    boxes = Shape(pos=dense[..., 0:3].contiguous(), dims=dense[..., 3:6].contiguous(), rot=dense[..., 6:7].contiguous(),
                  probs=logits[..., None].contiguous(), velo=torch.randn(B, N, 2, generator=g).double().to(DEV), valid=valid,
                  class_id=torch.randint(0, 5, (B, N, 1), generator=g, dtype=torch.int32).to(DEV),
                  difficulty=torch.randint(0, 3, (B, N, 1), generator=g, dtype=torch.int32).to(DEV))
    out, keep, counts = iou_based_nms_batched(boxes, 0.1, post_nms_max_boxes=64)
    for b in range(B):
        n = int(counts[b])
        k = keep[b, :n]
        for name in ("pos", "dims", "rot", "probs", "velo", "class_id", "difficulty", "valid"):
            got, src = getattr(out, name)[b], getattr(boxes, name)[b]
            assert got.dtype == src.dtype
            assert torch.equal(got[:n], src[k]), (b, name)
            pad = False if name == "valid" else (INVALID_CLASS_ID if name in ("class_id", "difficulty") else 0.0)
            assert bool((got[n:] == pad).all()), (b, name)
    # and per sample it is iou_based_nms on the compacted sample, mapped back to slots
    from liso_amd.utils.nms_iou import iou_based_nms

    for b in (0, 3):
        s = boxes[b].drop_padding_boxes()
        slots = torch.nonzero(boxes.valid[b]).reshape(-1)
        ref = slots[iou_based_nms(s, 0.1, post_nms_max_boxes=64)]
        got = keep[b, : int(counts[b])]
        if not torch.equal(got, ref):  # only where the unstable reference sort reordered tied scores
            assert len(torch.unique(s.probs)) < s.probs.numel()


# ------------------------------------------------------------------------------------------------------- 4. edge geometry
def test_edge_geometry_matches_full_mask():
    from oracle import iou3d as O

    n = 700
    bx, s = O.random_boxes(n, 21, 20.0)
    b = torch.from_numpy(bx)
    b[0:5, 3:5] = torch.tensor([1e4, 2e4])          # huge boxes: the circle reject must not skip a suppressed pair
    b[5:8, 3:5] = torch.tensor([3e18, 1e18])         # radius overflows to inf
    b[8:10, 0] = 1e7                                 # far away
    b[10:20, 3:5] = 0.0                              # zero-size
    b[20, 0] = float("nan")
    b[21, 3] = float("inf")
    b[22, 6] = float("nan")
    b[23, 1] = -float("inf")
    dense = b[None].to(DEV)
    scores = torch.from_numpy(s)[None].to(DEV)
    scores[0, :30] = scores[0, :30] + 1.0  # the odd boxes rank first, so they act on everything else
    allv = torch.ones(1, n, dtype=torch.bool, device=DEV)
    for thresh in (0.1, 0.0, -0.5):
        for post in (1, 200, 1024):
            keep, counts = _run(dense, scores, thresh, None, post)
            _check_against(keep, counts, _yardstick(dense, scores, allv, thresh, None, post), post)


# ------------------------------------------------------------------------------------------------------- 5. predict_boxes
def _reference_style(net, pcls, cfg, pre, post, sigmoid_probs, logit_threshold=-1e32):
    """run_val / tracker post-processing from existing pieces, with a stable sort in rotate_nms_pcdet's place"""
    from liso_amd import iou3d_nms_cuda as M
    from liso_amd.utils.nms_iou import convert_shapes_to_dense_3d

    with torch.no_grad():
        pred = net(None, pcls, train=False)[0]
    out = []
    for b in range(pred.valid.shape[0]):
        s = pred[b].drop_padding_boxes()
        s = s[~torch.squeeze(s.probs < logit_threshold, dim=-1)]
        ranked = s.clone()
        ranked.probs = torch.sigmoid(ranked.probs)
        if sigmoid_probs:
            s = ranked
        order = torch.sort(torch.squeeze(ranked.probs, -1), stable=True, descending=True)[1]
        if pre is not None:
            order = order[:pre]
        kd, nd = M.nms_gpu_device(convert_shapes_to_dense_3d(ranked.clone())[order].float().contiguous(), cfg.nms_iou_threshold)
        idx = order[kd[: int(nd.item())]][:post]
        out.append(s[idx])
    return pred, out


@pytest.mark.parametrize("mode", ["run_val", "tracker"])
def test_predict_boxes_equals_reference_style_path(mode):
    net, pcls, cfg = _untrained_detector_map(256, batch=2, seed=4)
    kw = {} if mode == "run_val" else {"pre_nms_max_boxes": 1000, "post_nms_max_boxes": 100, "sigmoid_probs": True}
    pre, post = kw.get("pre_nms_max_boxes"), kw.get("post_nms_max_boxes", 500)
    pred, ref = _reference_style(net, pcls, cfg, pre, post, kw.get("sigmoid_probs", False))
    with torch.no_grad():
        again = net(None, pcls, train=False)[0]
    assert torch.equal(again.probs, pred.probs) and torch.equal(again.pos, pred.pos)  # the forward itself is deterministic
    out, keep, counts = net.predict_boxes(None, pcls, **kw)
    assert keep.shape == (2, post)
    for b, r in enumerate(ref):
        n = int(counts[b])
        assert n == r.valid.shape[0] and n > 0
        for name in ("pos", "dims", "rot", "probs", "velo", "class_id", "difficulty", "valid"):
            got, want = getattr(out, name)[b, :n], getattr(r, name)
            assert got.dtype == want.dtype and torch.equal(got, want), (mode, b, name)
        assert not bool(out.valid[b, n:].any())


# ------------------------------------------------------------------------------------------------------- 6. hipGraph
def test_graph_replay_equals_eager():
    from liso_amd.utils.nms_iou import iou_based_nms_batched

    dense, logits, valid = _batch_case(seed=9, n=5000)
    from liso_amd.kabsch.shape_utils import Shape

    boxes = Shape(pos=dense[..., 0:3].contiguous(), dims=dense[..., 3:6].contiguous(), rot=dense[..., 6:7].contiguous(),
                  probs=logits[..., None].contiguous(), valid=valid)
    scores = torch.sigmoid(logits)

    def run():
        return iou_based_nms_batched(boxes, 0.1, 1000, 100, scores=scores, logit_threshold=-1.0, threshold_values=logits)

    e1, e2 = run(), run()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_out = run()
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    for a, b, c in ((e1[1], e2[1], g_out[1]), (e1[2], e2[2], g_out[2])):
        assert torch.equal(a, b) and torch.equal(a, c)
    for name in ("pos", "dims", "rot", "probs", "velo", "class_id", "difficulty", "valid"):
        a, b, c = getattr(e1[0], name), getattr(e2[0], name), getattr(g_out[0], name)
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)) and torch.equal(a.view(torch.uint8), c.view(torch.uint8)), name


# ------------------------------------------------------------------------------------------------------- 7. guard bands
@pytest.mark.parametrize("n,post", [(1, 1), (1, 500), (1000, 300), (4097, 1024), (300, 300), (65, 64)])
def test_guarded_edge_sizes(n, post):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import iou3d as O
    from tests.guarded_alloc import guarded

    bx, s = O.random_boxes(n, n + post, 10.0)
    dense = torch.from_numpy(bx)[None].to(DEV).repeat(2, 1, 1).contiguous()
    scores = torch.from_numpy(s)[None].to(DEV).repeat(2, 1).contiguous()
    valid = torch.ones(2, n, dtype=torch.bool, device=DEV)
    valid[1, ::3] = False
    with guarded() as g:
        keep, counts = _run(dense, scores, 0.2, None, post, valid=valid)
        keys, _ = _D().order(scores, None, valid)
        g.check()
    _check_against(keep, counts, _yardstick(dense, scores, valid, 0.2, None, post), post)
    assert int((keys[1] == -1).sum()) == int((~valid[1]).sum())


def test_empty_samples():
    D = _D()
    keys, idx = D.order(torch.zeros(3, 0, device=DEV))
    keep, counts = D.select(torch.zeros(3, 0, 7, device=DEV), keys, idx, 0.1, None, 10)
    assert keep.shape == (3, 10) and bool((keep == -1).all()) and bool((counts == 0).all())
    (pos,) = D.gather(keep, counts, [torch.zeros(3, 0, 3, device=DEV)], [0.0])
    assert pos.shape == (3, 10, 3) and bool((pos == 0).all())
