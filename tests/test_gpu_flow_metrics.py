"""The scene-flow metrics accumulator (include/liso_flow_metrics.h) against the reference's own numbers
(tests/golden/flow_metrics_reference.npz, tests/golden/make_flow_metrics_golden.py): per-point EPE bit for bit, every count and
ratio exactly, the means to 1e-6; update splitting, run-to-run and hipGraph determinism, and edge sizes inside guard bands."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FLOWS = ("raw", "agg", "rig")
RATIOS = ("ACC3D_0_05", "ACC3D_0_1", "Outliers3D", "RobustOutliers3D")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "flow_metrics_reference.npz"))


def _batches(z, case):
    dev = torch.device("cuda")
    out = []
    for i in range(int(z[f"{case}__n"])):
        g = lambda k: torch.from_numpy(np.ascontiguousarray(z[f"{case}__{i}__{k}"])).to(dev)  # noqa: E731
        out.append(dict(points=g("points"), gt=g("gt"), preds=g("preds"), valid=g("valid"), moving=g("moving"), label=g("label"),
                        epe=z[f"{case}__{i}__epe"]))
    return out


def _close(a, b, rel, scale=0.0):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert np.array_equal(np.isnan(a), np.isnan(b)), (a, b)
    ok = ~np.isnan(a)
    assert np.all(np.abs(a[ok] - b[ok]) <= rel * np.maximum(np.abs(b[ok]), scale)), (a, b)


def _check_metrics(mine, ref_get, keys_ref):
    for key in keys_ref:
        m = mine[key]
        n = int(ref_get(key, "num_pts_used"))
        assert m["num_pts_used"] == n, key
        assert list(m) == ["ACC3D_0_05", "ACC3D_0_1", "Outliers3D", "RobustOutliers3D", "AEE", "AVG_FLOW_VECTOR",
                           "AVG_FLOW_VECTOR_LENGTH", "AVG_GT_FLOW_VECTOR", "AVG_GT_FLOW_VECTOR_LENGTH", "AVG_ERROR_FLOW_VECTOR",
                           "num_pts_used", "mean_gt_flow"]
        for r in RATIOS:
            ref = float(ref_get(key, r))
            if np.isnan(ref):
                assert np.isnan(m[r]), (key, r)
            else:  # the counts themselves are exact: ratio * n recovers the same integer
                assert round(ref * n) == round(m[r] * n) and abs(ref - m[r]) <= 1e-12, (key, r, ref, m[r])
        _close(m["AEE"], ref_get(key, "AEE"), 1e-6)
        for k in ("AVG_FLOW_VECTOR_LENGTH", "AVG_GT_FLOW_VECTOR_LENGTH", "mean_gt_flow"):
            _close(m[k], ref_get(key, k), 1e-6)
        # vector means: components near zero are relative to the mean length (the reference sums f32)
        _close(m["AVG_FLOW_VECTOR"], ref_get(key, "AVG_FLOW_VECTOR"), 1e-6, float(np.nan_to_num(ref_get(key, "AVG_FLOW_VECTOR_LENGTH"))))
        _close(m["AVG_GT_FLOW_VECTOR"], ref_get(key, "AVG_GT_FLOW_VECTOR"), 1e-6, float(np.nan_to_num(ref_get(key, "mean_gt_flow"))))
        _close(m["AVG_ERROR_FLOW_VECTOR"], ref_get(key, "AVG_ERROR_FLOW_VECTOR"), 1e-6, float(np.nan_to_num(ref_get(key, "AEE"))))


@pytest.mark.parametrize("case", ["mixed", "custom_bins", "no_moving", "empty_overall"])
def test_accumulator_matches_the_reference(golden, case):
    from liso_amd.eval.flow_metrics import FlowMetrics, FlowMetricsState
    from liso_amd.slim.utils.metrics import category_metrics

    z = golden
    bins = z[f"{case}__bins"]
    st = FlowMetricsState(torch.device("cuda"))
    for bt in _batches(z, case):
        epe = torch.empty((3,) + tuple(bt["valid"].shape), dtype=torch.float32, device="cuda")
        st.update(bt["points"], bt["gt"], [bt["preds"][k] for k in range(3)], bt["valid"], bt["moving"], bt["label"], bins, epe)
        e = epe.cpu().numpy()
        assert np.array_equal(np.isnan(e), np.isnan(bt["epe"]))
        fin = ~np.isnan(e)
        assert np.array_equal(e[fin].view(np.uint32), bt["epe"][fin].view(np.uint32))  # bit for bit
    r = st.read()
    keys_ref = [str(k) for k in z[f"{case}__keys"]]
    mine = {}
    for cat in ("overall", "moving", "still"):
        for k, f in enumerate(FLOWS):
            m = category_metrics(r, k, cat)
            if m is not None:
                mine[f"{f}/{cat}"] = m
    assert list(mine) == keys_ref
    _check_metrics(mine, lambda key, mk: z[f"{case}__m__{key}__{mk}"], keys_ref)
    if case == "empty_overall":
        assert int(r["empty_overall"]) == 1 and np.isnan(mine["raw/overall"]["AEE"])
    for k, f in enumerate(FLOWS):
        fm = FlowMetrics._view(st, k, bins)
        for c in ("still", "moving", "overall"):
            pre = f"{case}__fm__{f}__"
            assert np.array_equal(fm.num_points_in_range_bin[c], z[pre + f"num_points_in_range_bin__{c}"]), (f, c)
            assert fm.total_num_pts[c] == int(z[pre + f"total_num_pts__{c}"])
            _close(fm.aee_per_range_bin[c], z[pre + f"aee_per_range_bin__{c}"], 1e-6)
            _close(fm.total_aees[c], z[pre + f"total_aees__{c}"], 1e-6)


def test_public_functions_match_the_reference(golden):
    """the reference's call sequence through the public names: FlowMetrics.update per sample, compute_scene_flow_metrics... per
    batch and category, aggregate_metrics"""
    from liso_amd.eval.flow_metrics import FlowMetrics
    from liso_amd.slim.utils import metrics as M

    z, case = golden, "empty_overall"
    lists = {f"{f}/{c}": [] for c in ("overall", "moving", "still") for f in FLOWS}
    fms = {f: FlowMetrics() for f in FLOWS}
    for bt in _batches(z, case):
        mm = bt["moving"] & bt["valid"] & bt["label"]
        sm = ~mm & bt["valid"] & bt["label"]
        for k, f in enumerate(FLOWS):
            flow = bt["preds"][k]
            for b in range(flow.shape[0]):
                fms[f].update(points=bt["points"][b], flow_pred=flow[b], flow_gt=bt["gt"][b], is_moving=mm[b], mask=bt["valid"][b])
            lists[f"{f}/overall"].append(M.compute_scene_flow_metrics_for_points_in_this_mask(flow, bt["gt"], mm | sm))
            if int(mm.sum()) > 0:
                lists[f"{f}/moving"].append(M.compute_scene_flow_metrics_for_points_in_this_mask(flow, bt["gt"], mm))
            if int(sm.sum()) > 0:
                lists[f"{f}/still"].append(M.compute_scene_flow_metrics_for_points_in_this_mask(flow, bt["gt"], sm))
            if int((mm | sm).sum()) > 0:
                ratios = M.get_inlier_outlier_ratios(flow, bt["gt"], mm | sm)
                d = lists[f"{f}/overall"][-1]
                assert ratios == {r: d[r] for r in RATIOS}
                epe = torch.from_numpy(np.linalg.norm(flow.cpu().numpy() - bt["gt"].cpu().numpy(), axis=-1)).cuda()
                assert M.get_ratio_for_thresh(epe, 0.3, 0.3, bt["gt"], mm | sm, "outliers", True) == d["RobustOutliers3D"]
    keys = [k for k, v in lists.items() if v]
    assert keys == [str(k) for k in z[f"{case}__keys"]]
    mine = {k: M.aggregate_metrics(lists[k]) for k in keys}
    _check_metrics(mine, lambda key, mk: z[f"{case}__m__{key}__{mk}"], keys)
    for f in FLOWS:
        pre = f"{case}__fm__{f}__"
        for c in ("still", "moving", "overall"):
            assert np.array_equal(fms[f].num_points_in_range_bin[c], z[pre + f"num_points_in_range_bin__{c}"])
            _close(fms[f].aee_per_range_bin[c], z[pre + f"aee_per_range_bin__{c}"], 1e-6)
        log = fms[f].log_metrics_curves(0, writer_prefix=f)
        assert list(log) == [f"{f}/AEE/still", f"{f}/AEE/moving", f"{f}/AEE/overall"]
        _close([log[f"{f}/AEE/{c}"] for c in ("still", "moving", "overall")],
               [float(z[pre + f"total_aees__{c}"]) for c in ("still", "moving", "overall")], 1e-6)


def _random(seed, B, N, dev):
    g = torch.Generator().manual_seed(seed)
    pts = (torch.rand(B, N, 4, generator=g) - 0.5) * 200
    gt = torch.randn(B, N, 3, generator=g)
    preds = [gt + torch.randn(B, N, 3, generator=g) * s for s in (0.3, 0.1, 0.03)]
    valid = torch.rand(B, N, generator=g) > 0.05
    moving = torch.rand(B, N, generator=g) > 0.6
    label = torch.rand(B, N, generator=g) > 0.04
    return [t.to(dev) for t in (pts, gt)], [p.to(dev) for p in preds], [t.to(dev) for t in (valid, moving, label)]


def test_split_updates_equal_one_update():
    from liso_amd.eval.flow_metrics import FlowMetricsState

    dev = torch.device("cuda")
    (pts, gt), preds, (valid, moving, label) = _random(1, 1, 50000, dev)
    bins = np.linspace(0, 100, 11)
    one, split = FlowMetricsState(dev), FlowMetricsState(dev)
    one.update(pts, gt, preds, valid, moving, label, bins)
    for a, b in ((0, 777), (777, 20000), (20000, 50000)):
        split.update(pts[:, a:b], gt[:, a:b], [p[:, a:b] for p in preds], valid[:, a:b], moving[:, a:b], label[:, a:b], bins)
    r1, r2 = one.read(), split.read()
    for f in ("label_count", "range_count"):
        assert np.array_equal(r1[f], r2[f])
    for f in ("label_sum", "range_sum"):
        assert np.all(np.abs(r1[f] - r2[f]) <= 1e-12 * np.maximum(np.abs(r1[f]), 1.0))
    assert int(r2["updates"]) == 3 and int(r2["empty_overall"]) == 0


def test_bitwise_run_to_run_and_graph_replay():
    from liso_amd.eval.flow_metrics import FlowMetricsState

    dev = torch.device("cuda")
    (pts, gt), preds, (valid, moving, label) = _random(2, 2, 60000, dev)
    bins = np.linspace(0, 100, 11)
    # a packed decoder-style output: three flows as column slices of one [B,N,9] tensor (no copy)
    packed = torch.cat(preds, dim=-1).contiguous()
    views = [packed[..., 3 * k:3 * k + 3] for k in range(3)]

    def run(st):
        st.update(pts, gt, views, valid, moving, label, bins)
        st.update(pts, gt, views, valid, moving, label, bins)

    a, b = FlowMetricsState(dev), FlowMetricsState(dev)
    run(a)
    run(b)
    ra, rb = a.read(), b.read()
    assert ra.tobytes() == rb.tobytes()
    c = FlowMetricsState(dev)
    c.update(pts, gt, [p.contiguous() for p in preds], valid, moving, label, bins)
    c.update(pts, gt, [p.contiguous() for p in preds], valid, moving, label, bins)
    assert c.read().tobytes() == ra.tobytes()  # strided slices == contiguous copies

    g = FlowMetricsState(dev)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run(g)  # warm-up
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run(g)
    g.reset()
    graph.replay()
    torch.cuda.synchronize()
    assert g.read().tobytes() == ra.tobytes()


@pytest.mark.parametrize("B,N", [(1, 0), (1, 1), (1, 255), (1, 257), (4, 1), (2, 1031)])
def test_edge_sizes_inside_guard_bands(B, N):
    from tests.guarded_alloc import guarded

    from liso_amd.eval.flow_metrics import FlowMetricsState

    dev = torch.device("cuda")
    bins = np.linspace(0, 100, 33)  # 32 bins, the maximum
    with guarded() as gd:
        st = FlowMetricsState(dev)
        pts = torch.empty(B, N, 4, device=dev)
        gt = torch.empty(B, N, 3, device=dev)
        preds = [torch.empty(B, N, 3, device=dev) for _ in range(3)]
        valid = torch.empty(B, N, dtype=torch.bool, device=dev)
        moving = torch.empty(B, N, dtype=torch.bool, device=dev)
        label = torch.empty(B, N, dtype=torch.bool, device=dev)
        epe = torch.empty(3, B, N, device=dev)
        (p0, g0), pr0, (v0, m0, l0) = _random(3, B, N, dev)
        pts.copy_(p0), gt.copy_(g0), valid.copy_(v0), moving.copy_(m0), label.copy_(l0)
        for p, q in zip(preds, pr0):
            p.copy_(q)
        st.update(pts, gt, preds, valid, moving, label, bins, epe)
        r = st.read()
        gd.check()
    vm = (valid & moving & label).cpu().numpy()
    vs = (valid & ~moving & label).cpu().numpy()
    assert r["label_count"][:, 0, 0].tolist() == [int(vm.sum())] * 3
    assert r["label_count"][:, 1, 0].tolist() == [int(vs.sum())] * 3
    assert int(r["range_count"][0, 0, 32] + r["range_count"][0, 1, 32]) == int(valid.sum())
    assert int(r["empty_overall"]) == int(vm.sum() + vs.sum() == 0)
    ref = np.stack([np.linalg.norm(p.cpu().numpy() - gt.cpu().numpy(), axis=-1) for p in preds])
    assert np.array_equal(epe.cpu().numpy().view(np.uint32), ref.view(np.uint32))
