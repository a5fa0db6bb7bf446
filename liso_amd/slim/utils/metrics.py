"""Scene-flow metrics of SLIM's validation pass.  Mirror of liso/slim/utils/metrics.py (same functions, signatures and keys) on
device tensors: the per-point work runs in the accumulator of include/liso_flow_metrics.h (liso_amd/eval/flow_metrics.py), and
each call reads its numbers from the device once.  Batched [B,N,3] flows and [B,N] masks are taken as the reference receives
them (experiment.py:800-822); [N,3] / [N] as well.

Means here are f64 sums divided by integer counts; the reference averages f32 arrays with numpy (pairwise f32 sums), so the
means agree to ~1e-7 relative while counts and ratios agree exactly.  An empty mask gives NaN for every value but
`num_pts_used` (0): with the installed numpy the reference raises ZeroDivisionError in `get_ratio_for_thresh` instead
(np.count_nonzero returns a Python int)."""
import numpy as np
import torch

from liso_amd.eval.flow_metrics import LABEL_MOVING, LABEL_STILL, FlowMetricsState

_STATES = {}  # (device, stream) -> FlowMetricsState of the one-call functions below

_RATIO_KEYS = ("ACC3D_0_05", "ACC3D_0_1", "Outliers3D", "RobustOutliers3D")


def _state(device):
    """the scratch accumulator of the calling stream: reset, updated and read on that stream inside one call (the read waits for
    it), so calls on different streams never share a state, and calls on one stream are ordered by the stream.  (These one-call
    functions read the device and cannot be captured into a hipGraph; a captured validation step owns a FlowMetricsState.)"""
    with torch.cuda.device(device):
        key = (device, torch.cuda.current_stream().cuda_stream)
    st = _STATES.get(key)
    if st is None:
        st = _STATES[key] = FlowMetricsState(device)
    else:
        st.reset()
    return st


def _one_mask_result(pred_flow, gt_flow, mask):
    """the label statistics of `mask` (label "moving" category = mask & mask & mask) for one flow: one update, one read"""
    st = _state(gt_flow.device)
    st.update(None, gt_flow, [pred_flow], mask, mask)
    r = st.read()
    return r["label_count"][0, LABEL_MOVING], r["label_sum"][0, LABEL_MOVING]


def metrics_from_sums(count, sums):
    """the dict of compute_scene_flow_metrics_for_points_in_this_mask from the accumulated counts [5] and sums [12] of one category
    (include/liso_flow_metrics.h: LISO_FM_* order)"""
    n = int(count[0])
    if n == 0:
        nan = float("nan")
        nan3 = np.full(3, np.nan)
        return {**{k: nan for k in _RATIO_KEYS}, "AEE": nan, "AVG_FLOW_VECTOR": nan3, "AVG_FLOW_VECTOR_LENGTH": nan,
                "AVG_GT_FLOW_VECTOR": nan3.copy(), "AVG_GT_FLOW_VECTOR_LENGTH": nan, "AVG_ERROR_FLOW_VECTOR": nan3.copy(),
                "num_pts_used": 0, "mean_gt_flow": nan}
    s = np.asarray(sums, dtype=np.float64)
    return {
        **{k: int(count[1 + i]) / n for i, k in enumerate(_RATIO_KEYS)},
        "AEE": float(s[0] / n),
        "AVG_FLOW_VECTOR": s[1:4] / n,
        "AVG_FLOW_VECTOR_LENGTH": float(s[4] / n),
        "AVG_GT_FLOW_VECTOR": s[5:8] / n,
        "AVG_GT_FLOW_VECTOR_LENGTH": float(s[8] / n),
        "AVG_ERROR_FLOW_VECTOR": s[9:12] / n,
        "num_pts_used": n,
        "mean_gt_flow": float(s[8] / n),
    }


def aggregate_metrics(list_of_metrics_dicts_overall):
    """reference :4-17 (host numbers): every value weighted by `num_pts_used`, vectors elementwise"""
    in_out_liers_dict_overall = {}
    just_accumulate = ["num_pts_used"]
    for k, _v in list_of_metrics_dicts_overall[0].items():
        if k in just_accumulate:
            in_out_liers_dict_overall[k] = sum(el[k] for el in list_of_metrics_dicts_overall)
            continue
        in_out_liers_dict_overall[k] = sum(el[k] * el["num_pts_used"] for el in list_of_metrics_dicts_overall) / sum(
            el["num_pts_used"] for el in list_of_metrics_dicts_overall)
    return in_out_liers_dict_overall


def get_inlier_outlier_ratios(pred_flow, gt_flow, inspect_these_points_mask):
    """reference :20-70"""
    count, _ = _one_mask_result(pred_flow, gt_flow, inspect_these_points_mask)
    n = int(count[0])
    return {k: int(count[1 + i]) / n if n else float("nan") for i, k in enumerate(_RATIO_KEYS)}


def get_ratio_for_thresh(end_point_errors, abs_thresh, rel_thresh, gt_flow, inspect_these_points_mask, mode, abs_AND_rel: bool):
    """reference :73-110 for any thresholds, one host read.  Unlike the functions above this one does not run on the
    liso_flow_metrics kernel (whose four thresholds are fixed): it is torch elementwise f32 arithmetic on the device in numpy's order,
    |gt| = sqrt((x*x + y*y) + z*z) as separate operations and the thresholds compared as f32.  Its counts equal numpy's as long as
    torch's f32 sqrt and division on the device are correctly rounded (hipcc's default, which PyTorch's ROCm build keeps);
    `end_point_errors` is taken as given."""
    assert mode in ["inliers", "outliers"]
    g = gt_flow.float()
    sq = g * g
    relative_error = end_point_errors / torch.sqrt((sq[..., 0] + sq[..., 1]) + sq[..., 2])
    if mode == "inliers":
        point_is_inlier_absolute = end_point_errors < abs_thresh
        point_is_inlier_relative = relative_error < rel_thresh
    else:
        point_is_inlier_absolute = end_point_errors > abs_thresh
        point_is_inlier_relative = relative_error > rel_thresh
    if abs_AND_rel:
        point_is_inlier = point_is_inlier_absolute & point_is_inlier_relative
    else:
        point_is_inlier = point_is_inlier_absolute | point_is_inlier_relative
    counts = torch.stack([(point_is_inlier & inspect_these_points_mask).sum(), inspect_these_points_mask.sum()]).cpu()
    num_inliers, num_pts_total = int(counts[0]), int(counts[1])
    return num_inliers / num_pts_total if num_pts_total else float("nan")


def compute_scene_flow_metrics_for_points_in_this_mask(pred_flow, gt_flow, mask):
    """reference :113-137"""
    count, sums = _one_mask_result(pred_flow, gt_flow, mask)
    return metrics_from_sums(count, sums)


def category_metrics(result, flow, category):
    """the aggregated dict of label category `category` ("overall" / "moving" / "still") of flow `flow` of a FlowMetricsState read
    (run_eval_on_this_dataset); None when the reference would have appended nothing"""
    cnt, sm = result["label_count"][flow], result["label_sum"][flow]
    if category == "overall":
        m = metrics_from_sums(cnt[LABEL_MOVING] + cnt[LABEL_STILL], sm[LABEL_MOVING] + sm[LABEL_STILL])
        if int(result["empty_overall"]):  # one batch gave an all-NaN dict (num_pts_used 0): its weighted sums are NaN
            m = {k: (v if k == "num_pts_used" else (np.full(3, np.nan) if isinstance(v, np.ndarray) else float("nan"))) for k, v in m.items()}
        return m
    c = LABEL_MOVING if category == "moving" else LABEL_STILL
    return metrics_from_sums(cnt[c], sm[c]) if int(cnt[c][0]) > 0 else None
