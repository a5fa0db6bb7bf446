"""SLIM's validation pass on the device: liso/slim/experiment.py:580-833 (`run_eval_on_this_dataset`) without its images.

Per batch: one forward-direction SLIM inference of the three evaluated flows (SLIM.infer_eval_flows) and ONE metrics update of
all three into a device accumulator (include/liso_flow_metrics.h) -- no host sync.  The numbers are read once at the end."""
import numpy as np
import torch

from liso_amd.eval.flow_metrics import FlowMetrics, FlowMetricsState, check_bins
from liso_amd.slim.utils.metrics import category_metrics

FLOW_KINDS = ("raw", "agg", "rig")
_CATEGORIES = ("overall", "moving", "still")


def run_eval_on_this_dataset(model, val_batches, max_iterations=None, range_bins=None):
    """`model`: SLIM (eval mode is the caller's business, as in the reference); `val_batches`: iterable of (sample_t0, sample_t1,
    ...) in the reference's sample layout with `gt.flow_ta_tb`, `gt.moving_mask`, `gt.point_has_valid_flow_label`.
    -> (eval_metrics, flow_metrics): eval_metrics keyed "raw/overall", "agg/overall", "rig/overall", "raw/moving", ... like the
    reference's, a key present only where the reference would have appended a dict; flow_metrics {raw, agg, rig: FlowMetrics}."""
    edges = check_bins(np.linspace(start=0.0, stop=100.0, num=11) if range_bins is None else range_bins)
    dev = next(model.parameters()).device
    state = FlowMetricsState(dev)
    n = 0
    with torch.no_grad():
        for batch in val_batches:
            if max_iterations is not None and n >= max_iterations:  # the reference's `num_val_steps > max_iterations` break
                break
            s0, s1 = batch[0], batch[1]
            n += 1
            pred = model.infer_eval_flows(s0, s1)
            pa, gt = s0["pcl_ta"], s0["gt"]
            state.update(pa["pcl"].to(dev), gt["flow_ta_tb"].to(dev),
                         [pred.static_flow, pred.aggregated_flow, pred.static_aggr_flow], pa["pcl_is_valid"].to(dev),
                         gt["moving_mask"].to(dev), gt["point_has_valid_flow_label"].to(dev), edges)
    result = state.read()
    eval_metrics = {}
    if n:
        for cat in _CATEGORIES:
            for k, name in enumerate(FLOW_KINDS):
                m = category_metrics(result, k, cat)
                if m is not None:
                    eval_metrics[f"{name}/{cat}"] = m
    flow_metrics = {name: FlowMetrics._view(state, k, edges, result) for k, name in enumerate(FLOW_KINDS)}
    return eval_metrics, flow_metrics
