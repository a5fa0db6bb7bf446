"""Scene-flow validation metrics on the device.  Mirror of liso/eval/flow_metrics.py (FlowMetrics: AEE per range bin of still /
moving / overall points) on the accumulator of include/liso_flow_metrics.h, which also carries the label-category statistics of
liso/slim/utils/metrics.py (liso_amd/slim/utils/metrics.py).

`FlowMetricsState` is the device state: `update` enqueues two launches and never synchronises (graph-capturable once the state
exists); `read()` is the one device->host copy.  Plotting and TensorBoard images of the reference's `log_metrics_curves` are not
part of this package."""
import ctypes

import numpy as np
import torch

from liso_amd import _lib as L

MAX_FLOWS, MAX_BINS = 3, 32
# liso_flow_metrics_result (include/liso_flow_metrics.h)
RESULT_DTYPE = np.dtype([("label_count", "<u8", (MAX_FLOWS, 2, 5)), ("label_sum", "<f8", (MAX_FLOWS, 2, 12)),
                         ("range_count", "<u8", (MAX_FLOWS, 2, MAX_BINS + 1)), ("range_sum", "<f8", (MAX_FLOWS, 2, MAX_BINS + 1)),
                         ("empty_overall", "<u4"), ("updates", "<u4"), ("reserved", "<u4", (2,))])
# label categories [moving, still]; range categories [still, moving]
LABEL_MOVING, LABEL_STILL = 0, 1
RANGE_STILL, RANGE_MOVING = 0, 1


def _rows(t, what, last, dtype):
    """-> (tensor with rows of a single stride, rows, row stride in elements); `t` is [N,last] / [B,N,last] (last = None: >= 3)"""
    if not torch.is_tensor(t):
        raise TypeError(f"{what}: expected a torch.Tensor, got {type(t).__name__}")
    if t.dtype != dtype:
        raise TypeError(f"{what}: expected {dtype}, got {t.dtype}")
    if t.dim() not in (2, 3) or (last is not None and t.shape[-1] != last) or (last is None and t.shape[-1] < 3):
        raise ValueError(f"{what}: expected [N,{last or '>=3'}] or [B,N,{last or '>=3'}], got {tuple(t.shape)}")
    def row_stride(t):
        if t.shape[-2] > 1:
            return t.stride(-2)
        return t.stride(0) if t.dim() == 3 and t.shape[0] > 1 else t.shape[-1]

    if (t.stride(-1) != 1 or row_stride(t) < t.shape[-1]
            or (t.dim() == 3 and t.shape[0] > 1 and t.shape[1] > 1 and t.stride(0) != t.shape[1] * t.stride(1))):
        t = t.contiguous()
    return t, t.numel() // t.shape[-1], row_stride(t)


def _mask(t, what, shape):
    if not torch.is_tensor(t):
        raise TypeError(f"{what}: expected a torch.Tensor, got {type(t).__name__}")
    if t.dtype != torch.bool:
        raise TypeError(f"{what}: expected torch.bool, got {t.dtype}")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
    return t.contiguous()


def check_bins(range_bins):
    edges = np.asarray(range_bins, dtype=np.float64).reshape(-1)
    if edges.size - 1 > MAX_BINS:
        raise ValueError(f"at most {MAX_BINS} range bins ({MAX_BINS + 1} edges), got {edges.size - 1}")
    if edges.size == 1 or (edges.size > 1 and not np.all(edges[:-1] <= edges[1:])):
        raise ValueError(f"range bin edges must be >= 2 non-decreasing numbers, got {edges}")
    return np.ascontiguousarray(edges)


class FlowMetricsState:
    """One device accumulator (include/liso_flow_metrics.h) for up to three predicted flows of the same points."""

    def __init__(self, device):
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        nbytes = L.lib().liso_flow_metrics_state_bytes()
        assert L.lib().liso_flow_metrics_result_bytes() == RESULT_DTYPE.itemsize
        self.buf = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        self.reset()

    def reset(self):
        with torch.cuda.device(self.device):
            L.check(L.lib().liso_flow_metrics_reset(L.ptr(self.buf), L.stream_ptr()), "flow_metrics_reset")

    def update(self, points, gt_flow, pred_flows, pcl_is_valid, moving_mask, has_flow_label=None, range_bins=None, point_epe=None):
        """points [.., >=3] (None when range_bins is None), gt_flow / pred_flows[k] [.., 3] f32, masks bool; [N,..] or [B,N,..]"""
        edges = None if range_bins is None else check_bins(range_bins)
        preds = list(pred_flows)
        if not 1 <= len(preds) <= MAX_FLOWS:
            raise ValueError(f"1 to {MAX_FLOWS} predicted flows, got {len(preds)}")
        gt, rows, gst = _rows(gt_flow, "gt_flow", 3, torch.float32)
        lead = tuple(gt.shape[:-1])
        pp = []
        for k, p in enumerate(preds):
            p2, r, s = _rows(p, f"pred_flow[{k}]", 3, torch.float32)
            if tuple(p2.shape[:-1]) != lead:
                raise ValueError(f"pred_flow[{k}]: shape {tuple(p.shape)} does not match gt_flow {tuple(gt_flow.shape)}")
            pp.append((p2, s))
        pts, pst = None, 0
        if edges is not None:
            if points is None:
                raise ValueError("range bins need the points")
            pts, _, pst = _rows(points, "points", None, torch.float32)
            if tuple(pts.shape[:-1]) != lead:
                raise ValueError(f"points: shape {tuple(points.shape)} does not match gt_flow {tuple(gt_flow.shape)}")
        valid = _mask(pcl_is_valid, "pcl_is_valid", lead)
        moving = _mask(moving_mask, "moving_mask", lead)
        label = None if has_flow_label is None else _mask(has_flow_label, "point_has_valid_flow_label", lead)
        if point_epe is not None and (point_epe.dtype != torch.float32 or not point_epe.is_contiguous()
                                      or point_epe.numel() != len(preds) * rows):
            raise ValueError(f"point_epe: expected a contiguous float32 tensor of {len(preds)} x {rows} elements")
        tensors = [gt, valid, moving] + [p for p, _ in pp] + [t for t in (pts, label, point_epe) if t is not None]
        L.require_cuda(*tensors)
        if any(t.device != self.device for t in tensors):
            raise ValueError(f"every tensor must be on {self.device}")
        while len(pp) < MAX_FLOWS:
            pp.append((None, 0))
        nb = 0 if edges is None else edges.size - 1
        e = edges.ctypes.data_as(ctypes.c_void_p) if nb > 0 else None
        with torch.cuda.device(self.device):
            L.check(L.lib().liso_flow_metrics_update(
                L.ptr(self.buf), rows, L.ptr(pts) if pts is not None else None, pst, L.ptr(gt), gst, len(preds),
                *[a for p, s in pp for a in ((L.ptr(p) if p is not None else None), s)],
                L.ptr(valid), L.ptr(moving), L.ptr(label) if label is not None else None, e, nb,
                L.ptr(point_epe) if point_epe is not None else None, L.stream_ptr()), "flow_metrics_update")

    def read(self):
        """-> numpy record of RESULT_DTYPE (the one device->host copy; waits for the current stream)"""
        out = np.zeros((), dtype=RESULT_DTYPE)
        with torch.cuda.device(self.device):
            L.check(L.lib().liso_flow_metrics_read(L.ptr(self.buf), out.ctypes.data_as(ctypes.c_void_p), L.stream_ptr()),
                    "flow_metrics_read")
        return out


class FlowMetrics:
    """liso/eval/flow_metrics.py:13-180.  `update` takes device tensors and never synchronises; the reference's attributes
    `aee_per_range_bin`, `num_points_in_range_bin`, `total_aees`, `total_num_pts` (same dict layout) are read from the device on
    access.  The reference keeps running averages; here the EPE sums are f64 and divided on reading."""

    def __init__(self, range_bins=None, device=None):
        if range_bins is None:
            range_bins = np.linspace(start=0.0, stop=100.0, num=11)
        self._edges = check_bins(range_bins)
        self.range_bins = np.array(range_bins)
        self.categories = ("still", "moving", "overall")
        self.colors = ("green", "red", "blue")
        self._state, self._flow = None, 0
        if device is not None:
            self._state = FlowMetricsState(device)

    @classmethod
    def _view(cls, state, flow, range_bins, result=None):
        """the range statistics of flow `flow` of a shared FlowMetricsState (run_eval_on_this_dataset); `result`: a read
        already made"""
        fm = cls(range_bins)
        fm._state, fm._flow, fm._result = state, flow, result
        return fm

    def update(self, points, flow_pred, flow_gt, is_moving, mask):
        """reference :32-80: points [N,>=3] / [B,N,>=3], flows [..,3] f32, is_moving / mask bool"""
        if self._state is None:
            if not torch.is_tensor(flow_gt):
                raise TypeError("FlowMetrics.update takes device tensors")
            L.require_cuda(flow_gt)
            self._state = FlowMetricsState(flow_gt.device)
        self._result = None
        self._state.update(points, flow_gt, [flow_pred], mask, is_moving, None, self._edges)

    def _read(self):
        r = getattr(self, "_result", None)
        if r is None:
            if self._state is None:
                r = np.zeros((), dtype=RESULT_DTYPE)
            else:
                r = self._state.read()
        return r

    def _tables(self):
        r = self._read()
        nb = self._edges.size - 1
        cnt = r["range_count"][self._flow].astype(np.int64)
        sm = r["range_sum"][self._flow]
        c = {"still": cnt[RANGE_STILL], "moving": cnt[RANGE_MOVING], "overall": cnt[RANGE_STILL] + cnt[RANGE_MOVING]}
        s = {"still": sm[RANGE_STILL], "moving": sm[RANGE_MOVING], "overall": sm[RANGE_STILL] + sm[RANGE_MOVING]}
        return nb, c, s

    @property
    def num_points_in_range_bin(self):
        nb, c, _ = self._tables()
        return {k: c[k][:nb].copy() for k in self.categories}

    @property
    def aee_per_range_bin(self):
        nb, c, s = self._tables()
        return {k: np.divide(s[k][:nb], c[k][:nb], out=np.zeros(nb, np.float64), where=c[k][:nb] > 0) for k in self.categories}

    @property
    def total_num_pts(self):
        _, c, _ = self._tables()
        return {k: int(c[k][MAX_BINS]) for k in self.categories}

    @property
    def total_aees(self):
        _, c, s = self._tables()
        return {k: float(s[k][MAX_BINS] / c[k][MAX_BINS]) if c[k][MAX_BINS] > 0 else 0.0 for k in self.categories}

    def log_metrics_curves(self, global_step, summary_writer=None, writer_prefix="", path=None):
        """reference :82-180 without its figures: -> {<prefix>/AEE/<category>: total AEE}"""
        if summary_writer is not None or path is not None:
            raise NotImplementedError("FlowMetrics.log_metrics_curves: plots and TensorBoard images are not part of liso_amd; "
                                      "log the returned scalars instead")
        summary_prefix = writer_prefix.rstrip("/")
        aees = self.total_aees
        return {summary_prefix + "/AEE/" + k: aees[k] for k in self.categories}
