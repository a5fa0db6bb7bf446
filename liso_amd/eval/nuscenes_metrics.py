"""nuScenes detection metrics of the detector's validation pass: mAP over the centre-distance thresholds 0.5 / 1 / 2 / 4 m, the
true-positive errors mATE / mASE / mAOE / mAVE / mAAE and NDS (C ABI of the device part: include/liso_nusc_metrics.h).

Mirror of liso/eval/nuscenes_metrics_wrapper.py (`NuscenesObjectDetectionMetrics`: the per-class radial filter, the clamp of the
predictions' sizes, `evaluate`, the scalars `log` writes) and of the part of the nuScenes devkit it drives
(nuscenes/eval/detection/algo.py `accumulate` / `calc_ap` / `calc_tp`, data_classes.py `DetectionMetricData` / `DetectionMetrics`,
eval/common/utils.py `cummean` / `scale_iou` / `yaw_diff`), without the devkit package, its box classes, plots and PDFs.

Where the work is.  The devkit's matching loop walks all predictions of the data set by descending confidence, but its `taken` set
is per sample: it is one greedy walk per frame plus a data-set wide sort.  The walk of every (frame, threshold) runs on the device
in one launch per padded batch (`nusc_match_packed`, liso_det_val_nusc_f32) and leaves the matched pairs and the error terms of
every match; `nusc_match_host` is its numpy restatement, fp32 in the same operation order, equal bit for bit.  The sort, the
cumulative precision / recall, the 101-point interpolations and the cumulative means of the errors are `evaluate()`, on the host in
float64 for the reasons liso_amd/eval/od_metrics.py gives, vectorised over all frames: every accumulated batch is flattened once
to per-prediction arrays, `evaluate()` loops over (class, threshold) only.

As the reference feeds the devkit, every velocity is (0, 0) and every attribute is empty: the velocity error of a match is 0, its
attribute error NaN, which the devkit's cumulative mean turns into 1.  Both are kept, they enter NDS.

Tie rule.  The devkit orders predictions of equal confidence by their position in its list, and the reference's torch.argsort
leaves that position unspecified.  Here: within a frame ascending slot index (the stable `order` of liso_amd.det_nms.order that the
walk follows), across frames ascending frame in order of `update` / `accumulate_matches`.  Scores are carried in fp32.

`sigmoid_scores=True` applies torch.sigmoid in fp32 before anything reads the scores (run_val :494-509).  It is not irrelevant
here although it is monotone: the errors are interpolated BY confidence, and fp32 saturation can make scores equal.  It runs where
the scores are: torch's sigmoid on the device and on the host can differ in the last bit, and so can the confidences reported.  A
score outside [0, 1] is a ValueError (the reference asserts the same, nuscenes_metrics_wrapper.py:185-187).
"""
import ctypes
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from liso_amd import _lib as L
from liso_amd.kabsch.shape_utils import Shape
from liso_amd.utils.device_args import opt_ptr as _p

MAX_BOXES = 1024  # LISO_DET_VAL_MAX_BOXES
MAX_THRESHOLDS = 8  # LISO_NUSC_MAX_THRESHOLDS
DIST_THS = (0.5, 1.0, 2.0, 4.0)
DIST_TH_TP, MIN_RECALL, MIN_PRECISION, MEAN_AP_WEIGHT, NELEM = 2.0, 0.1, 0.1, 5, 101
MOVABLE_RANGES = {"movable": 50}
PER_CLASS_RANGES = {"car": 50, "truck": 50, "bus": 50, "trailer": 50, "construction_vehicle": 50, "pedestrian": 40, "motorcycle": 40,
                    "bicycle": 40}
NUSC_MOVABLE_CLASSES = ("car", "truck", "trailer", "bus", "construction_vehicle", "bicycle", "motorcycle", "pedestrian")  # by class id
TP_METRICS = ("trans_err", "scale_err", "orient_err", "vel_err", "attr_err")  # the devkit's order
MEAN_TAGS = {"trans_err": "mATE", "scale_err": "mASE", "orient_err": "mAOE", "vel_err": "mAVE", "attr_err": "mAAE"}
CLASS_TAGS = {"trans_err": "ATE", "scale_err": "ASE", "orient_err": "AOE", "vel_err": "AVE", "attr_err": "AAE"}
OUT_KEYS = ("count", "pairs", "err", "gt_in", "pred_in")


# ---- device path ----------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def nusc_match_packed(gt, pred, order, radius, as_one: bool, thresholds: Sequence[float] = DIST_THS, pred_class=None):
    """The per-frame part for a padded batch, on the device, in one launch with no host sync (graph-capturable).  gt / pred: dicts as
    `det_validation.pack_boxes` lays them out (rows fp32 [F,N,7], valid uint8 [F,N], cls int32 [F,N]); order int32 [F,P]; radius fp32
    [n_classes] (device); pred_class int32 [F,P] replaces pred["cls"] (run_val's transferred classes).
    -> dict of device tensors: count int32 [F,T], pairs int16 [F,T,M,2], err fp32 [F,T,M,3], gt_in uint8 [F,G], pred_in uint8 [F,P]."""
    pc = pred["cls"] if pred_class is None else pred_class
    L.require_cuda(gt["rows"], gt["valid"], gt["cls"], pred["rows"], pred["valid"], pc, order, radius)
    (F, G), P, T = gt["valid"].shape, pred["valid"].shape[1], len(thresholds)
    if pred["valid"].shape[0] != F or tuple(order.shape) != (F, P) or tuple(pc.shape) != (F, P):
        raise L.LisoHipError(f"shapes: gt {(F, G)}, pred {tuple(pred['valid'].shape)}, order {tuple(order.shape)}, classes {tuple(pc.shape)}")
    if G > MAX_BOXES or P > MAX_BOXES or not 1 <= T <= MAX_THRESHOLDS:
        raise L.LisoHipError(f"at most {MAX_BOXES} boxes per frame and 1..{MAX_THRESHOLDS} thresholds, got G={G}, P={P}, T={T}")
    if radius.dtype != torch.float32 or order.dtype != torch.int32 or pc.dtype != torch.int32 or gt["cls"].dtype != torch.int32:
        raise L.LisoHipError("radius must be fp32, order and the classes int32")
    dev, M = gt["rows"].device, min(G, P)
    new = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)  # noqa: E731
    out = {"count": new((F, T), torch.int32), "pairs": new((F, T, M, 2), torch.int16), "err": new((F, T, M, 3), torch.float32),
           "gt_in": new((F, G), torch.uint8), "pred_in": new((F, P), torch.uint8)}
    thr = (ctypes.c_float * T)(*[float(t) for t in thresholds])
    with torch.cuda.device(dev):
        L.check(L.lib().liso_det_val_nusc_f32(F, G, P, _p(gt["rows"]), _p(gt["valid"]), _p(gt["cls"]), _p(pred["rows"]), _p(pred["valid"]),
                                              _p(pc.contiguous()), _p(order.contiguous()), L.ptr(radius), radius.numel(), int(bool(as_one)),
                                              thr, T, _p(out["count"]), _p(out["pairs"]), _p(out["err"]), _p(out["gt_in"]),
                                              _p(out["pred_in"]), L.stream_ptr()), "det_val nusc")
    return out


# ---- numpy restatement ------------------------------------------------------------------------------------------------------------
def _member_host(rows, valid, cls, radius):
    f32 = np.float32
    x, y = rows[..., 0], rows[..., 1]
    ok = np.asarray(valid).astype(bool) & (cls >= 0) & (cls < radius.shape[0])
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.sqrt(x * x + y * y, dtype=f32)
        return ok & (r <= radius[np.where(ok, cls, 0)])  # NaN fails


def nusc_err_terms_host(g, p):
    """(trans, scale, orient) of matched rows g, p fp32 [m,7], each in fp32 operation by operation (include/liso_nusc_metrics.h)"""
    from liso_amd.eval.det_validation import tp_terms_host

    f32 = np.float32
    trans, _, orient = tp_terms_host(g, p)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        s = np.where(p[:, 3:6] < f32(1e-4), f32(1e-4), p[:, 3:6])  # a NaN stays
        inter = (np.minimum(g[:, 3], s[:, 0]) * np.minimum(g[:, 4], s[:, 1])) * np.minimum(g[:, 5], s[:, 2])
        union = (g[:, 3] * g[:, 4]) * g[:, 5] + (s[:, 0] * s[:, 1]) * s[:, 2] - inter
        scale = f32(1.0) - inter / union
    qnan = np.array(0x7FC00000, np.uint32).view(f32)  # one NaN pattern, whatever operation made it
    return trans, np.where(np.isnan(scale), qnan, scale).astype(f32), np.where(np.isnan(orient), qnan, orient).astype(f32)


def nusc_match_host(gt_rows, gt_valid, gt_class, pred_rows, pred_valid, pred_class, order, radius, as_one: bool,
                    thresholds: Sequence[float] = DIST_THS):
    """numpy restatement of liso_det_val_nusc_f32 (the header states every rule): the same outputs, numpy, bit for bit."""
    f32 = np.float32
    g, p = np.ascontiguousarray(gt_rows, f32), np.ascontiguousarray(pred_rows, f32)
    radius, order = np.asarray(radius, f32).reshape(-1), np.asarray(order)
    (F, G), P, T = g.shape[:2], p.shape[1], len(thresholds)
    if G > MAX_BOXES or P > MAX_BOXES or not 1 <= T <= MAX_THRESHOLDS or radius.shape[0] < 1:
        raise L.LisoHipError(f"at most {MAX_BOXES} boxes per frame, 1..{MAX_THRESHOLDS} thresholds and a radius, got G={G}, P={P}, T={T}")
    gc = np.zeros((F, G), np.int32) if as_one else np.asarray(gt_class, np.int32)
    pc = np.zeros((F, P), np.int32) if as_one else np.asarray(pred_class, np.int32)
    g_in, p_in = _member_host(g, gt_valid, gc, radius), _member_host(p, pred_valid, pc, radius)
    M = min(G, P)
    out = {"count": np.zeros((F, T), np.int32), "pairs": np.full((F, T, M, 2), -1, np.int16), "err": np.zeros((F, T, M, 3), f32),
           "gt_in": g_in.astype(np.uint8), "pred_in": p_in.astype(np.uint8)}
    slots = np.arange(G)
    for f in range(F):
        visit = [int(q) for q in order[f] if 0 <= q < P and p_in[f, q]]
        gx, gy = g[f, :, 0], g[f, :, 1]
        for t, thr in enumerate(thresholds):
            thr, free, pairs = f32(thr), g_in[f].copy(), []
            for q in visit:
                cand = free & (gc[f] == pc[f, q])
                if not cand.any():
                    continue
                with np.errstate(invalid="ignore", over="ignore"):
                    dx, dy = gx - p[f, q, 0], gy - p[f, q, 1]
                    d = np.sqrt(dx * dx + dy * dy, dtype=f32)
                    cand &= d < thr  # NaN never passes
                if cand.any():
                    b = int(slots[cand][np.argmin(d[cand])])  # the smallest distance, the lowest slot among equal ones
                    free[b] = False
                    if len(pairs) < M:
                        pairs.append((b, q))
            if pairs:
                pr = np.array(pairs, np.int64)
                out["count"][f, t] = len(pairs)
                out["pairs"][f, t, :len(pairs)] = pr
                out["err"][f, t, :len(pairs)] = np.stack(nusc_err_terms_host(g[f][pr[:, 0]], p[f][pr[:, 1]]), -1)
    return out


# ---- the devkit's curves, float64 --------------------------------------------------------------------------------------------------
def cummean(x):
    """the devkit's NaN-aware cumulative mean (eval/common/utils.py): all NaN -> ones; NaN entries are left out of sum and count"""
    x = np.asarray(x, np.float64)
    nan = np.isnan(x)
    if nan.all():
        return np.ones(len(x))
    s, n = np.nancumsum(x), np.cumsum(~nan)
    return np.divide(s, n, out=np.zeros_like(s), where=n != 0)


def no_predictions():
    """DetectionMetricData.no_predictions(): precision and confidence 0, every error 1"""
    md = {"recall": np.linspace(0, 1, NELEM), "precision": np.zeros(NELEM), "confidence": np.zeros(NELEM)}
    md.update({k: np.ones(NELEM) for k in TP_METRICS})
    return md


def accumulate_curves(conf, tp, errs, npos):
    """`accumulate` after its matching loop (algo.py:122-169).  conf float64 [n], tp bool [n], errs float64 [n,5] (TP_METRICS order;
    read at the true positives only): all predictions of one class in the tie rule's order.  -> dict of 101-point arrays."""
    if npos == 0 or not tp.any():
        return no_predictions()
    srt = np.argsort(-conf, kind="stable")
    conf, tp, errs = conf[srt], tp[srt], errs[srt]
    tp_c, fp_c = np.cumsum(tp).astype(float), np.cumsum(~tp).astype(float)
    prec, rec = tp_c / (fp_c + tp_c), tp_c / float(npos)
    rec_interp = np.linspace(0, 1, NELEM)
    md = {"recall": rec_interp, "precision": np.interp(rec_interp, rec, prec, right=0), "confidence": np.interp(rec_interp, rec, conf, right=0)}
    match_conf = conf[tp]
    for i, k in enumerate(TP_METRICS):
        tmp = cummean(errs[tp, i])
        md[k] = np.interp(md["confidence"][::-1], match_conf[::-1], tmp[::-1])[::-1]
    return md


def calc_ap(md, min_recall=MIN_RECALL, min_precision=MIN_PRECISION):
    prec = np.copy(md["precision"])[round(100 * min_recall) + 1:]  # the bins above min_recall
    prec -= min_precision
    prec[prec < 0] = 0
    return float(np.mean(prec)) / (1.0 - min_precision)


def calc_tp(md, metric_name, min_recall=MIN_RECALL):
    first_ind = round(100 * min_recall) + 1
    non_zero = np.nonzero(md["confidence"])[0]
    last_ind = 0 if len(non_zero) == 0 else int(non_zero[-1])  # max_recall_ind: the last index of non-zero confidence
    if last_ind < first_ind:
        return 1.0
    return float(np.mean(md[metric_name][first_ind: last_ind + 1]))


class NuscenesObjectDetectionMetrics:
    """The reference's collection (liso/eval/nuscenes_metrics_wrapper.py:71-343) without the devkit.

    eval_movable_classes_as_one=True: every box is class "movable", radius 50 m.  False: `class_names` are the names BY CLASS ID
    (default: the reference's nuScenes order) and `class_ranges` maps each to its radius (default: the reference's 50 / 40 m);
    the classes are evaluated in `class_ranges`' order.  The devkit's special cases for "traffic_cone" and "barrier" are not built:
    the reference evaluates neither."""

    def __init__(self, eval_movable_classes_as_one: bool = True, class_names: Optional[Sequence[str]] = None,
                 class_ranges: Optional[Dict[str, float]] = None, sigmoid_scores: bool = False):
        self.eval_movable_classes_as_one, self.sigmoid_scores = bool(eval_movable_classes_as_one), bool(sigmoid_scores)
        if class_ranges is None:
            class_ranges = MOVABLE_RANGES if self.eval_movable_classes_as_one else PER_CLASS_RANGES
            if class_names is not None and not self.eval_movable_classes_as_one:  # a subset of the reference's classes keeps their radii
                class_ranges = {c: r for c, r in PER_CLASS_RANGES.items() if c in class_names}
        if class_names is None:
            class_names = tuple(class_ranges) if self.eval_movable_classes_as_one else NUSC_MOVABLE_CLASSES
        self.class_names, self.class_ranges = tuple(class_names), dict(class_ranges)
        if self.eval_movable_classes_as_one and len(self.class_names) != 1:
            raise ValueError(f"evaluated as one class: one class name, got {self.class_names}")
        bad = [c for c in self.class_names if c not in self.class_ranges or c in ("traffic_cone", "barrier")]
        if bad or set(self.class_ranges) != set(self.class_names):
            raise ValueError(f"class_ranges {sorted(self.class_ranges)} must name exactly the classes {self.class_names}, "
                             "none of them traffic_cone or barrier")
        self.target_class_names = list(self.class_ranges)
        self.radius = np.array([self.class_ranges[c] for c in self.class_names], np.float32)  # by class id
        self.matching_thresholds, self.tp_metric_thresh, self.threshold_unit = DIST_THS, DIST_TH_TP, "m"
        self.min_recall, self.min_precision, self.mean_ap_weight = MIN_RECALL, MIN_PRECISION, MEAN_AP_WEIGHT
        self._radius_dev = {}
        self._conf, self._cls, self._tp, self._err = [], [], [], []  # per accumulated batch, flattened over (frame, slot)
        self._npos = np.zeros(len(self.class_names), np.int64)

    def radius_on(self, device):
        key = str(device)
        if key not in self._radius_dev:
            self._radius_dev[key] = torch.from_numpy(self.radius).to(device)
        return self._radius_dev[key]

    def scores_seen(self, probs):
        """the scores this collection reads: fp32, after the sigmoid when asked for (torch, any device)"""
        probs = probs.float()
        return torch.sigmoid(probs) if self.sigmoid_scores else probs

    # -- accumulation -----------------------------------------------------------------------------------------------------------
    def update(self, *, non_batched_gt_boxes: Shape, non_batched_pred_boxes: Shape, sample_token: str = ""):
        """one frame, the reference's entry: unbatched Shapes [G] / [P] on any device, matched through the numpy restatement"""
        from liso_amd.eval.det_validation import pack_boxes, stable_order_host

        g = {k: v.cpu().numpy() for k, v in pack_boxes(_batch_of_one(non_batched_gt_boxes)).items()}
        pred = _batch_of_one(non_batched_pred_boxes)
        pred.probs = self.scores_seen(pred.probs)
        p = {k: v.cpu().numpy() for k, v in pack_boxes(pred).items()}
        order = stable_order_host(p["score"], p["valid"])
        o = nusc_match_host(g["rows"], g["valid"], g["cls"], p["rows"], p["valid"], p["cls"], order, self.radius, self.eval_movable_classes_as_one)
        self.accumulate_matches(p["score"], p["cls"], g["cls"], **o)

    def accumulate_matches(self, score, pred_class, gt_class, count, pairs, err, gt_in, pred_in):
        """The entry for matches made elsewhere (`nusc_match_packed` on the device, `nusc_match_host`), one padded batch: score fp32
        [F,P] as the walk's `order` saw them (after the sigmoid when asked for), pred_class int [F,P] and gt_class int [F,G] as the
        walk read them, and the walk's outputs.  Flattens the batch to per-prediction arrays, vectorised over the frames."""
        score, p_in, g_in = np.asarray(score, np.float32), np.asarray(pred_in).astype(bool), np.asarray(gt_in).astype(bool)
        count, pairs, err = np.asarray(count), np.asarray(pairs), np.asarray(err)
        F, P = p_in.shape
        T, M = count.shape[1], pairs.shape[2]
        assert T == len(self.matching_thresholds), (T, self.matching_thresholds)
        conf = score[p_in]
        if not np.all((conf >= 0.0) & (conf <= 1.0)):  # NaN fails
            raise ValueError("nuScenes metrics need confidences in [0, 1] (sigmoid_scores=True for raw logits)")
        as_one = self.eval_movable_classes_as_one
        self._npos += np.bincount(np.zeros(int(g_in.sum()), np.int64) if as_one else np.asarray(gt_class)[g_in].astype(np.int64),
                                  minlength=len(self.class_names))
        n = conf.shape[0]
        lut = (np.cumsum(p_in.reshape(-1)) - 1).reshape(F, P)  # (frame, slot) -> position among the members, frame-major
        tp, e = np.zeros((T, n), bool), np.zeros((T, n, 3), np.float32)
        for t in range(T):
            fi, mi = np.nonzero(np.arange(M)[None, :] < count[:, t, None])
            at = lut[fi, pairs[fi, t, mi, 1].astype(np.int64)]
            tp[t, at], e[t, at] = True, err[fi, t, mi]
        self._conf.append(conf)
        self._cls.append(np.zeros(n, np.int64) if as_one else np.asarray(pred_class)[p_in].astype(np.int64))
        self._tp.append(tp)
        self._err.append(e)

    # -- the numbers ------------------------------------------------------------------------------------------------------------
    def evaluate(self):
        """`evaluate()` + DetectionMetrics.serialize(): dict(label_aps {class: {thr: AP}}, label_tp_errors {class: {metric: value}},
        mean_dist_aps, mean_ap, tp_errors, tp_scores, nd_score, metric_data {(class, thr): dict of the 101-point arrays})"""
        T = len(self.matching_thresholds)
        cat = lambda parts, axis, empty, dt: np.concatenate(parts, axis=axis) if parts else np.zeros(empty, dt)  # noqa: E731
        conf, cls = cat(self._conf, 0, (0,), np.float32).astype(np.float64), cat(self._cls, 0, (0,), np.int64)
        tp, err = cat(self._tp, 1, (T, 0), bool), cat(self._err, 1, (T, 0, 3), np.float32)
        if len(self._conf) > 1:  # keep the flattened state: a later evaluate() concatenates nothing again
            self._conf, self._cls, self._tp, self._err = [conf.astype(np.float32)], [cls], [tp], [err]
        md, aps, tps = {}, {}, {}
        for name in self.target_class_names:
            c = self.class_names.index(name)
            sel = cls == c
            errs = np.zeros((int(sel.sum()), 5))
            errs[:, 4] = np.nan  # no attributes: NaN per match; velocities (0, 0): 0 per match
            for t, thr in enumerate(self.matching_thresholds):
                errs[:, :3] = err[t][sel]
                md[(name, thr)] = accumulate_curves(conf[sel], tp[t][sel], errs, int(self._npos[c]))
            aps[name] = {thr: calc_ap(md[(name, thr)], self.min_recall, self.min_precision) for thr in self.matching_thresholds}
            tps[name] = {k: calc_tp(md[(name, self.tp_metric_thresh)], k, self.min_recall) for k in TP_METRICS}
        mean_dist_aps = {name: float(np.mean(list(aps[name].values()))) for name in aps}
        tp_errors = {k: float(np.nanmean([tps[name][k] for name in self.target_class_names])) for k in TP_METRICS}
        tp_scores = {k: max(0.0, 1.0 - tp_errors[k]) for k in TP_METRICS}
        mean_ap = float(np.mean(list(mean_dist_aps.values())))
        nd_score = float(self.mean_ap_weight * mean_ap + np.sum(list(tp_scores.values()))) / float(self.mean_ap_weight + len(tp_scores))
        return {"label_aps": aps, "label_tp_errors": tps, "mean_dist_aps": mean_dist_aps, "mean_ap": mean_ap, "tp_errors": tp_errors,
                "tp_scores": tp_scores, "nd_score": nd_score, "metric_data": md}

    def compute(self, writer_prefix: str = "") -> Dict[str, float]:
        """the scalars the reference's `log()` writes (:260-339), under `writer_prefix.rstrip("/")`"""
        r, p = self.evaluate(), writer_prefix.rstrip("/")
        out = {f"{p}/mAP": r["mean_ap"]}
        out.update({f"{p}/{MEAN_TAGS[k]}": v for k, v in r["tp_errors"].items()})
        out[f"{p}/NDS"] = r["nd_score"]
        for name, ap in r["mean_dist_aps"].items():
            out[f"{p}/{name}/AP"] = ap
            out.update({f"{p}/{name}/{CLASS_TAGS[k]}": v for k, v in r["label_tp_errors"][name].items()})
        return out


def _batch_of_one(boxes: Shape) -> Shape:
    return Shape.from_list_of_shapes([boxes.clone()])
