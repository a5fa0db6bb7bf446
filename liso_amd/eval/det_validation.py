"""Detector validation with all the matching on the device (C ABI: include/liso_det_val.h).

The reference's run_val (liso/eval/eval_ours.py:120-757) feeds every frame to many `ObjectDetectionMetrics` collections, each
of which filters the boxes, builds a pair matrix and walks the predictions once per class and threshold: more than a hundred
matchings, launches and host reads per frame.  Here one call matches ALL frames of a padded batch against ALL collections in at
most three launches of the project's kernels (four with Waymo-style collections) and reads nothing back:

  `match_detections`       the device call on padded `Shape` batches, device tensors only
  `match_detections_host`  its numpy restatement (pair matrices: an argument, by default the library's host twin)
  `DetectionValidator`     the metric collections of a validation pass: `update_batch` appends device outputs without a host
                           sync, `flush` moves what is pending to the host in one read, `compute` feeds the existing
                           `ObjectDetectionMetrics` book-keeping and AP code (the precision / recall sweep stays on the host,
                           liso_amd/eval/od_metrics.py says why) and returns the reference's tags.

Tie rule: predictions of equal score are visited in ascending slot index (`liso_amd.det_nms.order`, a stable sort); the
reference's torch.argsort leaves that order unspecified.  Scores are carried in fp32, the dtype `predict_boxes` returns.

Waymo-style collections (`Collection(..., kind="waymo")`, `WaymoObjectDetectionMetrics`: L1 / L2 AP@0.4) do not walk greedily: they
keep the pairs of an OPTIMAL assignment on the IoU.  Their jobs live in assignment tables of their own (`JobTable(assignment=True)`,
one per ground-truth set) and run in one more launch per set, liso_det_val_assign_f32: a shortest-augmenting-path solver, one
wavefront per (job, frame) cell; `assign_host` is its numpy restatement.  Tie rule: which of several equally good assignments is
taken is this package's own rule, the one `assign_host` states (rows in ascending slot order; among equal reduced distances a free
column first, then the lowest column position); scipy's linear_sum_assignment, which the reference and the per-frame path call, leaves it unspecified.
The ground truth's `difficulty` travels as one byte per box (difficulty > 0) and reaches the host with the one flush.  Optimal
assignment on the centre distance is not built.

nuScenes collections (`Collection(..., kind="nusc")`, liso_amd/eval/nuscenes_metrics.py: mAP over centre-distance thresholds, the
true-positive errors, NDS) use neither the job tables nor the pair matrices: each costs one more launch per batch,
liso_det_val_nusc_f32 (include/liso_nusc_metrics.h), on the class-transferred predictions, and its outputs ride in the one flush.  A
collection with `sigmoid_scores=True` walks in the stable order of the fp32 sigmoid of the scores (one sigmoid and one
`det_nms.order` more per batch, shared by all such collections).
"""
import ctypes
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from liso_amd import _lib as L
from liso_amd.eval.nuscenes_metrics import NUSC_MOVABLE_CLASSES, NuscenesObjectDetectionMetrics, nusc_match_host, nusc_match_packed
from liso_amd.eval.nuscenes_metrics import OUT_KEYS as NUSC_OUT_KEYS
from liso_amd.eval.od_metrics import ObjectDetectionMetrics, WaymoObjectDetectionMetrics
from liso_amd.kabsch.shape_utils import Shape
from liso_amd.utils.device_args import opt_ptr as _p

MAX_BOXES = 1024  # LISO_DET_VAL_MAX_BOXES
CRITERIA = {"iou_bev": 0, "iou_3d": 1, "dist": 2}  # LISO_DET_VAL_*
CLASS_TRANSFER_THRESHOLD_M = 3.0  # run_val :408

FILTER_DTYPE = np.dtype([("area", np.float32, 4), ("range", np.float32, 2), ("use_area", np.int32), ("use_range", np.int32),
                         ("class_id", np.int32)])  # liso_det_val_filter
JOB_DTYPE = np.dtype([("filter", np.int32), ("criterion", np.int32), ("threshold", np.float32)])  # liso_det_val_job


class FilterSet(NamedTuple):
    """BEV-area bounds (min_x, min_y, max_x, max_y), inclusive; radial range (min, max), min <= r < max; class id (-1: any).
    None switches a part off."""
    area: Optional[Tuple[float, float, float, float]] = None
    range: Optional[Tuple[float, float]] = None
    class_id: int = -1


class Job(NamedTuple):
    filter: int
    criterion: str
    threshold: float


class JobTable:
    """The filter sets and jobs of a call: host tables, uploaded once per device."""

    def __init__(self, filters: Sequence[FilterSet] = (), jobs: Sequence[Job] = (), assignment: bool = False):
        self.assignment = bool(assignment)  # a table of optimal-assignment jobs (liso_det_val_assign_f32): IoU criteria only
        self.filters: List[FilterSet] = []
        self.jobs: List[Job] = []
        self._dev = {}
        for f in filters:
            self.add_filter(f)
        for j in jobs:
            self.add_job(*j)

    def add_filter(self, f: FilterSet) -> int:
        f = FilterSet(None if f.area is None else tuple(float(v) for v in f.area),
                      None if f.range is None else tuple(float(v) for v in f.range), int(f.class_id))
        if f not in self.filters:
            self.filters.append(f)
            self._dev = {}
        return self.filters.index(f)

    def add_job(self, filter_idx: int, criterion: str, threshold: float) -> int:
        if criterion not in CRITERIA:
            raise NotImplementedError(criterion)
        if self.assignment and criterion == "dist":
            raise NotImplementedError("optimal assignment on the centre distance is not built: IoU criteria only")
        if not 0 <= filter_idx < len(self.filters):
            raise L.LisoHipError(f"job names filter set {filter_idx}, the table has {len(self.filters)}")
        j = Job(int(filter_idx), criterion, float(np.float32(threshold)))
        if j not in self.jobs:
            self.jobs.append(j)
            self._dev = {}
        return self.jobs.index(j)

    @property
    def needs_classes(self) -> bool:
        return any(self.filters[j.filter].class_id >= 0 for j in self.jobs)

    @property
    def criteria_mask(self) -> int:
        m = 0
        for j in self.jobs:
            m |= 1 << CRITERIA[j.criterion]
        return m

    def host_tables(self):
        f = np.zeros(len(self.filters), FILTER_DTYPE)
        for i, s in enumerate(self.filters):
            f[i] = ((0, 0, 0, 0) if s.area is None else s.area, (0, 0) if s.range is None else s.range, s.area is not None,
                    s.range is not None, s.class_id)
        j = np.zeros(len(self.jobs), JOB_DTYPE)
        for i, b in enumerate(self.jobs):
            j[i] = (b.filter, CRITERIA[b.criterion], b.threshold)
        return f, j

    def device_tables(self, device):
        key = str(device)
        if key not in self._dev:
            f, j = self.host_tables()
            up = lambda a: torch.from_numpy(np.frombuffer(a.tobytes() or b"\0", np.uint8).copy()).to(device)  # noqa: E731
            self._dev[key] = (up(f), up(j))
        return self._dev[key]


assert FILTER_DTYPE.itemsize == 36 and JOB_DTYPE.itemsize == 12


# ---- packing: padded Shape batches -> the arrays the kernels and the host restatement read ------------------------------------
def _rows7(s: Shape):
    from liso_amd.utils.nms_iou import pad_attr_to_3d_if_necessary

    rot = s.rot if s.rot is not None else torch.zeros_like(s.pos[..., :1])
    dense = torch.cat([pad_attr_to_3d_if_necessary(s.pos, 0.0), pad_attr_to_3d_if_necessary(s.dims, 1.0), rot[..., :1]], dim=-1).float()
    return torch.where(s.valid[..., None], dense, torch.zeros_like(dense)).contiguous()  # what invalid slots hold never matters


def pack_boxes(boxes: Shape, moving_velocity_thresh: Optional[float] = None, with_hard: bool = False):
    """padded Shape [F,N] (torch, any device) -> dict(rows fp32 [F,N,7], valid uint8 [F,N], cls int32 [F,N], score fp32 [F,N],
    moving uint8 [F,N] (|velo| > moving_velocity_thresh; zeros without a threshold); with_hard: also hard uint8 [F,N], difficulty > 0,
    what the Waymo-style collections' L1 category leaves out)"""
    assert len(boxes.valid.shape) == 2, "a padded [F, N] batch"
    valid = boxes.valid.bool()
    out = {"rows": _rows7(boxes), "valid": valid.contiguous().view(torch.uint8),
           "cls": torch.where(valid, boxes.class_id[..., 0].to(torch.int32), -1).contiguous(),
           "score": boxes.probs[..., 0].float().contiguous()}
    if moving_velocity_thresh is None:
        out["moving"] = torch.zeros_like(out["valid"])
    else:
        moving = (torch.linalg.norm(boxes.velo, dim=-1) > moving_velocity_thresh) & valid
        out["moving"] = moving.contiguous().view(torch.uint8)
    if with_hard:
        out["hard"] = ((boxes.difficulty[..., 0] > 0) & valid).contiguous().view(torch.uint8)
    return out


def _check_packed(gt, pred):
    F, G = gt["valid"].shape
    F2, P = pred["valid"].shape
    if F != F2:
        raise L.LisoHipError(f"ground truth has {F} frames, predictions {F2}")
    if G > MAX_BOXES or P > MAX_BOXES:
        raise L.LisoHipError(f"at most {MAX_BOXES} boxes per frame, got G={G}, P={P}")
    return F, G, P


# ---- device path ----------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def match_detections_packed(gt, pred, table: JobTable, class_draws=None, order=None,
                            transfer_threshold: float = CLASS_TRANSFER_THRESHOLD_M, pred_class=None, assign: Optional[JobTable] = None):
    """`match_detections` on packed arrays (`pack_boxes`), all on one device."""
    _check_assign_table(assign)
    F, G, P = _check_packed(gt, pred)
    L.require_cuda(gt["rows"], gt["valid"], gt["cls"], pred["rows"], pred["valid"], pred["cls"], pred["score"])
    dev = gt["rows"].device
    if pred["rows"].device != dev:
        raise L.LisoHipError(f"ground truth on {dev}, predictions on {pred['rows'].device}")
    if class_draws is not None:
        L.require_cuda(class_draws)
        if tuple(class_draws.shape) != (F, P):
            raise L.LisoHipError(f"class_draws must have shape {(F, P)}, got {tuple(class_draws.shape)}")
        class_draws = class_draws.to(torch.int32).contiguous()
    if order is None:
        from liso_amd import det_nms as D

        if F > 0 and P > 0:
            _, order = D.order(pred["score"], None, pred["valid"], None)
        else:
            order = torch.zeros((F, P), dtype=torch.int32, device=dev)
    J, S, M = len(table.jobs), len(table.filters), min(G, P)
    lib = L.lib()
    new = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)  # noqa: E731
    mask = table.criteria_mask | (assign.criteria_mask if assign is not None else 0) | (4 if class_draws is not None else 0)
    mats = {k: (new((F, P, G), torch.float32) if (mask >> c) & 1 else None) for k, c in CRITERIA.items()}
    out = {"order": order, **{k: v for k, v in mats.items() if v is not None}}
    with torch.cuda.device(dev):
        if mask:
            L.check(lib.liso_det_val_pairs_f32(F, G, P, _p(gt["rows"]), _p(gt["valid"]), _p(pred["rows"]), _p(pred["valid"]),
                                               _p(mats["iou_bev"]), _p(mats["iou_3d"]), _p(mats["dist"]), L.stream_ptr()), "det_val pairs")
        if pred_class is None:
            pred_class = pred["cls"]
        if class_draws is not None:
            pred_class = new((F, P), torch.int32)
            L.check(lib.liso_det_val_transfer_classes(F, G, P, _p(gt["valid"]), _p(gt["cls"]), _p(pred["valid"]), _p(order),
                                                      _p(mats["dist"]), float(transfer_threshold), _p(class_draws), _p(pred_class),
                                                      L.stream_ptr()), "det_val class transfer")
        out["pred_class"] = pred_class
        out["count"], out["pairs"], out["sums"] = new((F, J), torch.int32), new((F, J, M, 2), torch.int16), new((F, J, 3), torch.float64)
        out["gt_in"], out["pred_in"] = new((F, S, G), torch.uint8), new((F, S, P), torch.uint8)
        if J:
            ft, jt = table.device_tables(dev)
            L.check(lib.liso_det_val_match_f32(F, G, P, _p(gt["rows"]), _p(gt["valid"]), _p(gt["cls"]), _p(pred["rows"]), _p(pred["valid"]),
                                               _p(pred_class), _p(order), _p(mats["iou_bev"]), _p(mats["iou_3d"]), _p(mats["dist"]),
                                               table.criteria_mask, L.ptr(ft), S, L.ptr(jt), J, _p(out["count"]), _p(out["pairs"]),
                                               _p(out["sums"]), _p(out["gt_in"]), _p(out["pred_in"]), L.stream_ptr()), "det_val match")
        if assign is not None:
            JA, SA = len(assign.jobs), len(assign.filters)
            out["assign_count"], out["assign_pairs"] = new((F, JA), torch.int32), new((F, JA, M, 2), torch.int16)
            out["assign_gt_in"], out["assign_pred_in"] = new((F, SA, G), torch.uint8), new((F, SA, P), torch.uint8)
            if JA:
                ft, jt = assign.device_tables(dev)
                L.check(lib.liso_det_val_assign_f32(F, G, P, _p(gt["rows"]), _p(gt["valid"]), _p(gt["cls"]), _p(pred["rows"]), _p(pred["valid"]),
                                                    _p(pred_class), _p(mats["iou_bev"]), _p(mats["iou_3d"]), assign.criteria_mask, L.ptr(ft), SA,
                                                    L.ptr(jt), JA, _p(out["assign_count"]), _p(out["assign_pairs"]), _p(out["assign_gt_in"]),
                                                    _p(out["assign_pred_in"]), L.stream_ptr()), "det_val assign")
    return out


def _check_assign_table(assign):
    if assign is not None and (not assign.assignment or any(j.criterion == "dist" for j in assign.jobs)):
        raise NotImplementedError("an assignment table is a JobTable(assignment=True): IoU criteria only, `dist` is not built")


@torch.no_grad()
def match_detections(gt: Shape, pred: Shape, table: JobTable, class_draws=None, order=None,
                     transfer_threshold: float = CLASS_TRANSFER_THRESHOLD_M, assign: Optional[JobTable] = None):
    """All frames of a padded batch against all jobs of `table`, on the device, with no host sync (graph-capturable).

    gt Shape [F,G], pred Shape [F,P] (cuda; holes in `valid` allowed; G, P <= 1024).  `class_draws` int [F,P] (cuda): run_val's
    class transfer (:406-447) runs first -- every valid prediction's class becomes its draw, a prediction matched by centre
    distance below `transfer_threshold` takes its ground-truth box's class -- and the class-filtered jobs read the result;
    None: the predictions' own class ids.  `order` int32 [F,P]: the visiting order (default `liso_amd.det_nms.order` on the
    probs: stable, most confident first).
    -> dict of device tensors: count int32 [F,J]; pairs int16 [F,J,min(G,P),2] (gt slot, pred slot) in match order, -1 padded;
    sums fp64 [F,J,3] (ATE, ASE, AOE); gt_in uint8 [F,S,G], pred_in uint8 [F,S,P]; pred_class int32 [F,P]; order; and the pair
    matrices the jobs needed, fp32 [F,P,G]: iou_bev, iou_3d, dist.
    `assign`: a `JobTable(assignment=True)` of optimal-assignment jobs (IoU criteria; one more launch, liso_det_val_assign_f32, after
    the class transfer) -> also assign_count int32 [F,JA], assign_pairs int16 [F,JA,min(G,P),2] in ascending ground-truth slot, -1
    padded, assign_gt_in uint8 [F,SA,G], assign_pred_in uint8 [F,SA,P] (the membership in THAT table's filter sets)."""
    L.require_cuda(gt.valid, pred.valid)
    return match_detections_packed(pack_boxes(gt), pack_boxes(pred), table, class_draws, order, transfer_threshold, assign=assign)


# ---- numpy restatement ------------------------------------------------------------------------------------------------------------
def host_pair_matrices(gt_rows, gt_valid, pred_rows, pred_valid):
    """the library's host twin of the pair kernel (liso_det_val_pairs_cpu_f32) -> dict(iou_bev, iou_3d, dist) fp32 [F,P,G]"""
    gt_rows, pred_rows = np.ascontiguousarray(gt_rows, np.float32), np.ascontiguousarray(pred_rows, np.float32)
    gv, pv = np.ascontiguousarray(gt_valid, np.uint8), np.ascontiguousarray(pred_valid, np.uint8)
    F, G, P = gt_rows.shape[0], gt_rows.shape[1], pred_rows.shape[1]
    mats = {k: np.zeros((F, P, G), np.float32) for k in CRITERIA}
    hp = lambda a: ctypes.c_void_p(a.ctypes.data) if a.size else None  # noqa: E731
    L.check(L.lib().liso_det_val_pairs_cpu_f32(F, G, P, hp(gt_rows), hp(gv), hp(pred_rows), hp(pv), hp(mats["iou_bev"]), hp(mats["iou_3d"]),
                                               hp(mats["dist"])), "det_val pairs (host)")
    return mats


def stable_order_host(score, valid):
    """`liso_amd.det_nms.order` on the host: valid slots by descending score (NaN first), equal scores in ascending slot index, the
    invalid slots after them.  -> int32 [F,P]"""
    score, valid = np.asarray(score, np.float32), np.asarray(valid).astype(bool)
    key = np.where(np.isnan(score), -np.inf, -score.astype(np.float64))
    key = np.where(valid, key, np.inf)
    return np.argsort(key, axis=-1, kind="stable").astype(np.int32)


def _in_set_host(rows, valid, cls, f: FilterSet):
    x, y = rows[:, 0], rows[:, 1]
    ok = np.asarray(valid).astype(bool).copy()
    with np.errstate(invalid="ignore"):
        if f.area is not None:
            a = np.float32(f.area)
            ok &= (a[0] <= x) & (x <= a[2]) & (a[1] <= y) & (y <= a[3])
        if f.range is not None:
            r = np.sqrt(x * x + y * y)
            ok &= (np.float32(f.range[0]) <= r) & (r < np.float32(f.range[1]))
    if f.class_id >= 0:
        ok &= cls == f.class_id
    return ok


def _walk_host(val, smaller_wins, thr, order, g_in, p_in):
    """the greedy walk on one frame's [P,G] matrix -> list of (gt slot, pred slot)"""
    thr = np.float32(thr)
    free = g_in.copy()
    P, out = val.shape[0], []
    for p in order:
        if p < 0 or p >= P or not p_in[p]:
            continue
        best, bg = None, -1
        for g in np.flatnonzero(free):
            v = val[p, g]
            if (v < thr) if smaller_wins else (v > thr):
                if best is None or ((v < best) if smaller_wins else (v > best)):
                    best, bg = v, g
        if bg >= 0:
            free[bg] = False
            out.append((bg, int(p)))
    return out


def assign_host(val, g_in, p_in, thr):
    """The optimal assignment of one cell (include/liso_det_val.h, "(4) Assign"), stated in numpy: val fp32 [P,G] pred-major, g_in /
    p_in the membership of the slots, thr the fp32 threshold -> list of kept (gt slot, pred slot) in ascending ground-truth slot.

    c(g,p) = val[p,g] if finite else -1; every member of the smaller set gets a distinct member of the larger one so that the sum of
    c is largest; pairs with c >= thr (fp32) are kept.  Rows: the smaller set in ascending slot order (the ground truth on equal
    sizes); columns: the other set in ascending slot order.  Rows are inserted one by one by a shortest augmenting path on the cost
    -c with fp64 potentials u (rows), v (columns), all 0 at the start: a search keeps the running minimum `minv` of the reduced
    distance of every unvisited column, takes the column of the smallest one -- among equal ones a FREE (unassigned) column before
    an assigned one, then the LOWEST COLUMN POSITION --, and shifts u and v of the visited rows / columns and minv of the others by
    it, until the column taken is free.  (Preferring free columns ends a search among equal distances at once; with the many equal
    values of a sparse IoU matrix, its zeros, it would otherwise wander through the assigned ones.)  The kernel performs these
    additions, subtractions and comparisons in the same order: the pairs are equal bit for bit."""
    val = np.asarray(val, np.float32)
    gs, ps = np.flatnonzero(g_in), np.flatnonzero(p_in)
    if gs.size == 0 or ps.size == 0:
        return []
    c = val[np.ix_(ps, gs)].T  # [n_g, n_p]
    c = np.where(np.isfinite(c), c, np.float32(-1.0))
    gt_rows = gs.size <= ps.size
    if not gt_rows:
        c = c.T
    cost = -c.astype(np.float64)  # [rows, columns]
    n, m = cost.shape
    u, v = np.zeros(n), np.zeros(m)
    owner = np.full(m, -1, np.int64)  # the row assigned to a column
    for i in range(n):
        minv, way, used = np.full(m, np.inf), np.full(m, -1, np.int64), np.zeros(m, bool)
        j0 = -1  # the search's start: a virtual column owned by row i
        while True:
            i0 = i if j0 < 0 else owner[j0]
            cur = (cost[i0] - u[i0]) - v
            better = ~used & (cur < minv)
            minv[better], way[better] = cur[better], j0
            cand = np.where(used, np.inf, minv)
            delta = cand.min()
            ties = cand == delta
            free_ties = ties & (owner < 0)
            j1 = int(np.argmax(free_ties if free_ties.any() else ties))  # a free column first, then the lowest position
            u[owner[used]] += delta
            v[used] -= delta
            minv[~used] -= delta
            u[i] += delta
            j0 = j1
            used[j0] = True
            if owner[j0] < 0:
                break
        while j0 >= 0:  # flip the path back to the start
            j1 = way[j0]
            owner[j0] = i if j1 < 0 else owner[j1]
            j0 = j1
    cols = np.flatnonzero(owner >= 0)
    rows = owner[cols]
    keep = c[rows, cols] >= np.float32(thr)
    rows, cols = rows[keep], cols[keep]
    pairs = list(zip(gs[rows].tolist(), ps[cols].tolist())) if gt_rows else list(zip(gs[cols].tolist(), ps[rows].tolist()))
    return sorted(pairs)


def _nan_min(a, b):
    return np.minimum(a, b)  # NaN if either is NaN


def tp_terms_host(g, p):
    """the ATE / ASE / AOE terms of matched rows g, p fp32 [m,7], evaluated in fp32 operation by operation (include/liso_det_val.h)"""
    f32 = np.float32
    with np.errstate(invalid="ignore", divide="ignore"):
        dx, dy = g[:, 0] - p[:, 0], g[:, 1] - p[:, 1]
        ate = np.sqrt(dx * dx + dy * dy)
        inter = _nan_min(g[:, 3], p[:, 3]) * _nan_min(g[:, 4], p[:, 4]) * _nan_min(g[:, 5], p[:, 5])
        uni = g[:, 3] * g[:, 4] * g[:, 5] + p[:, 3] * p[:, 4] * p[:, 5] - inter
        den = np.where(uni < f32(1e-6), f32(1e-6), uni)
        ase = f32(1.0) - inter / den
        pi, two_pi = f32(np.pi), f32(2.0 * np.pi)
        r = np.fmod(g[:, 6] - p[:, 6] + pi, two_pi)
        r = np.where(r != 0, np.where(r < 0, r + two_pi, r), f32(0.0))
        d = r - pi
        d = np.where(d > pi, d - two_pi, d)
        aoe = np.abs(d)
    return ate.astype(f32), ase.astype(f32), aoe.astype(f32)


def match_detections_host(gt, pred, table: JobTable, class_draws=None, order=None, pairs=None,
                          transfer_threshold: float = CLASS_TRANSFER_THRESHOLD_M, pred_class=None, assign: Optional[JobTable] = None):
    """numpy restatement of `match_detections_packed`.  gt / pred: dicts of numpy arrays as `pack_boxes` lays them out (rows, valid,
    cls, score); `pairs`: dict(iou_bev, iou_3d, dist) of [F,P,G] matrices, default `host_pair_matrices`.  -> the same dictionary, numpy."""
    _check_assign_table(assign)
    gt = {k: np.asarray(v) for k, v in gt.items()}
    pred = {k: np.asarray(v) for k, v in pred.items()}
    F, G, P = _check_packed(gt, pred)
    if order is None:
        order = stable_order_host(pred["score"], pred["valid"])
    order = np.asarray(order)
    if pairs is None:
        pairs = host_pair_matrices(gt["rows"], gt["valid"], pred["rows"], pred["valid"])
    J, S, M = len(table.jobs), len(table.filters), min(G, P)
    gv, pv = gt["valid"].astype(bool), pred["valid"].astype(bool)
    if pred_class is None:
        pred_class = pred["cls"].astype(np.int32)
    if class_draws is not None:
        pred_class = np.where(pv, np.asarray(class_draws).astype(np.int32), np.int32(-1))
        for f in range(F):
            if G and P:
                for g, p in _walk_host(pairs["dist"][f], True, transfer_threshold, order[f], gv[f], pv[f]):
                    pred_class[f, p] = gt["cls"][f, g]
    out = {"order": order, "pred_class": pred_class, "count": np.zeros((F, J), np.int32), "pairs": np.full((F, J, M, 2), -1, np.int16),
           "sums": np.zeros((F, J, 3), np.float64), "gt_in": np.zeros((F, S, G), np.uint8), "pred_in": np.zeros((F, S, P), np.uint8)}
    for f in range(F):
        for j, job in enumerate(table.jobs):
            fs = table.filters[job.filter]
            g_in = _in_set_host(gt["rows"][f], gv[f], gt["cls"][f], fs)
            p_in = _in_set_host(pred["rows"][f], pv[f], pred_class[f], fs)
            out["gt_in"][f, job.filter], out["pred_in"][f, job.filter] = g_in, p_in
            if not (G and P):
                continue
            m = _walk_host(pairs[job.criterion][f], job.criterion == "dist", job.threshold, order[f], g_in, p_in)
            out["count"][f, j] = len(m)
            if m:
                mm = np.array(m, np.int64)
                out["pairs"][f, j, :len(m)] = mm
                terms = tp_terms_host(gt["rows"][f][mm[:, 0]], pred["rows"][f][mm[:, 1]])
                out["sums"][f, j] = [np.cumsum(t, dtype=np.float64)[-1] for t in terms]  # in match order, as the kernel adds them
    if assign is not None:
        JA, SA = len(assign.jobs), len(assign.filters)
        out.update(assign_count=np.zeros((F, JA), np.int32), assign_pairs=np.full((F, JA, M, 2), -1, np.int16),
                   assign_gt_in=np.zeros((F, SA, G), np.uint8), assign_pred_in=np.zeros((F, SA, P), np.uint8))
        for f in range(F):
            for j, job in enumerate(assign.jobs):
                fs = assign.filters[job.filter]
                g_in = _in_set_host(gt["rows"][f], gv[f], gt["cls"][f], fs)
                p_in = _in_set_host(pred["rows"][f], pv[f], pred_class[f], fs)
                out["assign_gt_in"][f, job.filter], out["assign_pred_in"][f, job.filter] = g_in, p_in
                if not (G and P):
                    continue
                m = assign_host(pairs[job.criterion][f], g_in, p_in, job.threshold)
                out["assign_count"][f, j] = len(m)
                if m:
                    out["assign_pairs"][f, j, :len(m)] = np.array(m, np.int64)
    return out


# ---- the metric collections of a validation pass -------------------------------------------------------------------------------
class Collection(NamedTuple):
    """One `ObjectDetectionMetrics`: its tag under `<prefix>` (compute() appends `/<criterion>/...`), the ground-truth set it reads
    ("gt": the visible boxes, "benchmark": the benchmark's), and the constructor arguments.  kind "waymo": one
    `WaymoObjectDetectionMetrics` (optimal assignment, L1 / L2); its compute() appends `<criterion>/...` to the tag with no
    separator, as the reference's log() does.  kind "nusc": one `NuscenesObjectDetectionMetrics`; its compute() appends `/mAP`, `/NDS`,
    `/<class>/AP`, ... to the tag stripped of trailing slashes."""
    tag: str
    gt_set: str
    kwargs: dict
    kind: str = "od"


RANGE_BINS = ((0.0, 1000.0), (0.0, 20.0), (20.0, 40.0), (40.0, 60.0))  # run_val :162
KINDS = {"od": ObjectDetectionMetrics, "waymo": WaymoObjectDetectionMetrics, "nusc": NuscenesObjectDetectionMetrics}


class DetectionValidator:
    """The metric collections of a detector validation pass, matched on the device.

    `collections`: `Collection`s.  `transfer_classes`: run run_val's class transfer before the class-filtered jobs, with draws
    the caller passes to `update_batch`, or drawn on the device from `generator` -- `torch.multinomial` on `class_frequencies`
    when given, else `torch.randint(0, n_classes)`."""

    def __init__(self, collections: Sequence[Collection], transfer_classes: bool = False, n_classes: int = 1, class_frequencies=None,
                 generator=None):
        self.collections = [c if isinstance(c, Collection) else Collection(*c) for c in collections]
        for c in self.collections:
            if c.kind not in KINDS:
                raise ValueError(f"kind must be one of {sorted(KINDS)}, got {c.kind!r}")
        self.metrics = [KINDS[c.kind](**c.kwargs) for c in self.collections]
        self.transfer_classes, self.n_classes, self.class_frequencies, self.generator = transfer_classes, int(n_classes), class_frequencies, generator
        self.tables = {"gt": JobTable(), "benchmark": JobTable()}
        self.assign_tables = {"gt": JobTable(assignment=True), "benchmark": JobTable(assignment=True)}  # the Waymo-style collections' jobs
        self.job_of = []  # per collection: {(class_name, thr): job index in its table}; Waymo-style: {(class_name, criterion): ...}
        thresholds = set()
        for c, m in zip(self.collections, self.metrics):
            if c.gt_set not in self.tables:
                raise ValueError(f"gt_set must be 'gt' or 'benchmark', got {c.gt_set!r}")
            if c.kind == "nusc":  # no jobs: a launch of its own per batch
                self.job_of.append({})
                continue
            if c.kind == "waymo":
                t, jobs = self.assign_tables[c.gt_set], {}
                area = tuple(m.bev_range_min_xy_m.tolist() + m.bev_range_max_xy_m.tolist())
                rng = None if (m.max_eval_range_m is None or m.min_eval_range_m is None) else (m.min_eval_range_m, m.max_eval_range_m)
                for class_idx, class_name in zip(m.class_idxs, m.class_names):
                    fi = t.add_filter(FilterSet(area, rng, -1 if class_name == "overall" else int(class_idx)))
                    for crit in m.CRITERIA:
                        jobs[(class_name, crit)] = t.add_job(fi, crit, m.iou_matching_threshold)
                self.job_of.append(jobs)
                continue
            if m.box_matching_criterion == "dist" and not m.use_slow_nuscenes_matching:
                raise NotImplementedError("optimal assignment on the centre distance is not built on the device (host: scipy, as in the reference)")
            thresholds.add(float(m.moving_velocity_thresh))
            t, jobs = self.tables[c.gt_set], {}
            area = None if m.bev_range_min_xy_m is None else tuple(m.bev_range_min_xy_m.tolist() + m.bev_range_max_xy_m.tolist())
            rng = None if (m.max_eval_range_m is None or m.min_eval_range_m is None) else (m.min_eval_range_m, m.max_eval_range_m)
            for class_idx, class_name in zip(m.class_idxs, m.class_names):
                fi = t.add_filter(FilterSet(area, rng, -1 if class_name == "overall" else int(class_idx)))
                for thr in m.matching_thresholds:
                    jobs[(class_name, thr)] = t.add_job(fi, m.box_matching_criterion, thr)
            self.job_of.append(jobs)
        if len(thresholds) > 1:
            raise NotImplementedError("one moving_velocity_thresh per validator")
        self.moving_velocity_thresh = thresholds.pop() if thresholds else 0.0
        self._pending, self._host = [], []

    # -- run_val :162-248 ------------------------------------------------------------------------------------------------------
    @classmethod
    def for_run_val(cls, dataset_kind: str, movable_class_names: Sequence[str] = (), class_idxs: Sequence[int] = (),
                    moving_velocity_thresh: float = 0.1, class_frequencies=None, generator=None, waymo_metrics: bool = False,
                    nuscenes_metrics: bool = False, sigmoid_scores: bool = False):
        """visible / benchmark / waymo_cropped x 4 range bins x {iou_3d, iou_bev}, and the per-class collection of a KITTI
        ("kitti") or AV2 ("av2") validation set, with the per-dataset `min_precision`.

        nuscenes_metrics=True adds the reference's `nusc_metrics` (:209, 493-514, 729-734), which it feeds on EVERY data set: one
        `NuscenesObjectDetectionMetrics(eval_movable_classes_as_one=True)` on the visible ground truth under
        `final_result/NUSC_OFFICIAL/detection_metrics/` (mAP, mATE ... mAAE, NDS, movable/AP ...).  It also makes "nuscenes" buildable:
        the 24 range collections with `min_precision=0.1`, plus the per-class `NuscenesObjectDetectionMetrics` (:210-214) under
        `final_result/NUSC_OFFICIAL/per_class/detection_metrics/`, classes looked up by class id: `movable_class_names` at
        `class_idxs` (default: the reference's nuScenes order).  `sigmoid_scores`: both read the fp32 sigmoid of the scores
        (:494-509; `run_val` decides).  With the default every existing collection, tag and value is unchanged.

        waymo_metrics=True adds the reference's `waymo_metrics` (:249-255, 487-492, 741-747): one `WaymoObjectDetectionMetrics` per
        range bin on the BENCHMARK ground truth, matched by optimal assignment on the device.  Their tags are
        `final_result/WAYMO/detection_metrics/<lo>_<hi>m` followed DIRECTLY by the criterion: the reference writes no separator there
        (:746 with :1798), and neither does this.  It also makes "waymo" buildable: the 24 range collections with
        `min_precision=0.1` as for KITTI, plus the per-class `WaymoObjectDetectionMetrics` on the visible ground truth under
        `final_result/WAYMO/per_class/detection_metrics/`.  That collection takes the predictions' scores as the other per-class
        collections do: the reference's sigmoid on them (:494-509) is monotone, changes no order and no matching, and stays out."""
        if (dataset_kind not in ("kitti", "av2") and not (dataset_kind == "waymo" and waymo_metrics)
                and not (dataset_kind == "nuscenes" and nuscenes_metrics)):
            raise NotImplementedError(f"{dataset_kind}: only the KITTI and AV2 collection sets are built, Waymo's with waymo_metrics=True "
                                      "and nuScenes' with nuscenes_metrics=True")
        cols = []
        for cat in ("visible", "benchmark", "waymo_cropped"):
            for lo, hi in RANGE_BINS:
                for crit in ("iou_3d", "iou_bev"):
                    kw = dict(moving_velocity_thresh=moving_velocity_thresh, use_slow_nuscenes_matching=True, min_recall=0.0,
                              box_matching_criterion=crit, min_eval_range_m=lo, max_eval_range_m=hi)
                    if cat == "waymo_cropped":
                        kw.update(min_precision=0.0, iou_matching_thresholds=(0.3, 0.4, 0.5, 0.7),
                                  filter_detections_by_bev_area_min_max_m=[-50.0, -20.0, 50.0, 20.0])
                    else:
                        kw.update(min_precision=0.0 if dataset_kind == "av2" else 0.1)
                    cols.append(Collection(f"final_result/{cat}/detection_metrics/{int(lo)}_{int(hi)}m", "benchmark" if cat == "benchmark" else "gt", kw))
        if dataset_kind == "kitti":
            cols.append(Collection("final_result/KITTI/per_class/detection_metrics/", "gt", dict(
                moving_velocity_thresh=moving_velocity_thresh, use_slow_nuscenes_matching=True, class_names=tuple(movable_class_names),
                class_idxs=tuple(class_idxs), min_recall=0.0, box_matching_criterion="iou_bev", eval_movable_classes_as_one=False)))
        elif dataset_kind == "waymo":
            cols.append(Collection("final_result/WAYMO/per_class/detection_metrics/", "gt", dict(
                eval_movable_classes_as_one=False, class_names=tuple(movable_class_names), class_idxs=tuple(class_idxs)), "waymo"))
        elif dataset_kind == "nuscenes":
            names = tuple(movable_class_names) or NUSC_MOVABLE_CLASSES
            idxs = tuple(class_idxs) or tuple(range(len(names)))
            if sorted(idxs) != list(range(len(names))):
                raise ValueError(f"the nuScenes per-class radii are looked up by class id: class_idxs must number the names 0..{len(names) - 1}, got {idxs}")
            by_id = tuple(n for _, n in sorted(zip(idxs, names)))
            cols.append(Collection("final_result/NUSC_OFFICIAL/per_class/detection_metrics/", "gt", dict(
                eval_movable_classes_as_one=False, class_names=by_id, sigmoid_scores=sigmoid_scores), "nusc"))
        else:
            cols.append(Collection("final_result/AV2/per_class/detection_metrics/", "gt", dict(
                moving_velocity_thresh=moving_velocity_thresh, use_slow_nuscenes_matching=True, min_recall=0.0, min_precision=0.0,
                box_matching_criterion="iou_bev", eval_movable_classes_as_one=False)))
        if waymo_metrics:
            for lo, hi in RANGE_BINS:
                cols.append(Collection(f"final_result/WAYMO/detection_metrics/{int(lo)}_{int(hi)}m", "benchmark",
                                       dict(min_eval_range_m=lo, max_eval_range_m=hi), "waymo"))
        if nuscenes_metrics:
            cols.append(Collection("final_result/NUSC_OFFICIAL/detection_metrics/", "gt",
                                   dict(eval_movable_classes_as_one=True, sigmoid_scores=sigmoid_scores), "nusc"))
        n_classes = len(movable_class_names) or (len(NUSC_MOVABLE_CLASSES) if dataset_kind == "nuscenes" else 1)
        return cls(cols, transfer_classes=True, n_classes=n_classes, class_frequencies=class_frequencies, generator=generator)

    # -- accumulation -----------------------------------------------------------------------------------------------------------
    def _draws(self, F, P, device):
        if self.class_frequencies is not None:
            w = torch.as_tensor(self.class_frequencies, dtype=torch.float32, device=device)
            return torch.multinomial(w.expand(max(F, 1), -1), max(P, 1), replacement=True, generator=self.generator)[:F, :P].to(torch.int32)
        return torch.randint(0, self.n_classes, (F, P), device=device, generator=self.generator, dtype=torch.int32)

    @torch.no_grad()
    def update_batch(self, gt: Shape, benchmark_gt: Optional[Shape], pred: Shape, counts=None, class_draws=None):
        """One padded batch: gt / benchmark_gt Shape [F,G*], pred Shape [F,P] on the device (`predict_boxes`' first result;
        `counts` int32 [F], its third: when given only the first counts[f] slots of frame f take part).  Appends device outputs;
        builds nothing on the host and performs no host sync."""
        L.require_cuda(pred.valid)
        run = lambda name, *args, **kw: match_detections_packed(*args, **kw)  # noqa: E731

        def run_nusc(g, p, order, m, pred_class):
            return nusc_match_packed(g, p, order, m.radius_on(p["rows"].device), m.eval_movable_classes_as_one, m.matching_thresholds, pred_class)

        def order_of(score, valid):
            from liso_amd import det_nms as D

            return D.order(score.contiguous(), None, valid, None)[1] if score.numel() else torch.zeros(score.shape, dtype=torch.int32, device=score.device)
        self._pending.append(self._match_batch(gt, benchmark_gt, pred, counts, class_draws, run, lambda t: t, run_nusc, order_of))

    @torch.no_grad()
    def update_batch_host(self, gt: Shape, benchmark_gt: Optional[Shape], pred: Shape, counts=None, class_draws=None, pairs=None):
        """`update_batch` through the numpy restatement (host tensors; `pairs`: {"gt" / "benchmark": dict of pair matrices}, default
        the library's host twin): the same book-keeping fed by `match_detections_host`."""
        to_np = lambda t: t.cpu().numpy() if torch.is_tensor(t) else t  # noqa: E731

        def run(name, g, p, t, draws, order, pred_class=None, assign=None):
            g, p = ({k: to_np(v) for k, v in d.items()} for d in (g, p))
            return match_detections_host(g, p, t, to_np(draws), order, None if pairs is None else pairs.get(name), pred_class=pred_class,
                                         assign=assign)

        def run_nusc(g, p, order, m, pred_class):
            g, p = ({k: to_np(v) for k, v in d.items()} for d in (g, p))
            return nusc_match_host(g["rows"], g["valid"], g["cls"], p["rows"], p["valid"], to_np(pred_class), to_np(order), m.radius,
                                   m.eval_movable_classes_as_one, m.matching_thresholds)
        rec = self._match_batch(gt, benchmark_gt, pred, counts, class_draws, run, to_np, run_nusc,
                                lambda score, valid: stable_order_host(to_np(score), to_np(valid)))
        self._host.append(rec)

    def _match_batch(self, gt, benchmark_gt, pred, counts, class_draws, run, keep, run_nusc, order_of):
        p = pack_boxes(pred)
        F, P = p["valid"].shape
        dev = p["valid"].device
        if counts is not None:
            live = torch.arange(P, device=dev)[None, :] < counts.to(dev)[:, None]
            p["valid"] = (p["valid"].view(torch.bool) & live).view(torch.uint8)
        draws = None
        nusc = [(i, m) for i, (c, m) in enumerate(zip(self.collections, self.metrics)) if c.kind == "nusc"]
        if self.transfer_classes and (any(t.needs_classes for t in list(self.tables.values()) + list(self.assign_tables.values()))
                                      or any(not m.eval_movable_classes_as_one for _, m in nusc)):
            draws = class_draws if class_draws is not None else self._draws(F, P, dev)
        order = pred_class = None
        rec = {}
        seen = {}  # sigmoid_scores -> (the scores a nuScenes collection reads, their stable order)
        for name, boxes in (("gt", gt), ("benchmark", benchmark_gt)):
            t, at = self.tables[name], self.assign_tables[name]
            at = at if at.jobs else None
            nusc_here = [(i, m) for i, m in nusc if self.collections[i].gt_set == name]
            if not t.jobs and at is None and not nusc_here:
                continue
            if boxes is None:
                raise ValueError(f"collections read the {name!r} ground truth, none was given")
            g = pack_boxes(boxes, self.moving_velocity_thresh, with_hard=at is not None)
            kw = {} if at is None else {"assign": at}
            o = run(name, g, p, t, draws if name == "gt" else None, order, pred_class=pred_class, **kw)
            order = o["order"]
            if name == "gt" and draws is not None:
                pred_class = o["pred_class"]  # the benchmark's class-filtered jobs read the same transferred classes
            rec[name] = {k: o[k] for k in ("sums", "count", "pairs", "gt_in", "pred_in")}
            rec[name]["moving"] = keep(g["moving"])
            if at is not None:
                rec[name].update({k: o[k] for k in ("assign_count", "assign_pairs", "assign_gt_in", "assign_pred_in")})
                rec[name]["hard"] = keep(g["hard"])
            if nusc_here:
                rec[name]["cls"], rec[name]["pred_class"] = keep(g["cls"]), o["pred_class"]
            for i, m in nusc_here:
                if m.sigmoid_scores not in seen:
                    sc = m.scores_seen(p["score"])
                    seen[m.sigmoid_scores] = (sc, order_of(sc, p["valid"]) if m.sigmoid_scores else order)
                    rec.setdefault("nusc_score", {})[str(int(m.sigmoid_scores))] = keep(sc)
                n = run_nusc(g, p, seen[m.sigmoid_scores][1], m, o["pred_class"])
                rec[name].update({f"nusc{i}_{k}": v for k, v in n.items()})
        rec["score"] = keep(p["score"])
        return rec

    def flush(self):
        """moves what is pending to the host in ONE read: every pending tensor's bytes are concatenated on the device (widest
        element type first, so every segment stays aligned) and copied once"""
        if not self._pending:
            return
        flat = []
        for rec in self._pending:
            for k, v in rec.items():
                flat += [(rec, k, None, v)] if torch.is_tensor(v) else [(rec, k, kk, vv) for kk, vv in v.items()]
        flat.sort(key=lambda e: -e[3].element_size())
        blob = torch.cat([e[3].contiguous().view(-1).view(torch.uint8) for e in flat]).cpu().numpy()
        host, off = {}, 0
        for rec, k, kk, v in flat:
            n = v.numel() * v.element_size()
            arr = blob[off:off + n].view(getattr(np, str(v.dtype).split(".")[1])).reshape(tuple(v.shape))
            off += n
            h = host.setdefault(id(rec), {})
            if kk is None:
                h[k] = arr
            else:
                h.setdefault(k, {})[kk] = arr
        self._host += [host[id(rec)] for rec in self._pending]
        self._pending = []

    def _feed(self, rec):
        score = rec["score"]
        for i, (c, m, jobs) in enumerate(zip(self.collections, self.metrics, self.job_of)):
            if c.kind == "nusc":  # one call per batch: vectorised over the frames
                r = rec[c.gt_set]
                m.accumulate_matches(rec["nusc_score"][str(int(m.sigmoid_scores))], r["pred_class"], r["cls"],
                                     **{k: r[f"nusc{i}_{k}"] for k in NUSC_OUT_KEYS})
                continue
            if c.kind == "waymo":
                self._feed_waymo(rec[c.gt_set], self.assign_tables[c.gt_set], m, jobs, score)
                continue
            r, t = rec[c.gt_set], self.tables[c.gt_set]
            for f in range(score.shape[0]):
                for (class_name, thr), j in jobs.items():
                    fi = t.jobs[j].filter
                    g_in, p_in = r["gt_in"][f, fi].astype(bool), r["pred_in"][f, fi].astype(bool)
                    n = int(r["count"][f, j])
                    pr = r["pairs"][f, j, :n].astype(np.int64)
                    # slots -> the compacted indices of the filtered box lists the book-keeping expects
                    idx_gt, idx_pred = (np.cumsum(g_in) - 1)[pr[:, 0]], (np.cumsum(p_in) - 1)[pr[:, 1]]
                    gt_mask, pred_mask = np.zeros(int(g_in.sum()), bool), np.zeros(int(p_in.sum()), bool)
                    gt_mask[idx_gt], pred_mask[idx_pred] = True, True
                    m.accumulate_matches(gt_mask, pred_mask, score[f][p_in], idx_pred, idx_gt, r["moving"][f][g_in].astype(bool), thr,
                                         class_name, r["sums"][f, j])

    @staticmethod
    def _feed_waymo(r, t, m, jobs, score):
        for f in range(score.shape[0]):
            for (class_name, crit), j in jobs.items():
                fi = t.jobs[j].filter
                g_in, p_in = r["assign_gt_in"][f, fi].astype(bool), r["assign_pred_in"][f, fi].astype(bool)
                pr = r["assign_pairs"][f, j, :int(r["assign_count"][f, j])].astype(np.int64)
                idx_gt, idx_pred = (np.cumsum(g_in) - 1)[pr[:, 0]], (np.cumsum(p_in) - 1)[pr[:, 1]]
                gt_mask, pred_mask = np.zeros(int(g_in.sum()), bool), np.zeros(int(p_in.sum()), bool)
                gt_mask[idx_gt], pred_mask[idx_pred] = True, True
                m.accumulate_matches(gt_mask, pred_mask, score[f][p_in], idx_pred, idx_gt, r["hard"][f][g_in].astype(bool), crit, class_name)

    def compute(self, prefix: str = "") -> Dict[str, float]:
        """flushes, feeds the collections' book-keeping and returns the union of their `compute()` dictionaries under the reference's
        tags `<prefix>final_result/<category>/detection_metrics/<bin>/<criterion>/...`"""
        self.flush()
        for rec in self._host:
            self._feed(rec)
        self._host = []
        out = {}
        for c, m in zip(self.collections, self.metrics):
            out.update(m.compute(prefix + c.tag))
        return out
