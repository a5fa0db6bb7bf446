"""Harvest of the box-snippet database from tracked boxes: the step of `track_boxes_on_data_sequence` (reference
liso/tracker/tracking.py) that cuts, for chosen frames of every track, the points inside the refined box out of the sweep and
stores them in box coordinates -- :1521-1611 for tracked sequences, :1798-1891 for the `NotATracker` branch, :1893-1897 the size
cap.  The reference runs a Python loop per track and frame (the whole sweep times inv(sensor_T_box) in fp64, a boolean mask, a
device-to-host copy per snippet); here all snippets of a sequence are ONE call of include/liso_snippets.h
(liso_amd/csrc/snippet_harvest.hip) and the points stay on the device, from the sweeps to `BoxSnippetDb`.

* `cut_box_snippets_host`: numpy statement of the kernel's arithmetic (the host path and the CPU yardstick).
* `cut_box_snippets`: the device call.
* `draw_track_snippet_times`, `draw_untracked_box_idxs`: the reference's draws from numpy's global generator, in its order.
* `SnippetHarvester`: the database under construction.  Per sequence the host reads the J + 1 offsets; the LiDAR rows are read
  once, in `to_box_snippet_db()` (the ray-drop draws of `BoxAugmenter` are made on the host); the points are never read.

Arithmetic (both paths; the header states it in full): box_T_sensor is the closed-form inverse of the yaw-only pose in fp64 from the
widened fp32 box; p_box = ((m0*x + m1*y) + m2*z) + m3 per row in fp64, rounded once to fp32; inside when |p_box| <= float32(0.55)
* dims on all three axes, inclusive.  The reference writes the bound as `1.1 * 0.5 * box.dims` against a float32 tensor: Python
folds 1.1 * 0.5 to the double 0.55, torch rounds it to float32 and multiplies in float32, which is the bound used here
(tests/golden/make_snippet_harvest_golden.py asserts it).
"""
import numpy as np
import torch

from liso_amd import _lib as L
from liso_amd.kabsch.shape_utils import Shape
from liso_amd.tracker.augm_box_db_utils import get_empty_augm_box_db
from liso_amd.utils.device_args import opt_ptr

BLOAT_HALF = np.float32(0.55)  # 1.1 * 0.5 as the reference's float32 tensor product sees it
POINT_BYTES = 16  # one stored point: box-frame x, y, z and the intensity, float32


def _np(v):
    return v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)


def dense_boxes7(boxes):
    """Shape [J] (numpy or tensor attributes) or an array [J, 7] -> numpy float32 [J, 7]: x, y, z, dx, dy, dz, yaw"""
    if isinstance(boxes, Shape):
        pos, dims, rot = _np(boxes.pos), _np(boxes.dims), _np(boxes.rot)
        assert pos.ndim == 2 and pos.shape[-1] == 3 and dims.shape[-1] == 3, (pos.shape, dims.shape)
        return np.ascontiguousarray(np.concatenate([pos, dims, rot[:, :1]], -1).astype(np.float32))
    b = np.ascontiguousarray(_np(boxes), dtype=np.float32)
    assert b.ndim == 2 and b.shape[1] == 7, b.shape
    return b


def box_T_sensor_host(boxes7):
    """float32 [J, 7] -> inv(sensor_T_box) float64 [J, 4, 4], closed form"""
    b = boxes7.astype(np.float64)
    x, y, z, yaw = b[:, 0], b[:, 1], b[:, 2], b[:, 6]
    c, s = np.cos(yaw), np.sin(yaw)
    M = np.zeros((b.shape[0], 4, 4), np.float64)
    with np.errstate(invalid="ignore"):
        M[:, 0, 0], M[:, 0, 1], M[:, 0, 3] = c, s, -(c * x + s * y)
        M[:, 1, 0], M[:, 1, 1], M[:, 1, 3] = -s, c, s * x - c * y
    M[:, 2, 2], M[:, 2, 3], M[:, 3, 3] = 1.0, -z, 1.0
    return M


def cut_box_snippets_host(clouds, counts, lidar_rows, job_cloud, boxes, capacity=None):
    """numpy: clouds float32 [T, n_max, C >= 4] (intensity last), counts int [T] or None, lidar_rows int32 [T, n_max] or None,
    job_cloud int [J], boxes (Shape [J] or [J, 7]) -> (offsets int64 [J + 1], points float32 [rows, 4], rows int32 [rows] or None,
    box_T_sensor float64 [J, 4, 4]); `rows` is the total, or `capacity` when given (rows behind the total are zero)."""
    clouds = np.asarray(clouds, np.float32)
    assert clouds.ndim == 3 and clouds.shape[2] >= 4, clouds.shape
    T, n_max = clouds.shape[:2]
    b7 = dense_boxes7(boxes)
    job_cloud = np.asarray(job_cloud, np.int64).reshape(-1)
    J = job_cloud.shape[0]
    assert b7.shape[0] == J, (b7.shape, J)
    M = box_T_sensor_host(b7)
    pts, rows, sizes = [], [], np.zeros(J, np.int64)
    for j in range(J):
        t = int(job_cloud[j])
        if not 0 <= t < T:
            continue
        n = n_max if counts is None else min(max(int(counts[t]), 0), n_max)
        P = clouds[t, :n]
        x, y, z = (P[:, k].astype(np.float64) for k in range(3))
        with np.errstate(invalid="ignore"):
            q = np.stack([(((M[j, r, 0] * x + M[j, r, 1] * y) + M[j, r, 2] * z) + M[j, r, 3]).astype(np.float32) for r in range(3)], -1)
            inside = (np.abs(q) <= BLOAT_HALF * b7[j, 3:6]).all(-1)
        sizes[j] = int(inside.sum())
        pts.append(np.concatenate([q[inside], P[inside][:, -1:]], -1))
        if lidar_rows is not None:
            rows.append(np.asarray(lidar_rows[t, :n], np.int32)[inside])
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    points = np.concatenate(pts, 0).astype(np.float32) if pts else np.zeros((0, 4), np.float32)
    out_rows = (np.concatenate(rows) if rows else np.zeros(0, np.int32)) if lidar_rows is not None else None
    if capacity is not None:
        fit = lambda a: np.concatenate([a[:capacity], np.zeros((max(0, capacity - a.shape[0]),) + a.shape[1:], a.dtype)])  # noqa: E731
        points, out_rows = fit(points), (fit(out_rows) if out_rows is not None else None)
    return offsets, points, out_rows, M


@torch.no_grad()
def cut_box_snippets(clouds, counts, lidar_rows, job_cloud, boxes, capacity=None):
    """device: clouds float32 [T, n_max, C >= 4] (cuda), counts int32 [T] or None, lidar_rows int32 [T, n_max] or None, job_cloud
    (host integers: checked to lie in [0, T) and uploaded; a device tensor is taken as it is), boxes (Shape [J] or [J, 7]) ->
    (offsets int64 [J + 1], points float32 [capacity, 4], rows int32 [capacity] or None, box_T_sensor float64 [J, 4, 4]), all on
    the device.  With `capacity=None` the buffers are sized by one read of offsets[J] after a count-only call; with a capacity
    nothing is read back (graph-capturable) and the caller compares offsets[J] to it."""
    L.require_cuda(clouds)
    assert clouds.dim() == 3 and clouds.shape[2] >= 4 and clouds.dtype == torch.float32, (clouds.shape, clouds.dtype)
    clouds = clouds.contiguous()
    dev = clouds.device
    T, n_max, stride = clouds.shape
    if torch.is_tensor(job_cloud) and job_cloud.is_cuda:
        jc = job_cloud.to(torch.int32).contiguous()
    else:
        host = np.asarray(_np(job_cloud), np.int64).reshape(-1)
        assert host.size == 0 or (host.min() >= 0 and host.max() < T), f"job_cloud outside [0, {T})"
        jc = torch.from_numpy(host.astype(np.int32)).to(dev)
    if torch.is_tensor(boxes) and boxes.is_cuda:
        b7 = boxes.float().contiguous()
    elif isinstance(boxes, Shape) and torch.is_tensor(boxes.pos) and boxes.pos.is_cuda:
        b7 = torch.cat([boxes.pos, boxes.dims, boxes.rot[..., :1]], dim=-1).float().contiguous()
    else:
        b7 = torch.from_numpy(dense_boxes7(boxes)).to(dev)
    J = jc.shape[0]
    assert b7.shape == (J, 7), (b7.shape, J)
    cnt = counts.to(torch.int32).contiguous() if counts is not None else None
    rows_in = lidar_rows.to(torch.int32).contiguous() if lidar_rows is not None else None
    assert rows_in is None or rows_in.shape == (T, n_max), rows_in.shape
    offsets = torch.empty(J + 1, dtype=torch.int64, device=dev)
    box_T = torch.empty((J, 4, 4), dtype=torch.float64, device=dev)
    ws_bytes = int(L.lib().liso_snippet_cut_workspace_bytes(T, n_max, J))
    if ws_bytes == 0:
        raise L.LisoHipError(f"snippet_cut: sizes out of range (T={T}, n_max={n_max}, J={J})")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)

    def call(cap, points, rows):
        with torch.cuda.device(dev):
            L.check(L.TIMER.launch("snippet_cut", lambda: L.lib().liso_snippet_cut_f32(
                T, n_max, stride, L.ptr(clouds), opt_ptr(cnt), opt_ptr(rows_in if rows is not None else None), J, L.ptr(jc), L.ptr(b7), cap,
                L.ptr(offsets), opt_ptr(points), opt_ptr(rows), L.ptr(box_T), L.ptr(ws), ws_bytes, L.stream_ptr())), "snippet_cut")

    if capacity is None:
        call(0, None, None)
        capacity = int(offsets[J].item())
    capacity = int(capacity)
    points = torch.empty((capacity, 4), dtype=torch.float32, device=dev)
    rows = torch.empty(capacity, dtype=torch.int32, device=dev) if rows_in is not None else None
    call(capacity, *((points, rows) if capacity > 0 else (None, None)))  # (an empty tensor has no address to hand over)
    return offsets, points, rows, box_T


# ---- the reference's draws -------------------------------------------------------------------------------------------------------
def draw_track_snippet_times(track_len, start_time_idx, dist_covered_m, min_track_age):
    """reference :1541-1565: short tracks are sampled less often, far-travelled ones more; -> sweep indices of the chosen frames"""
    assert track_len >= min_track_age, (track_len, min_track_age)
    num = (int(track_len) // int(min_track_age)) * int(dist_covered_m)
    num = min(max(1, num), min(10, int(track_len)))
    return np.random.choice(np.arange(start=int(start_time_idx), stop=int(track_len + start_time_idx), step=1), size=num, replace=False)


def draw_untracked_box_idxs(probs, max_num=3):
    """reference :1825-1842: all boxes of the frame when there are at most `max_num`, else a confidence-weighted choice"""
    probs = _np(probs).reshape(-1)  # in the dtype they come in: the reference adds and normalises in the boxes' own precision
    n = probs.shape[0]
    if min(max_num, n) >= n:
        return np.arange(n)
    p = probs + 1e-6
    p /= p.sum()
    return np.random.choice(np.arange(n), size=max_num, p=p, replace=False)


# ---- the database under construction --------------------------------------------------------------------------------------------
def _cat(parts):
    return torch.cat(parts, 0) if torch.is_tensor(parts[0]) else np.concatenate(parts, 0)


def _span_index(offsets, keep):
    """row indices of the snippets `keep` (in that order) of a concatenated buffer"""
    spans = [np.arange(offsets[j], offsets[j + 1]) for j in keep]
    return np.concatenate(spans).astype(np.int64) if spans else np.zeros(0, np.int64)


def _take(buf, idx):
    if torch.is_tensor(buf):
        return buf.index_select(0, torch.from_numpy(idx).to(buf.device))
    return buf[idx]


class SnippetHarvester:
    """The snippet database of one mining round.  Device sweeps give a device-resident store (points, LiDAR rows and inverse poses
    as concatenated tensors); numpy sweeps run the host path and give a numpy store.  Boxes, snippet sizes and track ids, a few
    numbers per snippet, live on the host."""

    def __init__(self, max_augm_db_size_mb):
        self.max_augm_db_size_mb = max_augm_db_size_mb
        self.max_track_id = 0  # reference :1566-1567: every harvested track gets a fresh id
        self.points = None  # [P, 4] float32
        self.rows = None  # [P] int32, or None when the sweeps came without LiDAR rows
        self.box_T_sensor = None  # [M, 4, 4] float64
        self.counts = np.zeros(0, np.int64)
        self.boxes = []  # M Shapes of shape (), host tensors
        self.unique_track_id = []

    def __len__(self):
        return len(self.boxes)

    @property
    def offsets(self):
        return np.concatenate([[0], np.cumsum(self.counts)]).astype(np.int64)

    def size_mb(self):
        """estimate_augm_db_size_mb: the bytes of the stored points"""
        return int(self.counts.sum()) * POINT_BYTES * 1e-6

    # -- one sequence ------------------------------------------------------------------------------------------------------------
    def _cut_and_append(self, clouds, counts, lidar_rows, job_cloud, job_boxes, job_ids):
        if job_boxes:
            stacked = Shape(**{k: torch.stack([torch.as_tensor(_np(getattr(b, k))) for b in job_boxes]) for k in ("pos", "dims", "rot", "probs")})
            if torch.is_tensor(clouds):
                offsets, points, rows, box_T = cut_box_snippets(clouds, counts, lidar_rows, job_cloud, stacked)
                offsets = offsets.cpu().numpy()  # the J + 1 numbers the host reads per sequence
            else:
                offsets, points, rows, box_T = cut_box_snippets_host(clouds, counts, lidar_rows, job_cloud, stacked)
            sizes = np.diff(offsets)
            keep = np.flatnonzero(sizes > 0)  # an empty box is of no use for pasting (the reference's `continue`)
            if keep.size:
                if keep.size < sizes.size:
                    idx = _span_index(offsets, keep)
                    points, rows = _take(points, idx), (_take(rows, idx) if rows is not None else None)
                    box_T = _take(box_T, keep.astype(np.int64))
                assert len(self) == 0 or (rows is None) == (self.rows is None), "sequences with and without lidar_rows in one database"
                self.points = points if self.points is None else _cat([self.points, points])
                if rows is not None:
                    self.rows = rows if self.rows is None else _cat([self.rows, rows])
                self.box_T_sensor = box_T if self.box_T_sensor is None else _cat([self.box_T_sensor, box_T])
                self.counts = np.concatenate([self.counts, sizes[keep]])
                self.boxes += [_host_box(job_boxes[j]) for j in keep]
                self.unique_track_id += [job_ids[j] for j in keep]
        self._apply_size_cap()

    def add_tracked_sequence(self, clouds, counts, lidar_rows, sensor_refined, world_refined, min_track_age):
        """reference :1523-1611.  `sensor_refined` / `world_refined`: {(track_id, start_time_idx): Shape [track_len]}, the refined
        boxes of every kept track in sensor and in world coordinates."""
        job_cloud, job_boxes, job_ids = [], [], []
        for (track_id, start_time_idx), boxes_sensor in sensor_refined.items():
            boxes_world = world_refined[(track_id, start_time_idx)]
            track_len = boxes_sensor.shape[0]
            assert np.allclose(_np(boxes_world.dims), _np(boxes_sensor.dims)), "error: dims change with coordinate system"
            assert boxes_world.shape == boxes_sensor.shape, (track_id, boxes_world.shape, boxes_sensor.shape)
            dist_covered_m = np.linalg.norm(_np(boxes_world.pos[-1]) - _np(boxes_world.pos[0]))
            time_idxs = draw_track_snippet_times(track_len, start_time_idx, dist_covered_m, min_track_age)
            unique_track_id = self.max_track_id
            self.max_track_id += 1
            for t in time_idxs:
                job_cloud.append(int(t))
                job_boxes.append(boxes_sensor[int(t - start_time_idx)])  # the box sequence starts later than the sweeps
                job_ids.append(unique_track_id)
        self._cut_and_append(clouds, counts, lidar_rows, job_cloud, job_boxes, job_ids)

    def add_untracked_sequence(self, clouds, counts, lidar_rows, boxes_per_time, track_ids_per_time):
        """reference :1798-1891 (`NotATracker`): up to three boxes of every frame, chosen by confidence"""
        job_cloud, job_boxes, job_ids = [], [], []
        for t, boxes_at_t in enumerate(boxes_per_time):
            if np.count_nonzero(_np(boxes_at_t.valid)) == 0:
                continue
            for i in draw_untracked_box_idxs(np.squeeze(_np(boxes_at_t.probs), -1)):
                job_cloud.append(t)
                job_boxes.append(boxes_at_t[int(i)])
                job_ids.append(int(_np(track_ids_per_time[t])[int(i)]))
        self._cut_and_append(clouds, counts, lidar_rows, job_cloud, job_boxes, job_ids)

    # -- the size cap (reference :1893-1897 with drop_boxes_from_augmentation_db, augm_box_db_utils.py:78-110) ----------------------
    def _apply_size_cap(self):
        before = self.size_mb()
        if before <= self.max_augm_db_size_mb:
            return
        M = len(self)
        conf = np.squeeze(np.stack([_np(b.probs) for b in self.boxes]), axis=-1)
        num_keep = int(M / (before / self.max_augm_db_size_mb))
        # (the reference tests `len(np.unique(conf) == 1)`, true for any non-empty database: the random branch is the one that runs)
        if len(np.unique(conf) == 1):
            keep = np.random.choice(np.arange(0, M), num_keep, replace=False)
        else:
            floor, mask = conf.min(), np.ones_like(conf, dtype=bool)
            while mask.sum() > num_keep:
                floor = floor + 0.001
                mask[conf < floor] = False
            keep = np.arange(0, M)[mask]
        self.keep_snippets(keep)

    def keep_snippets(self, keep):
        """the database of the snippets `keep`, in that order: one gather of the point rows"""
        keep = np.asarray(keep, np.int64)
        idx = _span_index(self.offsets, keep)
        self.points = _take(self.points, idx)
        self.rows = _take(self.rows, idx) if self.rows is not None else None
        self.box_T_sensor = _take(self.box_T_sensor, keep)
        self.counts = self.counts[keep]
        self.boxes = [self.boxes[i] for i in keep]
        self.unique_track_id = [self.unique_track_id[i] for i in keep]

    # -- what leaves -------------------------------------------------------------------------------------------------------------
    def stacked_boxes(self):
        """host Shape [M]"""
        return Shape(**{k: torch.stack([getattr(b, k) for b in self.boxes]) for k in Shape._keys})

    def to_box_snippet_db(self, device=None):
        from liso_amd.datasets.box_augmentation import BoxSnippetDb

        assert len(self) > 0, "nothing was harvested"
        if torch.is_tensor(self.points):
            return BoxSnippetDb.from_device(self.points, self.offsets, self.stacked_boxes(), lidar_rows=self.rows, box_T_sensor=self.box_T_sensor)
        assert device is not None, "a host-side store needs the device to move to"
        return BoxSnippetDb(self.to_dict(stacked=True), device)

    def to_dict(self, stacked=False):
        """The reference's dictionary: per-snippet lists (`save_augmentation_database` writes it,
        `load_sanitize_box_augmentation_database` reads it back).  `stacked=True`: the form that is saved -- boxes as the attribute
        dictionary of a numpy Shape [M], box_T_sensor [M, 4, 4], unique_track_id uint32 [M]."""
        db = get_empty_augm_box_db()
        if len(self) == 0:
            return db
        off = self.offsets
        points, box_T = _np(self.points), _np(self.box_T_sensor)
        rows = _np(self.rows) if self.rows is not None else None
        db["pcl_in_box_cosy"] = [points[off[i]:off[i + 1]] for i in range(len(self))]
        db["lidar_rows"] = [rows[off[i]:off[i + 1]] for i in range(len(self))] if rows is not None else []
        if stacked:
            db["boxes"] = self.stacked_boxes().numpy().__dict__
            db["box_T_sensor"] = box_T
            db["unique_track_id"] = np.asarray(self.unique_track_id).astype(np.uint32)
            if rows is None:
                del db["lidar_rows"]
        else:
            db["boxes"] = list(self.boxes)
            db["box_T_sensor"] = [box_T[i] for i in range(len(self))]
            db["unique_track_id"] = list(self.unique_track_id)
        return db


def _host_box(box):
    """a Shape of shape () with host tensor attributes"""
    return Shape(**{k: torch.as_tensor(_np(getattr(box, k))).clone() for k in Shape._keys})
