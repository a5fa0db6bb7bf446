"""Track mining on the device (include/liso_track_mining.h, csrc/track_mining.hip): the stage of `track_boxes_on_data_sequence`
(reference liso/tracker/tracking.py) between the tracker and the databases -- the loop over `get_ids_lengths_of_longest_tracks()`
(:1099-1328: age and confidence filters, `decide_keep_or_drop_box`, `perform_local_box_refinement`,
`update_world_boxes_from_sensor_boxes`, the median confidence, track smoothing or a constant speed, `update_db_with_this_box_stuff`) and
the fold of the kept tracks into the per-sample `tracked_boxes_db` / `tracked_boxes_conf_stats` (:1613-1681) -- for a padded batch of
sequences, from `TrackedSequences` (liso_amd/tracker/device_tracker.py) to `MinedTracks`, without a copy to the host.

* `mine_tracked_sequences`       the whole stage on device tensors (no synchronisation; graph-capturable with "jerk" and "none")
* `select_tracks`, `refine_tracks`, `smooth_tracks`, `export_tracks`   its parts, callable on their own
* `mine_tracked_sequences_host`  the same contract in numpy / fp64: the yardstick of the device tests
* `MinedTracks.kept_tracks(s)`   what `SnippetHarvester.add_tracked_sequence` takes; `MinedTracks.to_dict(sample_ids)` the mined-box
                                 database of `save_mined_box_db` (liso_amd/tracker/mined_box_db_utils.py), the one copy to the host

A track is what `TrackedSequences.track_table(max_tracks)` says: its rows in frame order, row k taken as the row of frame start + k (the
reference's assumption at :1109-1115), hole-filling rows included.  THE ORDER OF TRACKS is that of
`DeviceFlowBasedBoxTracker.get_ids_lengths_of_longest_tracks`: descending length, EQUAL LENGTHS BY ASCENDING ID, where the reference
inherits whatever `torch.argsort` does with ties.  Inside a frame of the result the rows follow the reference's dict insertion order:
kept tracks that are not smoothed in track order (:1226), then the smoothed ones in track order (:1319).

Where this differs from the reference, all of it a consequence of static shapes:
* the smoothing sees every track padded to the T frames of the batch, not to the longest queued track.  So the reference's "tracks are
  too short" branch (:1250, longest queued track <= 4 frames) is decided on T; a queued track shorter than T has free frames behind
  its end (which the jerk objective may use, as it does for every but the longest track of a reference batch), and the displacement of
  a track's last row looks at the zero padding behind it, as it does in the reference for every but the longest track.
* one smoothing call is made per sequence ([max_tracks, T] tables, rows of tracks without SMOOTHED invalid): the jerk kernel scales its
  gradient by the number of rows of the call, so a call over the whole batch would make a sequence's result depend on its neighbours.
* `"bike_model"` runs L-BFGS, which reads its loss on the host at every step: that branch selects the smoothed tracks with one read
  and is not capturable.
* the per-frame `velo` is that of the world box (the mined speed): the detections come without one.
Confidences and dims are taken to be finite (a NaN confidence makes `torch.median` NaN in the reference)."""
import dataclasses
from typing import Optional

import numpy as np
import torch

from liso_amd import _lib as L
from liso_amd.kabsch.shape_utils import UNKNOWN_CLASS_ID, Shape
from liso_amd.tracker.device_tracker import TrackedSequences
from liso_amd.tracker.track_smoothing import (MIN_TRACK_LEN_FOR_SMOOTHING, batched_displacement_from_pos, smooth_track_bike_model,
                                              smooth_track_jerk)
from liso_amd.utils.device_args import opt_ptr

AGE_OK, CONF_OK, KEPT, SMOOTHED = 1, 2, 4, 8  # LISO_MINE_* of include/liso_track_mining.h
MAX_FRAMES, MAX_TRACKS = 1024, 8192  # LISO_MINE_MAX_FRAMES, LISO_MINE_MAX_TRACKS
QUANTILE_FLOW_CLUSTER, QUANTILE_NETWORK = 0.95, 0.6  # perform_local_box_refinement: box_dims_quantile


def dims_quantile(is_flow_cluster_detector):
    return QUANTILE_FLOW_CLUSTER if is_flow_cluster_detector else QUANTILE_NETWORK


# ---- host restatement --------------------------------------------------------------------------------------------------------------
def _compose(x, y, z, yaw):
    c, s = np.cos(yaw), np.sin(yaw)
    return np.array([[c, -s, 0.0, x], [s, c, 0.0, y], [0.0, 0.0, 1.0, z], [0.0, 0.0, 0.0, 1.0]], np.float64)


def _decompose(M):
    return M[:3, 3].copy(), np.arctan2(M[1, 0], M[0, 0])


def track_table_host(track_ids, max_tracks):
    """numpy `TrackedSequences.track_table`: rows int64 [S,max_tracks,T], the row of track m + 1 in each frame or -1"""
    S, T, _ = track_ids.shape
    rows = np.full((S, max_tracks, T), -1, np.int64)
    for s, t, r in zip(*np.where((track_ids >= 1) & (track_ids <= max_tracks))):
        rows[s, track_ids[s, t, r] - 1, t] = r
    return rows


def resize_keeping_closest_corner_host(pos, rot, dims, new_dims):
    """set_box_size_keep_closest_point_constant (reference :239-260) for one box: pos fp64 [3], rot fp64, dims / new_dims fp32 [3]"""
    c, s = np.cos(rot), np.sin(rot)
    best, corner = None, None
    for sx, sy in ((0.5, -0.5), (0.5, 0.5), (-0.5, -0.5), (-0.5, 0.5)):  # the bottom corners 0, 1, 4, 5 of Shape.get_box_corners
        ux, uy = np.float64(np.float32(sx) * dims[0]), np.float64(np.float32(sy) * dims[1])
        x, y = (c * ux + (-s) * uy) + pos[0], (s * ux + c * uy) + pos[1]
        r = np.sqrt(x * x + y * y)
        if best is None or r < best:
            best, corner = r, np.array([x, y, np.float64(np.float32(-0.5) * dims[2]) + pos[2]])
    with np.errstate(divide="ignore", invalid="ignore"):
        return corner + (new_dims / dims).astype(np.float64) * (pos - corner)


def mine_tracked_sequences_host(tracked, boxes, conf, clouds=None, counts=None, *, max_tracks, cap_out, min_track_age,
                                confidence_threshold_mined_boxes, min_track_obj_speed_mps, time_between_frames_s, is_flow_cluster_detector,
                                flow_cluster_detector_min_travel_dist_filter_m, fit_rot=False, fit_pos=False, fitting_dims_bloat_factor=1.0,
                                min_dist_for_track_smoothing=5.0, use_track_smoothing=True, track_smoothing_method="none",
                                in_annotated_fov=None, export_only_in_annotated_fov=False, margin=None, fits=None, smoother=None):
    """`tracked`: dict of numpy arrays named like the fields of `TrackedSequences` (what `track_sequences_host` returns); the other
    arguments as `mine_tracked_sequences` takes them, as numpy arrays -> dict of numpy arrays: the per-track fields, `sensor_raw_*`,
    `world_raw_*`, `refined_sensor_*` (the boxes behind the refinement, before the world round trip), `sensor_*`, `world_*`, `dims`,
    `probs`, `velo` per track row, `smooth_in_pos` / `smooth_in_yaw` / `smooth_in_valid` (the tables the smoothing is given) and
    `frame_*` per frame.  fp64 throughout; the quantile is the fp64 interpolation (`refined_dims_f64`) rounded once to fp32.

    With `margin`, every threshold a distance is compared to asserts that the decision is not within `margin` of it: the speed, the
    travel filter and `min_dist_for_track_smoothing` of every track that reaches them.  Confidence comparisons are exact fp32.
    The rectangle fit and the optimising smoothers are kernels: with `fit_rot` / `fit_pos` the caller passes `fits` = (count int32
    [S,T,M], fit float64 [S,T,M,5]) as the device produced them; a `track_smoothing_method` other than "none" needs `smoother(pos32,
    yaw32, valid) -> (pos, yaw, velo)` for one sequence's tables (numpy in, numpy out)."""
    del clouds, counts, fitting_dims_bloat_factor  # (only the fit reads them)
    ids, src, W = tracked["track_ids"], tracked["src"], tracked["w_T_sensor"]
    pos_world, rot_world = tracked["pos_world"], tracked["rot_world"]
    boxes, conf = np.asarray(boxes, np.float32), np.asarray(conf, np.float32)
    S, T, cap = ids.shape
    K, M, dt = boxes.shape[2], int(max_tracks), float(time_between_frames_s)
    assert not (fit_rot or fit_pos) or fits is not None, "the rectangle fit is a kernel: pass its results as `fits`"
    rows = track_table_host(ids, M)
    q = dims_quantile(is_flow_cluster_detector)
    f64, f32 = np.float64, np.float32
    out = {"n_tracks": np.maximum(ids.reshape(S, -1).max(axis=1), 0).astype(np.int64), "overflow": np.zeros(S, np.int32),
           "age": np.zeros((S, M), np.int32), "start": np.zeros((S, M), np.int32), "median_conf": np.zeros((S, M), f32),
           "dist_covered_m": np.zeros((S, M), f64), "verdict": np.zeros((S, M), np.uint8), "refined_dims": np.zeros((S, M, 3), f32),
           "refined_dims_f64": np.zeros((S, M, 3), f64)}
    for k in ("sensor_raw", "world_raw", "refined_sensor", "sensor", "world"):
        out[k + "_pos"], out[k + "_rot"] = np.zeros((S, M, T, 3), f64), np.zeros((S, M, T, 1), f64)
    out.update(raw_dims=np.zeros((S, M, T, 3), f32), raw_probs=np.zeros((S, M, T, 1), f32), dims=np.zeros((S, M, T, 3), f32),
               probs=np.zeros((S, M, T, 1), f32), velo=np.zeros((S, M, T, 1), f32), smooth_in_pos=np.zeros((S, M, T, 3), f32),
               smooth_in_yaw=np.zeros((S, M, T, 1), f32), smooth_in_valid=np.zeros((S, M, T), bool))
    track_rows = np.full((S, M, T), -1, np.int64)
    for s in range(S):
        for m in range(M):
            frames = np.where((rows[s, m] >= 0) & (rows[s, m] < cap))[0]
            n = len(frames)
            if n == 0:
                continue
            start = int(frames[0])
            r = rows[s, m, frames]
            track_rows[s, m, :n] = r
            at = [(start + k, int(r[k])) for k in range(n)]  # row k is taken as the row of frame start + k
            det = [src[s, f, i] for f, i in at]
            ok = [0 <= a < T and 0 <= b < K for a, b in det]
            c = np.array([conf[s, a, b] if o else 0.0 for (a, b), o in zip(det, ok)], f32)
            d = np.array([boxes[s, a, b, 3:6] if o else np.zeros(3, f32) for (a, b), o in zip(det, ok)], f32).reshape(n, 3)
            median = np.sort(c, kind="stable")[(n - 1) // 2]
            qpos = q * (n - 1)
            lo, hi = int(np.floor(qpos)), int(np.ceil(qpos))
            col = np.sort(d.astype(f64), axis=0)
            out["refined_dims_f64"][s, m] = col[lo] + (col[hi] - col[lo]) * (qpos - lo)
            refined = out["refined_dims_f64"][s, m].astype(f32)
            first, last = pos_world[s, at[0][0], at[0][1]], pos_world[s, at[-1][0], at[-1][1]]
            dx, dy = last[0] - first[0], last[1] - first[1]
            dist = np.sqrt(dx * dx + dy * dy)
            verdict = 0
            if n >= min_track_age:
                verdict |= AGE_OK
                if median >= f32(confidence_threshold_mined_boxes):
                    verdict |= CONF_OK
                    keep = True
                    if min_track_obj_speed_mps > 0.0:
                        speed = dist / (n * dt)
                        assert margin is None or abs(speed - min_track_obj_speed_mps) > margin, ("speed within the margin", s, m, speed)
                        keep = speed >= min_track_obj_speed_mps
                    if keep and is_flow_cluster_detector:
                        assert margin is None or abs(dist - flow_cluster_detector_min_travel_dist_filter_m) > margin, ("travel", s, m, dist)
                        keep = dist >= flow_cluster_detector_min_travel_dist_filter_m
                    if keep:
                        verdict |= KEPT
                        assert margin is None or abs(dist - min_dist_for_track_smoothing) > margin, ("smoothing distance", s, m, dist)
                        if dist > min_dist_for_track_smoothing and use_track_smoothing and n >= MIN_TRACK_LEN_FOR_SMOOTHING:
                            verdict |= SMOOTHED
            out["age"][s, m], out["start"][s, m], out["median_conf"][s, m], out["dist_covered_m"][s, m] = n, start, median, dist
            out["verdict"][s, m], out["refined_dims"][s, m] = verdict, refined
            if not verdict & KEPT:
                continue
            for k, (f, i) in enumerate(at):
                wp, wr = pos_world[s, f, i], rot_world[s, f, i]
                sp, sr = _decompose(np.linalg.inv(W[s, f]) @ _compose(wp[0], wp[1], wp[2], wr))
                out["world_raw_pos"][s, m, k], out["world_raw_rot"][s, m, k], out["raw_dims"][s, m, k], out["raw_probs"][s, m, k] = wp, wr, d[k], c[k]
                out["sensor_raw_pos"][s, m, k], out["sensor_raw_rot"][s, m, k] = sp, sr
                if fits is not None and fits[0][s, f, m] > 0:
                    fit = fits[1][s, f, m]
                    if fit_rot:
                        sr = sr + (fit[4] - sr)
                    if fit_pos:
                        sp[:2] = fit[:2]
                sp = resize_keeping_closest_corner_host(sp, sr, d[k], refined)
                out["refined_sensor_pos"][s, m, k], out["refined_sensor_rot"][s, m, k] = sp, sr
                out["world_pos"][s, m, k], out["world_rot"][s, m, k] = _decompose(W[s, f] @ _compose(sp[0], sp[1], sp[2], sr))
                out["dims"][s, m, k], out["probs"][s, m, k] = refined, median
                if not verdict & SMOOTHED:
                    out["velo"][s, m, k] = f32(dist) / (f32(n) * f32(dt))
        # ---- smoothing: one sequence's tables, tracks without SMOOTHED invalid
        valid = ((out["verdict"][s] & SMOOTHED) != 0)[:, None] & (np.arange(T)[None] < out["age"][s][:, None])
        pos32 = (out["world_pos"][s] * valid[..., None]).astype(f32)
        yaw32 = (out["world_rot"][s] * valid[..., None]).astype(f32)
        out["smooth_in_pos"][s], out["smooth_in_yaw"][s], out["smooth_in_valid"][s] = pos32, yaw32, valid
        if valid.any():
            if track_smoothing_method == "none" or T <= 4:
                step = np.linalg.norm(pos32[:, 1:] - pos32[:, :-1], axis=-1)
                new_pos, new_yaw, new_velo = pos32, yaw32, np.concatenate([step, step[:, -1:]], axis=1)[..., None]
            else:
                assert smoother is not None, "an optimising smoother is a kernel: pass `smoother`"
                new_pos, new_yaw, new_velo = smoother(pos32.copy(), yaw32.copy(), valid.copy())
            out["world_pos"][s][valid], out["world_rot"][s][valid] = new_pos[valid].astype(f64), new_yaw[valid].astype(f64)
            out["velo"][s][valid] = new_velo[valid].astype(f32)
        # ---- the sensor boxes from the world boxes
        for m in range(M):
            if out["verdict"][s, m] & KEPT:
                for k in range(out["age"][s, m]):
                    wp, wr, f = out["world_pos"][s, m, k], out["world_rot"][s, m, k, 0], out["start"][s, m] + k
                    out["sensor_pos"][s, m, k], out["sensor_rot"][s, m, k] = _decompose(np.linalg.inv(W[s, f]) @ _compose(wp[0], wp[1], wp[2], wr))
    # ---- the per-frame tables
    C = int(cap_out)
    fr = {"n_boxes": np.zeros((S, T), np.int32), "pos": np.zeros((S, T, C, 3), f64), "rot": np.zeros((S, T, C, 1), f64),
          "dims": np.zeros((S, T, C, 3), f32), "probs": np.zeros((S, T, C, 1), f32), "velo": np.zeros((S, T, C, 1), f32),
          "track_id": np.full((S, T, C), -1, np.int64), "lidar_T_box": np.zeros((S, T, C, 4, 4), f64),
          "max_confidence": np.full((S, T), -np.inf, f32), "valid": np.zeros((S, T, C), np.uint8)}
    for s in range(S):
        order = sorted(range(M), key=lambda m: (-int(out["age"][s, m]), m))  # descending length, equal lengths by ascending id
        order = [m for m in order if not out["verdict"][s, m] & SMOOTHED] + [m for m in order if out["verdict"][s, m] & SMOOTHED]
        for m in order:
            if not out["verdict"][s, m] & KEPT:
                continue
            for k in range(out["age"][s, m]):
                t = int(out["start"][s, m]) + k
                if export_only_in_annotated_fov:
                    a, b = src[s, t, track_rows[s, m, k]]
                    if not (0 <= a < T and 0 <= b < K and in_annotated_fov[s, a, b]):
                        continue
                i = int(fr["n_boxes"][s, t])
                if i >= C:
                    out["overflow"][s] += 1
                    continue
                fr["n_boxes"][s, t] = i + 1
                sp, sr = out["sensor_pos"][s, m, k], out["sensor_rot"][s, m, k, 0]
                fr["pos"][s, t, i], fr["rot"][s, t, i], fr["dims"][s, t, i], fr["probs"][s, t, i] = sp, sr, out["dims"][s, m, k], out["probs"][s, m, k]
                fr["velo"][s, t, i], fr["track_id"][s, t, i], fr["valid"][s, t, i] = out["velo"][s, m, k], m + 1, 1
                fr["lidar_T_box"][s, t, i] = _compose(sp[0], sp[1], sp[2], sr)
                fr["max_confidence"][s, t] = max(fr["max_confidence"][s, t], out["probs"][s, m, k, 0])
    out.update({"frame_" + k: v for k, v in fr.items()})
    return out


# ---- device ------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class SelectedTracks:
    """stage 1 (liso_select_tracks): the per-track fields, the raw boxes of the kept tracks' rows ([S,M,T]) and the per-frame box
    lists of the rectangle fit ([S,T,M,7], NaN where a track has no box); `workspace` is shared with the later stages"""
    n_tracks: torch.Tensor
    age: torch.Tensor
    start: torch.Tensor
    median_conf: torch.Tensor
    dist_covered_m: torch.Tensor
    verdict: torch.Tensor
    refined_dims: torch.Tensor
    sensor_raw: Shape
    world_raw: Shape
    fit_boxes: torch.Tensor
    workspace: torch.Tensor
    det_shape: tuple  # (K, cap) of the tracker's tables

    def row_valid(self, bit=KEPT):
        """bool [S,M,T]: row k of a track with `bit` set"""
        T = self.sensor_raw.pos.shape[2]
        return ((self.verdict & bit) != 0)[..., None] & (torch.arange(T, device=self.age.device).view(1, 1, T) < self.age[..., None])


@dataclasses.dataclass
class RefinedTracks:
    """stage 2 (liso_refine_tracks_apply): `sensor` the boxes behind the refinement, `world` what
    update_world_boxes_from_sensor_boxes makes of them, confidences the track's median, `world.velo` the constant speed of the kept
    tracks that are not smoothed; `fit_count` / `fit` [S,T,M(,5)] the rectangle fits, None when none was asked for"""
    sensor: Shape
    world: Shape
    fit_count: Optional[torch.Tensor]
    fit: Optional[torch.Tensor]


@dataclasses.dataclass
class FrameBoxes:
    """the mined boxes per frame, `cap_out` rows each (sensor coordinates), blank behind `n_boxes`"""
    n_boxes: torch.Tensor
    pos: torch.Tensor
    rot: torch.Tensor
    dims: torch.Tensor
    probs: torch.Tensor
    velo: torch.Tensor
    track_id: torch.Tensor
    lidar_T_box: torch.Tensor
    max_confidence: torch.Tensor
    valid: torch.Tensor


@dataclasses.dataclass
class MinedTracks:
    """device tensors only.  Per track [S,max_tracks]: age, start (int32), median_conf (float32), dist_covered_m (float64), verdict (uint8:
    AGE_OK | CONF_OK | KEPT | SMOOTHED), refined_dims (float32 [.,3]).  Per track row [S,max_tracks,T] as Shapes (pos, rot float64; dims,
    probs, velo float32; valid = row of a KEPT track): world_refined, sensor_refined, world_raw, sensor_raw.  Per frame: `frames`.
    `n_tracks` [S] (the caller compares it to max_tracks) and `overflow` [S] (rows that did not fit cap_out) are there to be looked at."""
    n_tracks: torch.Tensor
    overflow: torch.Tensor
    age: torch.Tensor
    start: torch.Tensor
    median_conf: torch.Tensor
    dist_covered_m: torch.Tensor
    verdict: torch.Tensor
    refined_dims: torch.Tensor
    world_refined: Shape
    sensor_refined: Shape
    world_raw: Shape
    sensor_raw: Shape
    frames: FrameBoxes

    @property
    def velo(self):
        return self.world_refined.velo

    @staticmethod
    def from_host(out, device="cpu"):
        """the dict of `mine_tracked_sequences_host` as a `MinedTracks` (tensors on `device`)"""
        t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(device) for k, v in out.items()}
        valid = ((t["verdict"] & KEPT) != 0)[..., None] & (torch.arange(t["dims"].shape[2], device=device).view(1, 1, -1) < t["age"][..., None])
        shape = lambda kind, dims, probs, **more: Shape(pos=t[kind + "_pos"], rot=t[kind + "_rot"], dims=dims, probs=probs, valid=valid, **more)  # noqa: E731
        frames = FrameBoxes(**{k: t["frame_" + k] for k in ("n_boxes", "pos", "rot", "dims", "probs", "velo", "track_id", "lidar_T_box",
                                                           "max_confidence", "valid")})
        return MinedTracks(t["n_tracks"], t["overflow"], t["age"], t["start"], t["median_conf"], t["dist_covered_m"], t["verdict"],
                           t["refined_dims"], shape("world", t["dims"], t["probs"], velo=t["velo"]), shape("sensor", t["dims"], t["probs"]),
                           shape("world_raw", t["raw_dims"], t["raw_probs"]), shape("sensor_raw", t["raw_dims"], t["raw_probs"]), frames)

    def kept_tracks(self, s):
        """-> (sensor_refined, world_refined): {(track_id, start_time_idx): Shape [track_len]} of sequence s, device tensors, in the
        reference's insertion order (kept tracks that are not smoothed in track order, then the smoothed ones) -- what
        `SnippetHarvester.add_tracked_sequence` takes.  Reads the sequence's age / start / verdict (3 max_tracks numbers)."""
        M = self.age.shape[1]
        host = torch.stack([self.age[s].long(), self.start[s].long(), self.verdict[s].long()]).cpu().numpy()
        age, start, verdict = host
        order = sorted(range(M), key=lambda m: (-int(age[m]), m))
        order = [m for m in order if verdict[m] & KEPT and not verdict[m] & SMOOTHED] + [m for m in order if verdict[m] & SMOOTHED]
        sensor, world = {}, {}
        for m in order:
            key, n = (m + 1, int(start[m])), int(age[m])
            sensor[key], world[key] = self.sensor_refined[s, m, :n], self.world_refined[s, m, :n]
        return sensor, world

    def to_dict(self, sample_ids):
        """sample_ids[s][t]: the name of frame t of sequence s -> (tracked_boxes_db, tracked_boxes_conf_stats) in the reference's layout
        (:1663-1681): db[name] = {"lidar_T_box": float64 [n,4,4], "raw_box": the `__dict__` of a numpy Shape [n], "track_id": int64 [n]},
        stats[name] = {"max_confidence": float, "num_boxes": int}.  A frame none of whose kept tracks has a row gets no entry at all; one
        whose rows all fail the FOV filter gets only the statistics (-inf, 0), as in the reference.  The one place that copies to the
        host."""
        f = self.frames
        host = {k: getattr(f, k).cpu().numpy() for k in ("n_boxes", "pos", "rot", "dims", "probs", "velo", "track_id", "lidar_T_box", "max_confidence")}
        age, start, verdict = self.age.cpu().numpy(), self.start.cpu().numpy(), self.verdict.cpu().numpy()
        db, stats = {}, {}
        S, T = host["n_boxes"].shape
        for s in range(S):
            kept = (verdict[s] & KEPT) != 0
            for t in range(T):
                if not (kept & (start[s] <= t) & (t < start[s] + age[s])).any():
                    continue
                name, n = sample_ids[s][t], int(host["n_boxes"][s, t])
                assert name not in stats, f"overwriting occuring for sample: {name}"
                if n > 0:
                    raw = Shape(pos=host["pos"][s, t, :n].copy(), dims=host["dims"][s, t, :n].copy(), rot=host["rot"][s, t, :n].copy(),
                                probs=host["probs"][s, t, :n].copy(), velo=host["velo"][s, t, :n].copy(), valid=np.ones(n, bool),
                                class_id=np.full((n, 1), UNKNOWN_CLASS_ID, np.int32))
                    db[name] = {"lidar_T_box": host["lidar_T_box"][s, t, :n].copy(), "raw_box": raw.__dict__,
                                "track_id": host["track_id"][s, t, :n].copy()}
                stats[name] = {"max_confidence": float(host["max_confidence"][s, t]), "num_boxes": n}
        return db, stats


def _new(dev):
    return lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)


def _refuse(what, S, T, K, cap, M):
    raise L.LisoHipError(f"{what}: sizes refused (S={S}, T={T}, K={K}, cap={cap}, max_tracks={M}; 1 <= T <= {MAX_FRAMES}, "
                         f"1 <= max_tracks <= {MAX_TRACKS}, K, cap >= 1)")


@torch.no_grad()
def select_tracks(tracked: TrackedSequences, boxes, conf, *, max_tracks, min_track_age, confidence_threshold_mined_boxes,
                  min_track_obj_speed_mps, time_between_frames_s, is_flow_cluster_detector, flow_cluster_detector_min_travel_dist_filter_m,
                  min_dist_for_track_smoothing=5.0, use_track_smoothing=True) -> SelectedTracks:
    """stage 1: `boxes` float32 [S,T,K,7] and `conf` float32 [S,T,K] are the tensors given to `track_sequences`"""
    L.require_cuda(tracked.track_ids, boxes, conf)
    S, T, cap = tracked.track_ids.shape
    K, M = boxes.shape[2], int(max_tracks)
    assert boxes.shape == (S, T, K, 7) and boxes.dtype == torch.float32, (boxes.shape, boxes.dtype)
    assert conf.shape == (S, T, K) and conf.dtype == torch.float32, (conf.shape, conf.dtype)
    ws_bytes = int(L.lib().liso_track_mining_workspace_bytes(S, T, K, cap, M))
    if ws_bytes == 0:
        _refuse("select_tracks", S, T, K, cap, M)
    boxes, conf = boxes.contiguous(), conf.contiguous()
    _, _, rows, n_tracks = tracked.track_table(M)
    rows = rows.contiguous()
    new = _new(boxes.device)
    i32, f32, f64 = torch.int32, torch.float32, torch.float64
    age, start, median, dist = new((S, M), i32), new((S, M), i32), new((S, M), f32), new((S, M), f64)
    verdict, refined = new((S, M), torch.uint8), new((S, M, 3), f32)
    wpos, wrot, spos, srot = new((S, M, T, 3), f64), new((S, M, T, 1), f64), new((S, M, T, 3), f64), new((S, M, T, 1), f64)
    dims, probs, fit_boxes = new((S, M, T, 3), f32), new((S, M, T, 1), f32), new((S, T, M, 7), f32)
    ws = new((ws_bytes,), torch.uint8)
    if S > 0:
        with torch.cuda.device(boxes.device):
            L.check(L.TIMER.launch("select_tracks", lambda: L.lib().liso_select_tracks(
                S, T, K, cap, M, L.ptr(rows), L.ptr(tracked.pos_world), L.ptr(tracked.rot_world), L.ptr(tracked.src), L.ptr(tracked.w_T_sensor),
                L.ptr(boxes), L.ptr(conf), int(min_track_age), float(confidence_threshold_mined_boxes), float(min_track_obj_speed_mps),
                float(time_between_frames_s), int(bool(is_flow_cluster_detector)), float(flow_cluster_detector_min_travel_dist_filter_m),
                float(min_dist_for_track_smoothing), int(bool(use_track_smoothing)), dims_quantile(is_flow_cluster_detector), L.ptr(age),
                L.ptr(start), L.ptr(median), L.ptr(dist), L.ptr(verdict), L.ptr(refined), L.ptr(wpos), L.ptr(wrot), L.ptr(spos), L.ptr(srot),
                L.ptr(dims), L.ptr(probs), L.ptr(fit_boxes), L.ptr(ws), ws_bytes, L.stream_ptr())), "select_tracks")
    sel = SelectedTracks(n_tracks, age, start, median, dist, verdict, refined, None, None, fit_boxes, ws, (K, cap))
    sel.sensor_raw = Shape(pos=spos, dims=dims, rot=srot, probs=probs)
    sel.world_raw = Shape(pos=wpos, dims=dims, rot=wrot, probs=probs)
    sel.sensor_raw.valid = sel.world_raw.valid = sel.row_valid()
    return sel


@torch.no_grad()
def refine_tracks(sel: SelectedTracks, tracked: TrackedSequences, clouds, counts, *, fit_rot, fit_pos, fitting_dims_bloat_factor,
                  time_between_frames_s) -> RefinedTracks:
    """stage 2: `clouds` float32 [S,T,N,C] NaN-padded with `counts` int32 [S,T] (the layout `cut_box_snippets` takes; read only with
    `fit_rot` / `fit_pos`).  Per sweep ONE call of `fit_boxes_to_points` over the boxes of all kept tracks of that frame -- S T launches
    (the fit takes one sweep per call) instead of one per track and frame -- then liso_refine_tracks_apply."""
    from liso_amd.tracker.tracking import fit_boxes_to_points

    S, M, T = sel.sensor_raw.pos.shape[:3]
    dev = sel.age.device
    fit_count = fit = None
    if fit_rot or fit_pos:
        L.require_cuda(clouds, counts)
        assert clouds.dim() == 4 and clouds.shape[:2] == (S, T) and clouds.dtype == torch.float32, (clouds.shape, clouds.dtype)
        assert counts.shape == (S, T), counts.shape
        in_cloud = torch.arange(clouds.shape[2], device=dev).view(1, 1, -1) < counts[..., None]
        parts = [fit_boxes_to_points(clouds[s, t], sel.fit_boxes[s, t], fitting_dims_bloat_factor, point_valid=in_cloud[s, t])
                 for s in range(S) for t in range(T)]
        fit_count = torch.stack([p[0] for p in parts]).view(S, T, M)
        fit = torch.stack([p[1] for p in parts]).view(S, T, M, 5)
    new = _new(dev)
    f32, f64 = torch.float32, torch.float64
    spos, srot, wpos, wrot = new((S, M, T, 3), f64), new((S, M, T, 1), f64), new((S, M, T, 3), f64), new((S, M, T, 1), f64)
    dims, probs, velo = new((S, M, T, 3), f32), new((S, M, T, 1), f32), new((S, M, T, 1), f32)
    if S > 0:
        raw = sel.sensor_raw
        with torch.cuda.device(dev):
            L.check(L.TIMER.launch("refine_tracks_apply", lambda: L.lib().liso_refine_tracks_apply(
                S, T, M, L.ptr(sel.verdict), L.ptr(sel.age), L.ptr(sel.start), L.ptr(sel.median_conf), L.ptr(sel.dist_covered_m),
                L.ptr(sel.refined_dims), L.ptr(raw.pos), L.ptr(raw.rot), L.ptr(raw.dims), L.ptr(tracked.w_T_sensor), opt_ptr(fit_count),
                opt_ptr(fit), int(bool(fit_rot)), int(bool(fit_pos)), float(time_between_frames_s), L.ptr(spos), L.ptr(srot), L.ptr(wpos),
                L.ptr(wrot), L.ptr(dims), L.ptr(probs), L.ptr(velo), L.stream_ptr())), "refine_tracks_apply")
    valid = sel.row_valid()
    return RefinedTracks(Shape(pos=spos, dims=dims, rot=srot, probs=probs, valid=valid),
                         Shape(pos=wpos, dims=dims, rot=wrot, probs=probs, velo=velo, valid=valid), fit_count, fit)


def smoothing_tables(sel: SelectedTracks, ref: RefinedTracks, s):
    """the tables the smoothing of sequence s is given: (pos float32 [M,T,3], yaw float32 [M,T,1], valid bool [M,T]); rows of tracks
    without SMOOTHED and rows behind a track's age are invalid and zero"""
    valid = sel.row_valid(SMOOTHED)[s]
    return (ref.world.pos[s] * valid[..., None]).float(), (ref.world.rot[s] * valid[..., None]).float(), valid


@torch.no_grad()
def smooth_tracks(sel: SelectedTracks, ref: RefinedTracks, *, track_smoothing_method="jerk", time_between_frames_s) -> RefinedTracks:
    """stage 3a (reference :1236-1318): `ref.world` with the positions, headings and per-frame displacements of the smoothers in the rows
    of the SMOOTHED tracks (float32 results widened, as the reference stores them); every other row as it was.  In place on `ref.world`."""
    if track_smoothing_method not in ("jerk", "bike_model", "none"):
        raise NotImplementedError(track_smoothing_method)
    S, M, T = ref.world.pos.shape[:3]
    for s in range(S):
        pos, yaw, valid = smoothing_tables(sel, ref, s)
        if track_smoothing_method == "none" or T <= 4:  # (the reference's "tracks are too short", decided on the static T)
            new_pos, new_yaw, new_velo = pos, yaw, batched_displacement_from_pos(pos)[..., None]
        elif track_smoothing_method == "jerk":
            new_pos, new_yaw, new_velo = smooth_track_jerk(batched_observed_pos_m=pos, batched_observed_yaw_angle_rad=yaw,
                                                           batched_valid_mask=valid, time_between_frames_s=time_between_frames_s)
        else:
            picked = torch.nonzero(valid[:, 0])[:, 0]  # (a read: L-BFGS reads its loss at every step anyway)
            if picked.numel() == 0:
                continue
            with torch.enable_grad():
                part = smooth_track_bike_model(batched_observed_pos_m=pos[picked], batched_observed_yaw_angle_rad=yaw[picked],
                                               batched_valid_mask=valid[picked], batched_vehicle_length_m=sel.refined_dims[s, picked, 0],
                                               time_between_frames_s=time_between_frames_s)
            new_pos, new_yaw, new_velo = pos.clone(), yaw.clone(), torch.zeros_like(yaw)
            new_pos[picked], new_yaw[picked], new_velo[picked] = part[0].detach().float(), part[1].detach().float(), part[2].detach().float()
        v = valid[..., None]
        ref.world.pos[s] = torch.where(v, new_pos.double(), ref.world.pos[s])
        ref.world.rot[s] = torch.where(v, new_yaw.double(), ref.world.rot[s])
        ref.world.velo[s] = torch.where(v, new_velo.float(), ref.world.velo[s])
    return ref


@torch.no_grad()
def export_tracks(sel: SelectedTracks, ref: RefinedTracks, tracked: TrackedSequences, *, cap_out, in_annotated_fov=None,
                  export_only_in_annotated_fov=False) -> MinedTracks:
    """stage 3b (liso_export_tracks): the sensor boxes from the world boxes and the per-frame tables.  `in_annotated_fov` uint8 [S,T,K],
    per detection; it is read through `tracked.src`, so a hole-filling row carries the flag of the detection it was carried from."""
    S, M, T = ref.world.pos.shape[:3]
    K, cap = sel.det_shape
    C, dev = int(cap_out), sel.age.device
    if C < 1:
        raise L.LisoHipError(f"export_tracks: cap_out = {C} refused (>= 1)")
    fov = None
    if export_only_in_annotated_fov:
        assert in_annotated_fov is not None, "export_only_in_annotated_fov needs in_annotated_fov"
        L.require_cuda(in_annotated_fov)
        assert in_annotated_fov.shape == (S, T, K), (in_annotated_fov.shape, (S, T, K))
        fov = in_annotated_fov.to(torch.uint8).contiguous()
    new = _new(dev)
    i32, f32, f64 = torch.int32, torch.float32, torch.float64
    spos, srot = new((S, M, T, 3), f64), new((S, M, T, 1), f64)
    fr = FrameBoxes(new((S, T), i32), new((S, T, C, 3), f64), new((S, T, C, 1), f64), new((S, T, C, 3), f32), new((S, T, C, 1), f32),
                    new((S, T, C, 1), f32), new((S, T, C), torch.int64), new((S, T, C, 4, 4), f64), new((S, T), f32), new((S, T, C), torch.uint8))
    overflow = new((S,), i32)
    w = ref.world
    if S > 0:
        with torch.cuda.device(dev):
            L.check(L.TIMER.launch("export_tracks", lambda: L.lib().liso_export_tracks(
                S, T, K, cap, M, C, L.ptr(sel.verdict), L.ptr(sel.age), L.ptr(sel.start), L.ptr(w.pos), L.ptr(w.rot), L.ptr(w.dims), L.ptr(w.probs),
                L.ptr(w.velo), L.ptr(tracked.w_T_sensor), L.ptr(tracked.src), opt_ptr(fov), int(fov is not None), L.ptr(spos), L.ptr(srot),
                L.ptr(fr.n_boxes), L.ptr(fr.pos), L.ptr(fr.rot), L.ptr(fr.dims), L.ptr(fr.probs), L.ptr(fr.velo), L.ptr(fr.track_id),
                L.ptr(fr.lidar_T_box), L.ptr(fr.max_confidence), L.ptr(fr.valid), L.ptr(overflow), L.ptr(sel.workspace),
                sel.workspace.numel(), L.stream_ptr())), "export_tracks")
    sensor = Shape(pos=spos, dims=w.dims, rot=srot, probs=w.probs, valid=w.valid)
    return MinedTracks(sel.n_tracks, overflow, sel.age, sel.start, sel.median_conf, sel.dist_covered_m, sel.verdict, sel.refined_dims, w, sensor,
                       sel.world_raw, sel.sensor_raw, fr)


@torch.no_grad()
def mine_tracked_sequences(tracked: TrackedSequences, boxes, conf, clouds, counts, *, max_tracks, cap_out, min_track_age,
                           confidence_threshold_mined_boxes, min_track_obj_speed_mps, time_between_frames_s, is_flow_cluster_detector,
                           flow_cluster_detector_min_travel_dist_filter_m, fit_rot, fit_pos, fitting_dims_bloat_factor,
                           min_dist_for_track_smoothing=5.0, use_track_smoothing=True, track_smoothing_method="jerk",
                           in_annotated_fov=None, export_only_in_annotated_fov=False) -> MinedTracks:
    """tracked: the result of `track_sequences`; boxes float32 [S,T,K,7] and conf float32 [S,T,K]: the tensors it was given; clouds float32
    [S,T,N,C] NaN-padded with counts int32 [S,T]; in_annotated_fov uint8 [S,T,K] per detection.  The scalar arguments are the reference's
    configuration entries of the same names (`is_flow_cluster_detector` = isinstance(box_predictor, FlowClusterDetector),
    `use_track_smoothing` = tracker_model_name == "flow_tracker" and flow_tracker.use_track_smoothing).  Nothing is read back."""
    sel = select_tracks(tracked, boxes, conf, max_tracks=max_tracks, min_track_age=min_track_age,
                        confidence_threshold_mined_boxes=confidence_threshold_mined_boxes, min_track_obj_speed_mps=min_track_obj_speed_mps,
                        time_between_frames_s=time_between_frames_s, is_flow_cluster_detector=is_flow_cluster_detector,
                        flow_cluster_detector_min_travel_dist_filter_m=flow_cluster_detector_min_travel_dist_filter_m,
                        min_dist_for_track_smoothing=min_dist_for_track_smoothing, use_track_smoothing=use_track_smoothing)
    ref = refine_tracks(sel, tracked, clouds, counts, fit_rot=fit_rot, fit_pos=fit_pos, fitting_dims_bloat_factor=fitting_dims_bloat_factor,
                        time_between_frames_s=time_between_frames_s)
    if use_track_smoothing:
        ref = smooth_tracks(sel, ref, track_smoothing_method=track_smoothing_method, time_between_frames_s=time_between_frames_s)
    return export_tracks(sel, ref, tracked, cap_out=cap_out, in_annotated_fov=in_annotated_fov,
                         export_only_in_annotated_fov=export_only_in_annotated_fov)
