"""The sequence tracker on the device (include/liso_tracking.h: liso_track_sequences, csrc/track_assoc.hip): what
`FlowBasedBoxTracker.run_tracker` (liso_amd/tracker/global_box_tracker.py, mirror of liso/tracker/global_box_tracker.py:13-514) does
for one sequence on the host, for a padded batch of sequences in one call, without a copy to the host.

* `track_sequences`        the batched call on device tensors -> `TrackedSequences` (no synchronisation, graph-capturable)
* `track_sequences_host`   the same contract in numpy with fp64 distances: the yardstick of the device tests
* `DeviceFlowBasedBoxTracker`  constructor, `update`, `run_tracker` and getters of `FlowBasedBoxTracker` for one sequence

The order in which tracks of equal confidence are served is stated here -- ascending row index -- where the host class inherits
whatever `torch.argsort` does with ties; `FlowBasedBoxTracker(tie_order="stable")` follows the same rule.
"""
import dataclasses
from typing import Dict, List

import numpy as np
import torch

from liso_amd import _lib as L
from liso_amd.kabsch.shape_utils import Shape
from liso_amd.tracker.global_box_tracker import INITIAL_TRACK_CONF, MAX_PROPAGATION_TIME, MIN_ALIVE_TRACK_CONF

MAX_CAP = 1024  # LISO_TRACK_MAX_CAP


# ---- host restatement ------------------------------------------------------------------------------------------------------------
def _walk_host(pos, prop_xy, frames, counter, threshold, cap, margin=None):
    """track_one_way over `frames` (indices into pos / prop_xy) -> (rows per visited frame, counter, rows that did not fit).  A frame's
    rows: dict of pos [m,3] f64, ids, conf f32, src [m,2], with the detections first.  With `margin`, every visited row asserts that
    fp32 rounding cannot decide for it: none of its distances lies within `margin` of the threshold, and no two of those below
    threshold + margin within `margin` of each other."""
    out, over = [], 0
    for f, t in enumerate(frames):
        n = min(len(pos[t]), cap)
        cur_pos, ids = pos[t][:n].copy(), np.full(n, -1, np.int64)
        src = np.stack([np.full(n, t), np.arange(n)], axis=1).astype(np.int32)
        lost_pos, lost_ids, lost_conf, lost_src = np.zeros((0, 3)), np.zeros(0, np.int64), np.zeros(0, np.float32), np.zeros((0, 2), np.int32)
        if f == 0:
            ids[:] = counter + 1 + np.arange(n)
            counter += n
        else:
            prev = out[-1]
            alive = prev["conf"] >= np.float32(MIN_ALIVE_TRACK_CONF)
            order = [i for i in np.argsort(-prev["conf"], kind="stable") if alive[i]]  # descending, equal ones by ascending row
            a = prev["pos"][:, :2].astype(np.float32).astype(np.float64)
            b = prop_xy[t][:n].astype(np.float32).astype(np.float64)
            matched = np.zeros(len(alive), bool)
            for i in order:
                if margin is not None:
                    d_all = np.sqrt(((b - a[i]) ** 2).sum(axis=1))
                    assert (np.abs(d_all - threshold) > margin).all(), ("a distance within the margin of the threshold", t, i)
                    assert (np.diff(np.sort(d_all[d_all < threshold + margin])) > margin).all(), ("two candidates within the margin", t, i)
                free = np.where(ids < 0)[0]
                if len(free) == 0:
                    break
                d = np.sqrt(((b[free] - a[i]) ** 2).sum(axis=1))
                if d.min() < threshold:
                    ids[free[np.argmin(d)]], matched[i] = prev["ids"][i], True  # argmin: the first detection on a tie
            born = ids < 0
            ids[born] = counter + 1 + np.arange(born.sum())
            counter += int(born.sum())
            lost = np.where(alive & ~matched)[0]
            lost_pos = prev["pos"][lost].copy()
            if f >= 2:
                for j, i in enumerate(lost):
                    before = np.where(out[-2]["ids"] == prev["ids"][i])[0]
                    if len(before):
                        lost_pos[j] = lost_pos[j] + (lost_pos[j] - out[-2]["pos"][before[0]])
            lost_ids, lost_src = prev["ids"][lost], prev["src"][lost]
            lost_conf = (np.float32(0.0001) + prev["conf"][lost]) - np.float32(INITIAL_TRACK_CONF / MAX_PROPAGATION_TIME)
        over += max(0, len(pos[t]) + len(lost_ids) - cap)
        room = cap - n
        out.append({"pos": np.concatenate([cur_pos, lost_pos[:room]]), "ids": np.concatenate([ids, lost_ids[:room]]),
                    "conf": np.concatenate([np.full(n, INITIAL_TRACK_CONF, np.float32), lost_conf[:room]]),
                    "src": np.concatenate([src, lost_src[:room]]), "n_det": n})
    return out, counter, over


def track_sequences_host(n_frames, n_det, boxes, conf, odom, into_prev, into_next, threshold, cap, margin=None):
    """numpy arrays shaped like the arguments of `track_sequences` -> dict of numpy arrays named like the fields of
    `TrackedSequences` (n_out, track_ids, pos_world, rot_world, src, is_fill, w_T_sensor, id_counter, overflow).  Distances are fp64
    on the positions rounded to fp32; `margin`: see `_walk_host`."""
    boxes, odom = np.asarray(boxes, np.float32), np.asarray(odom, np.float64)
    S, T, K = boxes.shape[:3]
    res = {"n_out": np.zeros((S, T), np.int32), "track_ids": np.full((S, T, cap), -1, np.int64), "pos_world": np.zeros((S, T, cap, 3)),
           "rot_world": np.zeros((S, T, cap)), "src": np.full((S, T, cap, 2), -1, np.int32), "is_fill": np.zeros((S, T, cap), np.uint8),
           "w_T_sensor": np.tile(np.eye(4), (S, T, 1, 1)), "id_counter": np.zeros(S, np.int64), "overflow": np.zeros(S, np.int32)}
    for s in range(S):
        nf = int(np.clip(n_frames[s], 0, T))
        W = res["w_T_sensor"][s]
        for t in range(1, nf):
            W[t] = W[t - 1] @ odom[s, t - 1]
        pos, rot, past, future = [], [], [], []
        for t in range(nf):
            n = int(np.clip(n_det[s][t], 0, K))
            b = boxes[s, t, :n].astype(np.float64)
            pos.append(b[:, :3] @ W[t][:3, :3].T + W[t][:3, 3])
            c, sn = np.cos(b[:, 6]), np.sin(b[:, 6])
            rot.append(np.arctan2(W[t][1, 0] * c + W[t][1, 1] * sn, W[t][0, 0] * c + W[t][0, 1] * sn))
            past.append((W[max(t - 1, 0)] @ np.asarray(into_prev[s][t][:n], np.float64))[:, :2, 3].reshape(n, 2))
            future.append((W[min(t + 1, nf - 1)] @ np.asarray(into_next[s][t][:n], np.float64))[:, :2, 3].reshape(n, 2))
        # the walk has room for 3 K rows per frame, which always suffice (`needed_capacity`), up to the kernel's LDS limit; `cap` only
        # limits the rows that are written out
        state_rows = min((MAX_PROPAGATION_TIME + 2) * K, MAX_CAP)
        fwd, counter, res["overflow"][s] = _walk_host(pos, past, list(range(nf)), 0, threshold, state_rows, margin)
        _, counter, _ = _walk_host(pos, future, list(range(nf))[::-1], counter, threshold, state_rows, margin)
        res["id_counter"][s] = counter
        rows = [{k: v[:fr["n_det"]] for k, v in fr.items() if k != "n_det"} for fr in fwd]  # a frame's result: its detections ...
        fill = [np.zeros(fr["n_det"], np.uint8) for fr in fwd]
        for track_id in (np.unique(np.concatenate([fr["ids"] for fr in fwd])) if nf else []):  # ... plus the holes of its tracks
            seen = np.array([bool((fr["ids"][:fr["n_det"]] == track_id).any()) for fr in fwd])
            first, last = int(np.argmax(seen)), nf - 1 - int(np.argmax(seen[::-1]))
            if last - first < 2:
                continue
            for t in first + np.where(~seen[first:last])[0]:
                where = np.where(fwd[t]["ids"] == track_id)[0]
                rows[t] = {k: np.concatenate([v, fwd[t][k][where]]) for k, v in rows[t].items()}
                fill[t] = np.concatenate([fill[t], np.ones(len(where), np.uint8)])
        for t in range(nf):
            m = min(len(rows[t]["ids"]), cap)
            res["overflow"][s] += len(rows[t]["ids"]) - m
            rows[t], fill[t] = {k: v[:m] for k, v in rows[t].items()}, fill[t][:m]
            res["n_out"][s, t] = m
            res["track_ids"][s, t, :m], res["pos_world"][s, t, :m], res["src"][s, t, :m] = rows[t]["ids"], rows[t]["pos"], rows[t]["src"]
            res["is_fill"][s, t, :m] = fill[t]
            res["rot_world"][s, t, :m] = [rot[a][k] for a, k in rows[t]["src"]]
    return res


# ---- device ------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class TrackedSequences:
    """the result tables of `track_sequences` (include/liso_tracking.h), device tensors; `boxes`: Shape [S,T,cap] in world coordinates,
    dims / probs gathered through `src`, valid = row < n_out"""
    n_out: torch.Tensor
    track_ids: torch.Tensor
    pos_world: torch.Tensor
    rot_world: torch.Tensor
    src: torch.Tensor
    is_fill: torch.Tensor
    w_T_sensor: torch.Tensor
    id_counter: torch.Tensor
    overflow: torch.Tensor
    boxes: Shape

    def track_table(self, max_tracks):
        """-> (ids int64 [S,max_tracks] ascending, -1 behind a sequence's tracks; lengths int64 [S,max_tracks]; rows int64
        [S,max_tracks,T]: the row of the track in each frame, -1 where it has none; n_tracks int64 [S]: the tracks the sequence has,
        which the caller compares to max_tracks).  The forward walk hands out the ids 1, 2, ... without gaps, each to a detection, so
        track i sits at index i - 1.  Device operations only."""
        S, T, cap = self.track_ids.shape
        ids = self.track_ids
        fits = (ids >= 1) & (ids <= max_tracks)
        slot = torch.where(fits, ids - 1, max_tracks)  # (rows without a slot go to a spare line)
        rows = torch.full((S, max_tracks + 1, T), -1, dtype=torch.long, device=ids.device)
        frame = torch.arange(T, device=ids.device).view(1, T, 1).expand(S, T, cap)
        row = torch.arange(cap, device=ids.device).view(1, 1, cap).expand(S, T, cap)
        rows.view(S, -1).scatter_(1, (slot * T + frame).reshape(S, -1), row.reshape(S, -1))
        rows = rows[:, :max_tracks]
        lengths = (rows >= 0).sum(dim=-1)
        names = torch.arange(1, max_tracks + 1, device=ids.device).expand(S, max_tracks)
        return torch.where(lengths > 0, names, -1), lengths, rows, ids.amax(dim=(1, 2)).clamp(min=0)

    def observed_for_smoothing(self, max_tracks):
        """-> (pos [S,max_tracks,T,3], yaw [S,max_tracks,T,1], valid bool [S,max_tracks,T], start int64 [S,max_tracks]): every track
        from its first frame on (column 0 = frame `start`), as smooth_track_jerk / smooth_track_bike_model take them once the two
        leading axes are flattened; padding is 0 / False.  Device operations only."""
        _, _, rows, _ = self.track_table(max_tracks)
        S, M, T = rows.shape
        present = rows >= 0
        start = torch.where(present.any(dim=-1), present.long().argmax(dim=-1), 0)
        frame = torch.arange(T, device=rows.device).view(1, 1, T) + start[..., None]
        inside = frame < T
        frame = frame.clamp(max=T - 1)
        row = rows.gather(2, frame)
        valid = inside & (row >= 0)
        flat = (frame * self.track_ids.shape[2] + row.clamp(min=0)).reshape(S, -1)
        pos = self.pos_world.reshape(S, -1, 3).gather(1, flat[..., None].expand(-1, -1, 3)).view(S, M, T, 3)
        yaw = self.rot_world.reshape(S, -1).gather(1, flat).view(S, M, T, 1)
        return pos * valid[..., None], yaw * valid[..., None], valid, start


@torch.no_grad()
def track_sequences(n_frames, n_det, boxes, conf, odom, into_prev, into_next, threshold, cap) -> TrackedSequences:
    """n_frames int32 [S], n_det int32 [S,T], boxes float32 [S,T,K,7], conf float32 [S,T,K], odom float64 [S,T,4,4], into_prev /
    into_next float64 [S,T,K,4,4] (device tensors, include/liso_tracking.h), threshold = box_matching_threshold_m, cap = rows per
    frame of the result (the walk has its own room: a small cap shortens the tables, never changes the tracks).  Nothing is read back:
    the caller looks at `overflow` when it wants to know whether `cap` was enough."""
    L.require_cuda(n_frames, n_det, boxes, conf, odom, into_prev, into_next)
    S, T, K = boxes.shape[:3]
    assert boxes.shape == (S, T, K, 7) and boxes.dtype == torch.float32, (boxes.shape, boxes.dtype)
    assert conf.shape == (S, T, K) and conf.dtype == torch.float32, (conf.shape, conf.dtype)
    assert n_frames.shape == (S,) and n_det.shape == (S, T) and n_frames.dtype == n_det.dtype == torch.int32
    assert odom.shape == (S, T, 4, 4) and odom.dtype == torch.float64, (odom.shape, odom.dtype)
    for m in (into_prev, into_next):
        assert m.shape == (S, T, K, 4, 4) and m.dtype == torch.float64, (m.shape, m.dtype)
    n_frames, n_det, boxes, conf, odom, into_prev, into_next = (v.contiguous() for v in (n_frames, n_det, boxes, conf, odom, into_prev,
                                                                                          into_next))
    cap = int(cap)
    ws_bytes = int(L.lib().liso_track_sequences_workspace_bytes(S, T, K, cap))
    if ws_bytes == 0:
        raise L.LisoHipError(f"track_sequences: sizes refused (S={S}, T={T}, K={K}, cap={cap}; 1 <= cap <= {MAX_CAP}, T, K >= 1)")
    dev = boxes.device
    new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)  # noqa: E731
    n_out, ids, pos, rot = new((S, T), torch.int32), new((S, T, cap), torch.int64), new((S, T, cap, 3), torch.float64), new((S, T, cap), torch.float64)
    src, fill, w_T = new((S, T, cap, 2), torch.int32), new((S, T, cap), torch.uint8), new((S, T, 4, 4), torch.float64)
    counter, overflow = new((S,), torch.int64), new((S,), torch.int32)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    if S > 0:
        with torch.cuda.device(dev):
            L.check(L.TIMER.launch("track_sequences", lambda: L.lib().liso_track_sequences(
                S, T, K, cap, L.ptr(n_frames), L.ptr(n_det), L.ptr(boxes), L.ptr(conf), L.ptr(odom), L.ptr(into_prev), L.ptr(into_next),
                float(threshold), L.ptr(n_out), L.ptr(ids), L.ptr(pos), L.ptr(rot), L.ptr(src), L.ptr(fill), L.ptr(w_T), L.ptr(counter),
                L.ptr(overflow), L.ptr(ws), ws_bytes, L.stream_ptr())), "track_sequences")
    flat = (src[..., 0].long() * K + src[..., 1].long()).clamp(min=0).view(S, T * cap)
    valid = torch.arange(cap, device=dev).view(1, 1, cap) < n_out[..., None]
    dims = boxes.view(S, T * K, 7)[..., 3:6].gather(1, flat[..., None].expand(-1, -1, 3)).view(S, T, cap, 3)
    probs = conf.view(S, T * K).gather(1, flat).view(S, T, cap, 1)
    shape = Shape(pos=pos, dims=dims * valid[..., None], rot=rot[..., None], probs=probs * valid[..., None], valid=valid)
    return TrackedSequences(n_out, ids, pos, rot, src, fill, w_T, counter, overflow, shape)


def _pad_frames(parts, K):
    """per-frame tensors [n_t, ...] -> [T, K, ...], zeros behind a frame's rows"""
    spare = parts[0].new_zeros((K,) + tuple(parts[0].shape[1:]))
    return torch.nn.utils.rnn.pad_sequence(list(parts) + [spare], batch_first=True)[:len(parts)]


def needed_capacity(n_per_frame):
    """rows per frame that always suffice: a frame holds its detections and the carried boxes of the previous frame's alive rows, which
    are that frame's detections and the detections of earlier frames carried at most MAX_PROPAGATION_TIME times"""
    back = MAX_PROPAGATION_TIME + 1  # (a box is carried at most that many times)
    n = [0] * back + [int(v) for v in n_per_frame]
    return max([1] + [sum(n[i - back:i + 1]) for i in range(back, len(n))])


class DeviceFlowBasedBoxTracker:
    """`FlowBasedBoxTracker` for one sequence with the frames kept on the device: `update` stores device tensors, `run_tracker` pads them
    and makes one `track_sequences` call, the getters return the host class's structures (tensors on the device) and cost one read of
    n_out / overflow / id counter / track ids at the first getter call.  `capacity`: rows per frame; None = `needed_capacity` of the frames,
    which cannot overflow, limited to the kernel's maximum."""

    def __init__(self, use_propagated_boxes=False, box_matching_threshold_m=5.0, association_strategy="ours", capacity=None) -> None:
        assert association_strategy in ("ours",)
        if not use_propagated_boxes:
            raise ValueError("DeviceFlowBasedBoxTracker needs use_propagated_boxes=True: the tracker associates a frame's detections by "
                             "their poses propagated into the previous frame (FlowBasedBoxTracker cannot run without them either)")
        self.use_propagated_boxes = use_propagated_boxes
        self.box_matching_threshold = box_matching_threshold_m
        self.association_strategy = association_strategy
        self.capacity = capacity
        self.boxes_sensor_ti, self.sti_T_stii, self.per_box_extra_attributes_dict = [], [], []
        self.propagated_box_poses_to_sensor_ti, self.propagated_box_poses_to_sensor_tiii = [], []
        self.max_track_id_counter = 0
        self.has_tracked = False
        self.result = None
        self._host = None

    def update(self, boxes_tii_s: Shape, predicted_box_poses_stiii, predicted_box_poses_sti, odom_stii_stiii: torch.Tensor,
               per_box_extra_attributes_tii: List[Dict[str, str]] = None):
        assert len(boxes_tii_s.pos.shape) == 2, ("batching not supported", boxes_tii_s.pos.shape)
        assert len(odom_stii_stiii.shape) == 2, ("batching not supported", odom_stii_stiii.shape)
        L.require_cuda(boxes_tii_s.pos, odom_stii_stiii)
        self.boxes_sensor_ti.append(boxes_tii_s.detach())
        self.sti_T_stii.append(odom_stii_stiii.detach())
        n = int(boxes_tii_s.valid.shape[0])  # (no attributes: one None per detection, as the host class substitutes)
        self.per_box_extra_attributes_dict.append(per_box_extra_attributes_tii if per_box_extra_attributes_tii is not None else [None] * n)
        self.propagated_box_poses_to_sensor_ti.append(predicted_box_poses_sti.detach())
        self.propagated_box_poses_to_sensor_tiii.append(predicted_box_poses_stiii.detach())

    def run_tracker(self):
        frames = self.boxes_sensor_ti
        T = len(frames)
        if T == 0:
            raise ValueError("DeviceFlowBasedBoxTracker.run_tracker: no frame was given to update()")
        counts = [int(b.valid.shape[0]) for b in frames]
        K = max(1, max(counts))
        self._cap = int(self.capacity) if self.capacity is not None else min(MAX_CAP, needed_capacity(counts))
        self._counts, self._K = counts, K
        # every attribute padded to [T,K,..]: the tracker reads position, size and heading; the getters gather the others through `src`
        self._padded = {k: _pad_frames([getattr(b, k) for b in frames], K) for k in ("pos", "dims", "rot", "probs", "velo", "class_id", "difficulty")}
        pd = self._padded
        dev = pd["pos"].device
        boxes = torch.cat([pd["pos"].float(), pd["dims"].float(), pd["rot"][..., :1].float()], dim=-1)[None]
        into_prev = _pad_frames([p.double().reshape(-1, 4, 4) for p in self.propagated_box_poses_to_sensor_ti], K)[None]
        into_next = _pad_frames([p.double().reshape(-1, 4, 4) for p in self.propagated_box_poses_to_sensor_tiii], K)[None]
        odom = torch.stack([o.double() for o in self.sti_T_stii])[None]
        n_frames = torch.tensor([T], dtype=torch.int32).to(dev, non_blocking=True)
        n_det = torch.tensor([counts], dtype=torch.int32).to(dev, non_blocking=True)
        self.result = track_sequences(n_frames, n_det, boxes, pd["probs"][..., 0].float()[None], odom, into_prev, into_next,
                                      self.box_matching_threshold, self._cap)
        self.w_Ts_sti = self.result.w_T_sensor[0]
        self._host = None
        self.has_tracked = True

    # ---- getters: the host class's structures -------------------------------------------------------------------------------------
    def _read(self):
        assert self.has_tracked, "need to run tracking first"
        if self._host is None:
            r = self.result
            T = r.n_out.shape[1]  # one blocking copy: row counts, overflow, id counter and the track ids
            host = torch.cat([r.n_out[0].long(), r.overflow[:1].long(), r.id_counter[:1], r.track_ids[0].reshape(-1)]).cpu()
            n_out, over, counter, ids = host[:T], int(host[T]), int(host[T + 1]), host[T + 2:].view(T, -1).numpy()
            if over > 0:
                raise L.LisoHipError(f"DeviceFlowBasedBoxTracker: {over} rows did not fit into capacity {self._cap}; "
                                     f"capacity {needed_capacity(self._counts)} always suffices for this sequence")
            n = [int(v) for v in n_out]
            self.max_track_id_counter = counter
            self.track_ids = [r.track_ids[0, t, :n[t]] for t in range(len(n))]
            self.boxes_world_ti = [self._frame(t, n[t]) for t in range(len(n))]
            # the host class lists per frame the attributes of its detections and then those of EVERY box the forward walk carried
            # into the frame, hole-filling or not: the alive rows of the frame before (detections, or boxes carried at most
            # MAX_PROPAGATION_TIME times) whose track has no detection here, in row order
            attrs = self.per_box_extra_attributes_dict
            state, self._attrs = [], []
            for t in range(len(n)):
                here = [(int(ids[t, k]), (t, k), 0) for k in range(self._counts[t])]
                taken = {i for i, _, _ in here}
                state = here + [(i, at, c + 1) for i, at, c in state if c <= MAX_PROPAGATION_TIME and i not in taken]
                self._attrs.append([attrs[a][k] for _, (a, k), _ in state])
            self._host = n
        return self._host

    def _frame(self, t, n):
        """frame t of the result as a Shape [n]: position and heading from the tracker (world coordinates), every other attribute
        that of the source detection"""
        r = self.result
        flat = r.src[0, t, :n, 0].long() * self._K + r.src[0, t, :n, 1].long()
        rest = {k: v.reshape((-1,) + tuple(v.shape[2:]))[flat] for k, v in self._padded.items() if k not in ("pos", "rot")}
        return Shape(pos=r.pos_world[0, t, :n].clone(), rot=r.rot_world[0, t, :n, None].clone(),
                     valid=torch.ones(n, dtype=torch.bool, device=flat.device), **rest)

    def get_boxes_in_world_coordinates(self):
        self._read()
        return self.boxes_world_ti

    def get_boxes_in_sensor_coordinates_at_each_timestamp(self):
        self._read()
        return [bw.clone().transform(torch.linalg.inv(w_T_s)) for bw, w_T_s in zip(self.boxes_world_ti, self.w_Ts_sti)]

    def get_extra_attributes_at_each_timestamp(self):
        self._read()
        return self._attrs

    def get_all_unique_track_ids_and_lengths(self):
        self._read()
        return torch.unique(torch.concat(self.track_ids, dim=0), return_counts=True)

    def get_min_max_track_id(self):
        ids, _ = self.get_all_unique_track_ids_and_lengths()
        if ids.size()[0] > 0:
            return ids.min(), ids.max()
        return torch.tensor(0).to(ids.device), torch.tensor(0).to(ids.device)

    def get_ids_lengths_of_longest_tracks(self):
        ids, lens = self.get_all_unique_track_ids_and_lengths()
        order = torch.argsort(lens, descending=True, stable=True)
        return ids[order], lens[order]

    def get_box_indices_start_time_for_track_id(self, track_id):
        self._read()
        padded = torch.nn.utils.rnn.pad_sequence(self.track_ids, batch_first=True, padding_value=-1)
        timestamps, box_idxs = torch.where(padded == track_id)
        return box_idxs, timestamps[0]
