/*
 * liso_track_mining.h -- C ABI of the stage between the sequence tracker and the databases of a mining round: the loop over
 * get_ids_lengths_of_longest_tracks() inside track_boxes_on_data_sequence (liso/tracker/tracking.py:1099-1328) and the fold of the
 * kept tracks into the per-sample mined-box database (:1521-1681), for n_seq padded sequences per call and without a host read.
 *
 * The inputs are the tables of liso_track_sequences (include/liso_tracking.h: pos_world, rot_world, src, w_T_sensor with `cap` rows
 * per frame), the detections it was given (boxes float32 [S,T,K,7], conf float32 [S,T,K]) and the row table of the tracks:
 *   rows  int64 [S,M,T]   the row of track m + 1 in each frame, -1 where it has none (M = max_tracks; the tracker hands out the ids
 *                         1, 2, ... without gaps, so track i sits at index i - 1).  Entries outside [0, cap) count as -1.
 * A track's rows are taken in frame order; `age` is their number, `start` the first frame that has one, and row k is treated as the
 * row of frame start + k, which is the reference's assumption (:1109-1115; the tracker fills one-frame holes and ends a track that
 * is lost for longer, so its tracks are contiguous).  Hole-filling rows count.  Per-track tables are [S,M], per-track-row tables
 * [S,M,T] with row k of the track at index k; entries of tracks that are not KEPT and behind a track's age are 0.
 *
 * ---- liso_select_tracks: one wavefront per (sequence, track) --------------------------------------------------------------------
 *   age, start    int32 [S,M]
 *   median_conf   float32 [S,M]   torch.median of the rows' confidences: element (age - 1) / 2 of the ascending sort, the lower of two
 *                                 middles, the value itself (bit exact).  Confidences and dims are taken to be finite.
 *   dist          float64 [S,M]   sqrt(dx dx + dy dy) of the last row's world position minus the first row's, fp64, operation by operation
 *   refined_dims  float32 [S,M,3] torch.quantile(dims, q, dim=0), linear: pos = q (age - 1) in fp64, lo = floor(pos), hi = ceil(pos),
 *                                 frac = float(pos - lo), then lo_value + (hi_value - lo_value) * frac in fp32 on the sorted column
 *   verdict       uint8 [S,M]     LISO_MINE_AGE_OK   age >= min_track_age (and age > 0)
 *                                 LISO_MINE_CONF_OK  AGE_OK and median_conf >= conf_threshold (the reference skips on <)
 *                                 LISO_MINE_KEPT     CONF_OK and (min_speed <= 0 or dist / (age * dt) >= min_speed) and
 *                                                    (not is_flow_cluster_detector or dist >= min_travel_dist)
 *                                 LISO_MINE_SMOOTHED KEPT and dist > min_dist_for_smoothing and use_track_smoothing and
 *                                                    age >= LISO_MINE_MIN_TRACK_LEN_FOR_SMOOTHING
 *                                 (median_conf, dist and refined_dims are filled for every track with age > 0)
 *   world_raw_pos float64 [S,M,T,3], world_raw_rot float64 [S,M,T]   the tracker's world boxes of a KEPT track's rows
 *   sensor_raw_pos / sensor_raw_rot                                   inv(w_T_sensor[start + k]) @ pose(world box), translation and
 *                                                                     atan2(R10, R00) (the adjugate inverse of an affine matrix, fp64)
 *   raw_dims float32 [S,M,T,3], raw_probs float32 [S,M,T]             the detection's, through `src`
 *   fit_boxes     float32 [S,T,M,7]  per frame the box list liso_fit_boxes_closeness_f32 takes: entry (t, m) is the sensor box
 *                                 (x, y, z, dx, dy, dz, yaw rounded to fp32) of KEPT track m + 1 in frame t, NaN where it has none
 *                                 (a NaN box holds no point)
 *   workspace     liso_track_mining_workspace_bytes(...) bytes, 8-byte aligned, shared by the three stages (the compacted row
 *                 table); 0 = sizes refused: the selection sorts a track's rows (<= T) in LDS, T <= LISO_MINE_MAX_FRAMES, and the
 *                 export ranks a frame's tracks in LDS, M <= LISO_MINE_MAX_TRACKS
 *
 * ---- liso_refine_tracks_apply: one thread per track row ----------------------------------------------------------------------------
 * perform_local_box_refinement (:2004-2133) and :1163-1224 for every row of a KEPT track.  fit_count int32 [S,T,M] / fit float64
 * [S,T,M,5] are the results of liso_fit_boxes_closeness_f32 on `fit_boxes` (NULL when neither fit_rot nor fit_pos is set).  Where the
 * count is > 0: rot <- rot + (fit yaw - rot) with fit_rot, x, y <- fitted centre with fit_pos.  Then
 * set_box_size_keep_closest_point_constant (:239-260) with the track's refined_dims: of the bottom corners (+,-), (+,+), (-,-), (-,+)
 * -- 0.5f * dims in fp32, through the pose in fp64 -- the one nearest the sensor in x, y (the first on a tie) stays in place:
 * pos <- c + double(refined_dims / dims) * (pos - c).  w_T_box = w_T_sensor[start + k] @ sensor_T_box in fp64 (entries ((a0 b0 + a1 b1) +
 * a2 b2) + a3 b3), world pos its translation, world rot atan2(R10, R00); probs <- median_conf; velo <- float(dist) / (float(age) *
 * float(dt)) in fp32 for KEPT tracks without SMOOTHED, 0 for those with it (the smoothing fills theirs).
 *   sensor_pos, world_pos float64 [S,M,T,3]; sensor_rot, world_rot float64 [S,M,T]; dims float32 [S,M,T,3]; probs, velo float32 [S,M,T]
 *
 * ---- liso_export_tracks: one workgroup per (sequence, frame) -----------------------------------------------------------------------
 * update_sensor_boxes_from_world_boxes (:290-316) for every row of a KEPT track -- sensor_T_box = inv(w_T_sensor[start + k]) @ w_T_box
 * from the (possibly smoothed) world box, dims left alone -- into sensor_pos / sensor_rot [S,M,T,..], and the per-frame tables of the
 * mined-box database (:1613-1681), `cap_out` rows per frame:
 *   a frame's rows are the rows of its KEPT tracks (with fov_only: those whose detection -- in_fov uint8 [S,T,K] through `src`, the
 *   detection a hole-filling row was carried from -- has the flag), first the tracks without SMOOTHED, then those with it, each group
 *   in the order of get_ids_lengths_of_longest_tracks: descending age, EQUAL AGES BY ASCENDING ID (the reference inherits whatever
 *   torch.argsort does with ties).  The rank is a count over the frame's tracks, no atomics: two runs are bitwise equal.
 *   n_boxes int32 [S,T] (at most cap_out); out_pos float64 [S,T,cap_out,3], out_rot float64 [S,T,cap_out]; out_dims float32 [..,3];
 *   out_probs, out_velo float32 [S,T,cap_out]; out_track_id int64 [S,T,cap_out] (-1 behind n_boxes; every row behind n_boxes is blank);
 *   out_lidar_T_box float64 [S,T,cap_out,4,4] the yaw-only pose of (out_pos, out_rot); max_conf float32 [S,T] the largest out_probs of
 *   the frame's written rows, -inf without one; out_valid uint8 [S,T,cap_out]; overflow int32 [S] rows that did not fit cap_out, summed
 *   over the frames (the rows that fit are the first ones in the order above).
 */
#ifndef LISO_TRACK_MINING_H
#define LISO_TRACK_MINING_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LISO_MINE_MAX_FRAMES 1024
#define LISO_MINE_MAX_TRACKS 8192
#define LISO_MINE_AGE_OK 1
#define LISO_MINE_CONF_OK 2
#define LISO_MINE_KEPT 4
#define LISO_MINE_SMOOTHED 8
/* MIN_TRACK_LEN_FOR_SMOOTHING of liso/tracker/track_smoothing.py:35 */
#define LISO_MINE_MIN_TRACK_LEN_FOR_SMOOTHING 4

size_t liso_track_mining_workspace_bytes(int n_seq, int max_frames, int max_det, int cap, int max_tracks);

int liso_select_tracks(int n_seq, int max_frames, int max_det, int cap, int max_tracks, const int64_t* rows, const double* pos_world,
                       const double* rot_world, const int32_t* src, const double* w_T_sensor, const float* boxes, const float* conf,
                       int min_track_age, float conf_threshold, double min_speed, double dt, int is_flow_cluster_detector,
                       double min_travel_dist, double min_dist_for_smoothing, int use_track_smoothing, double dims_quantile,
                       int32_t* age, int32_t* start, float* median_conf, double* dist, uint8_t* verdict, float* refined_dims,
                       double* world_raw_pos, double* world_raw_rot, double* sensor_raw_pos, double* sensor_raw_rot, float* raw_dims,
                       float* raw_probs, float* fit_boxes, void* workspace, size_t workspace_bytes, void* stream);

int liso_refine_tracks_apply(int n_seq, int max_frames, int max_tracks, const uint8_t* verdict, const int32_t* age, const int32_t* start,
                             const float* median_conf, const double* dist, const float* refined_dims, const double* sensor_raw_pos,
                             const double* sensor_raw_rot, const float* raw_dims, const double* w_T_sensor, const int32_t* fit_count,
                             const double* fit, int fit_rot, int fit_pos, double dt, double* sensor_pos, double* sensor_rot,
                             double* world_pos, double* world_rot, float* dims, float* probs, float* velo, void* stream);

int liso_export_tracks(int n_seq, int max_frames, int max_det, int cap, int max_tracks, int cap_out, const uint8_t* verdict,
                       const int32_t* age, const int32_t* start, const double* world_pos, const double* world_rot, const float* dims,
                       const float* probs, const float* velo, const double* w_T_sensor, const int32_t* src, const uint8_t* in_fov,
                       int fov_only, double* sensor_pos, double* sensor_rot, int32_t* n_boxes, double* out_pos, double* out_rot,
                       float* out_dims, float* out_probs, float* out_velo, int64_t* out_track_id, double* out_lidar_T_box,
                       float* max_conf, uint8_t* out_valid, int32_t* overflow, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LISO_TRACK_MINING_H */
