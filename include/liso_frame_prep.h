/*
 * liso_frame_prep.h -- C ABI of the stage between the detector and the sequence tracker: every frame of many padded sequences is
 * turned from post-NMS boxes into the tables liso_track_sequences (include/liso_tracking.h) and liso_export_tracks
 * (include/liso_track_mining.h) take, in at most three launches, without a host read.
 *
 * liso_prepare_tracker_frames replaces the per-frame body of track_boxes_on_data_sequence (liso/tracker/tracking.py:745-1017):
 *   - is_boxes_clearly_in_bev_range                        (liso/kabsch/shape_utils.py:549-560; tracking.py:745-767),
 *   - the min_points_in_box filter on get_points_in_boxes_mask   (tracking.py:769-815; liso/datasets/torch_dataset_commons.py:1902-1935),
 *   - count_box_points_in_kitti_annotated_fov              (liso/eval/eval_ours.py:96-116, on fit_bev_box_z_and_height_using_points_in_box,
 *                                                           liso/networks/flow_cluster_detector/flow_cluster_detector.py:339-384; tracking.py:821-835),
 *   - the two propagate_boxes_forward_using_flow calls     (tracking.py:942-970, 2168-2211),
 *   - soft_align_box_flip_orientation_with_motion_trafo    (shape_utils.py:608-644, with extract_motion_in_pred_box_coordinates :563-580
 *                                                           and extract_box_motion_transform_without_sensor_odometry :583-605; tracking.py:972-979),
 *   - drop_padding_boxes after each filter                 (shape_utils.py:243-269) and the padding of FlowBasedBoxTracker's frame lists.
 *
 * Inputs (S sequences of up to T frames, P box slots, N point rows per frame):
 *   n_frames     int32   [S]          frames of each sequence (clamped to [0, T])
 *   n_box        int32   [S,T]        post-NMS boxes of each frame (clamped to [0, P])
 *   boxes        float32 [S,T,P,7]    x, y, z, dx, dy, dz, yaw in sensor coordinates (the dense layout of include/liso_iou3d.h)
 *   conf         float32 [S,T,P]
 *   odom         float64 [S,T,4,4]    sensor(t) <- sensor(t + 1) (odom_ta_tb); read for every frame when `align` is set
 *   clouds       float32 [S,T,N,point_stride]   x, y, z first (pcl_ta: ground removed); counts int32 [S,T] valid rows (clamped to [0, N])
 *   point_valid  uint8   [S,T,N]      gates a point's flow, not its count (tracking.py:2181-2185)
 *   flow         float32 [S,T,N,3]
 *   fov_clouds   float32 [S,T,n_fov_points,fov_stride] or NULL (then n_fov_points < 0); fov_counts int32 [S,T]   (pcl_full_ta)
 * Rows at or behind n_box, counts, fov_counts and n_frames are never read.
 *
 * Per box, in this order and with this arithmetic:
 *   1. BEV boundary (drop_on_bev_boundaries): kept when |(|x| - dx / 2)| < bev_range_x / 2 and |(|y| - dx / 2)| < bev_range_y / 2, fp32 -- dx on both
 *      axes, as the reference has it.
 *   2. Point count (min_points_in_box > 0): points of `clouds` inside by `precision 0` of liso_points_in_boxes_f32 (fp64 product rounded
 *      to fp32, strict comparison); kept when count >= min_points_in_box.
 *   3. Annotated field of view (fov_clouds given): points of fov_clouds with atan2f(y, x) in [(float)(-41.95 / 180 * pi),
 *      (float)(40.16 / 180 * pi)] inside the box's own three dims by the same test; in_fov = count >= fov_min_points.  Without
 *      fov_clouds in_fov is 1 (tracking.py:817).  A flag: it never drops a box.
 *   4. Mean flow: inside by `precision 1` (fp32 inverse and product); sum of the flow of the points inside that are point_valid, in the
 *      2^-24 m int64 fixed point of liso_points_in_boxes_f32, divided by max(number inside, 1): bitwise that call's mean_flow and count.
 *   5. into_next = F(+mean) P, into_prev = F(-mean) P in fp64: P the yaw-only pose of Shape.get_poses (shape_utils.py:271-319), F the
 *      identity with the mean flow, converted to fp64, in its translation column.
 *   6. Alignment (align): b0_dT_b1 = inv(P) odom into_next; (bx, by) its translation, each entry ((a0 b0 + a1 b1) + a2 b2) + a3 in fp64
 *      and inv(P) in closed form; displacement = sqrt(bx bx + by by); flip = bx < 0 and displacement > no_align_below_m; a flipped box
 *      has yaw + (float)pi in fp32 and (bx, by) negated; ratio = clip((displacement - no_align_below_m) / (full_align_above_m -
 *      no_align_below_m), 0, 1); rot = (double)yaw + ratio * atan2(by, bx); velo = (displacement, 0, 0).  The poses of step 5 are those
 *      of the box before it is turned.  Without `align`, rot = (double)yaw and velo = 0.
 *   7. The boxes that passed 1 and 2 are written in their input order into the first rows of the frame (a stable compaction).
 *
 * Outputs, `cap` rows per frame; rows at or behind n_det and frames at or behind n_frames are zero, their src -1:
 *   n_det        int32   [S,T]          min(boxes kept, cap)
 *   out_boxes    float32 [S,T,cap,7]    the input row with column 6 = (float)rot
 *   rot          float64 [S,T,cap]
 *   out_conf     float32 [S,T,cap]
 *   velo         float64 [S,T,cap,3]
 *   into_prev, into_next  float64 [S,T,cap,4,4]
 *   in_fov       uint8   [S,T,cap]
 *   src          int32   [S,T,cap]      input slot of the row
 *   n_points     int32   [S,T,cap]      the count of step 4
 *   mean_flow    float32 [S,T,cap,3]
 *   dropped_bev, dropped_points  int32 [S,T]   boxes that failed step 1; boxes that passed step 1 and failed step 2
 *   overflow     int32   [S]            sum over the frames of max(0, boxes kept - cap): counted, never written
 *
 * Launches: one pass over `clouds` (grid = point chunks x tiles of 128 boxes x frames; the tile's boxes in LDS, both inside tests per
 * (point, box), counts per wavefront and flow sums per point into LDS integer atomics), the same pass over `fov_clouds` when given, and
 * one block per frame for steps 1 and 5-7.  A block of the passes stores the sums of its chunk of LISO_FRAME_PREP_CHUNK points, and the
 * last launch adds the chunks: integer sums, so the result does not depend on the order of blocks or points.  No table is accumulated
 * across blocks except `overflow`, which the first launch clears: the call needs no memset and no zeroed workspace.
 *
 *   workspace  liso_frame_prep_workspace_bytes(cfg) bytes, 256-byte aligned.  0 = sizes refused: max_box outside [1, LISO_FRAME_PREP_MAX_BOX],
 *              max_frames < 1, cap < 1, n_seq < 0, n_seq * max_frames > 65535, n_points < 0, a stride < 3.  n_seq = 0 is fine: nothing is launched.
 */
#ifndef LISO_FRAME_PREP_H
#define LISO_FRAME_PREP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LISO_FRAME_PREP_MAX_BOX 1024
#define LISO_FRAME_PREP_CHUNK 2048

typedef struct {
    int n_seq, max_frames, max_box, cap;   /* S, T, P, rows per frame of the result */
    long n_points;                         /* N */
    int point_stride;                      /* floats per row of clouds, >= 3 */
    long n_fov_points;                     /* rows per frame of fov_clouds; < 0: no field-of-view cloud */
    int fov_stride;                        /* floats per row of fov_clouds, >= 3 (ignored without one) */
    float bev_range_x, bev_range_y;        /* bev_range_m */
    int drop_on_bev_boundaries;            /* step 1 on / off */
    int min_points_in_box;                 /* step 2; <= 0: off */
    int fov_min_points;                    /* step 3 */
    int align;                             /* step 6 on / off */
    double no_align_below_m, full_align_above_m;
} liso_frame_prep_cfg;

size_t liso_frame_prep_workspace_bytes(const liso_frame_prep_cfg* cfg);

int liso_prepare_tracker_frames(const liso_frame_prep_cfg* cfg, const int32_t* n_frames, const int32_t* n_box, const float* boxes,
                                const float* conf, const double* odom, const float* clouds, const int32_t* counts,
                                const uint8_t* point_valid, const float* flow, const float* fov_clouds, const int32_t* fov_counts,
                                int32_t* n_det, float* out_boxes, double* rot, float* out_conf, double* velo, double* into_prev,
                                double* into_next, uint8_t* in_fov, int32_t* src, int32_t* n_points, float* mean_flow,
                                int32_t* dropped_bev, int32_t* dropped_points, int32_t* overflow, void* workspace,
                                size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LISO_FRAME_PREP_H */
