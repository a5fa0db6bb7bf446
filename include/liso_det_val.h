/*
 * liso_det_val.h -- C ABI of the detector's validation matching on the device: every frame of a padded batch against every
 * metric set of the validation pass, with no host synchronisation (graph-capturable).
 *
 * Replaces, per frame and per metric collection, what the reference's run_val (liso/eval/eval_ours.py:404-519) does through
 * ObjectDetectionMetrics.update (liso/eval/od_metrics.py:250-545): filter both box sets (BEV area :125-137, radial range
 * :139-150, class :152-158), build the pair matrix (liso/utils/nms_iou.py:124-207, torch.cdist), walk the predictions by
 * descending confidence and give each one the best free ground-truth box (box_groundtruth_matching_iou.py:28-68,
 * box_groundtruth_matching.py:193-229), and sum the true-positive errors (:489-545).  The precision / recall sweep stays on
 * the host (liso_amd/eval/od_metrics.py says why).
 *
 * Launches of this library's kernels per validation batch, whatever the number of frames F and of jobs J: at most THREE, and a
 * FOURTH only when Waymo-style collections (WaymoObjectDetectionMetrics, liso/eval/od_metrics.py:1397-1835) were asked for --
 *   (1) liso_det_val_pairs_f32        the [P,G] pair matrices of every frame
 *   (2) liso_det_val_transfer_classes run_val's class transfer (:406-447), a launch of its own BEFORE the jobs: the class
 *                                     filtered jobs of (3) read the classes it wrote (the alternative, every class job
 *                                     repeating the transfer walk, was not chosen)
 *   (3) liso_det_val_match_f32        all (job, frame) cells
 *   (4) liso_det_val_assign_f32       all (job, frame) cells of the optimal-assignment jobs (a job table of their own)
 *
 * Conventions (as include/liso_iou3d.h): device pointers, no allocation, no host synchronisation; every entry point checks
 * its arguments before it launches anything and returns LISO_OK, LISO_EINVAL or LISO_ELAUNCH.
 *
 * Inputs: a padded batch of F frames (F >= 0; F == 0 launches nothing).
 *   gt   fp32 [F,G,7] rows (x,y,z,dx,dy,dz,heading), gt_valid   uint8 [F,G], gt_class   int32 [F,G]
 *   pred fp32 [F,P,7],                               pred_valid uint8 [F,P], pred_class int32 [F,P]
 *   order int32 [F,P]: every frame's prediction slots, most confident first -- liso_det_nms_order's sorted_idx (stable:
 *        equal scores keep ascending slot index).  Entries outside [0,P) and slots that are not valid are skipped.
 *   0 <= G, P <= LISO_DET_VAL_MAX_BOXES.  Holes in the valid masks are allowed; what invalid slots hold is never used.
 *   Every index the kernels emit is a SLOT index.  (The ground truth's `moving` flags and the predictions' scores are not
 *   read by any kernel: the host book-keeping uses them.)
 */
#ifndef LISO_DET_VAL_H
#define LISO_DET_VAL_H

#include <stddef.h>
#include <stdint.h>

#include "liso_iou3d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LISO_DET_VAL_MAX_BOXES 1024 /* largest G and P: the bounds of predict_boxes */

#define LISO_DET_VAL_IOU_BEV 0
#define LISO_DET_VAL_IOU_3D 1
#define LISO_DET_VAL_DIST 2

/* A filter set.  A box (x, y) with class c belongs to it iff it is valid and
 *   use_area  == 0 or (area_min_x <= x && x <= area_max_x && area_min_y <= y && y <= area_max_y)      (inclusive)
 *   use_range == 0 or (range_min <= r && r < range_max) with r = sqrtf(x*x + y*y) in fp32
 *   class_id  <  0 or c == class_id
 * (a NaN coordinate fails every comparison of a part that is switched on). */
typedef struct {
    float area_min_x, area_min_y, area_max_x, area_max_y;
    float range_min, range_max;
    int32_t use_area, use_range, class_id;
} liso_det_val_filter;

/* A job: filter set `filter` (index into the filter table), criterion LISO_DET_VAL_*, threshold. */
typedef struct {
    int32_t filter;
    int32_t criterion;
    float threshold;
} liso_det_val_job;

/* (1) Pair matrices, pred-major: out[f][p][g] for ground-truth slot g and prediction slot p (the walk reads one prediction's
 *     row at a time).  Any of the three outputs may be NULL (not wanted).  Bytes per frame of each: 4*P*G.
 *   iou_bev: the value liso_iou3d_iou_bev_f32(gt[f], G, pred[f], P)[g][p], bit for bit (rbev_geom.h, ground truth as "box_a").
 *   iou_3d, after box_iou_matrix (liso/utils/nms_iou.py:179-207), with overlap = liso_iou3d_overlap_bev_f32's value:
 *       lo = z - 0.5f*dz, hi = z + 0.5f*dz                        (per box)
 *       h = min(hi_gt, hi_pred) - max(lo_gt, lo_pred)             (NaN if either operand is NaN, as torch.min / torch.max)
 *       inter = h > 0 ? overlap*h : 0
 *       union = (dx*dy)*dz [gt] + (dx*dy)*dz [pred] - inter
 *       iou = inter / max(union, FLT_EPSILON)                     (a NaN union stays NaN, as torch.clip)
 *   dist: sqrtf((gx-px)*(gx-px) + (gy-py)*(gy-py)), the 2-D centre distance.
 *   Entries of a pair with an invalid slot are written as 0. */
int liso_det_val_pairs_f32(int frames, int n_gt, int n_pred, const float* gt, const uint8_t* gt_valid, const float* pred,
                           const uint8_t* pred_valid, float* iou_bev, float* iou_3d, float* dist, void* stream);

/* Host twin of (1): host pointers, runs on the calling thread, the reference's host geometry (rbev_geom_host.h, the one
 * liso_iou3d_iou_bev_cpu_f32 uses: its iou_bev equals that function's bit for bit).  Gives the numpy restatement and the CPU
 * tests their matrices; not a fallback of the device path. */
int liso_det_val_pairs_cpu_f32(int frames, int n_gt, int n_pred, const float* gt, const uint8_t* gt_valid, const float* pred,
                               const uint8_t* pred_valid, float* iou_bev, float* iou_3d, float* dist);

/* (2) Class transfer (run_val :406-447).  Per frame: greedy walk over ALL valid boxes on `dist` (from (1)) with
 *     `threshold` (run_val: 3.0 m): a prediction takes the nearest free valid ground-truth box strictly closer than the
 *     threshold.  -> pred_class_out int32 [F,P] (4*P bytes per frame): draws[f][p] (the caller's random draw, int32 [F,P]) for a
 *     valid prediction, the ground-truth box's class for a matched one, -1 for an invalid slot. */
int liso_det_val_transfer_classes(int frames, int n_gt, int n_pred, const uint8_t* gt_valid, const int32_t* gt_class,
                                  const uint8_t* pred_valid, const int32_t* order, const float* dist, float threshold,
                                  const int32_t* draws, int32_t* pred_class_out, void* stream);

/* (3) Match: a grid of (job, frame) cells, one wavefront each.  The cell applies its job's filter set to both box sets, walks
 *     the surviving predictions in `order` and gives each one the not yet taken surviving ground-truth box of the best value
 *     in its row of the criterion's matrix: the largest IoU strictly above the threshold, or the smallest distance strictly
 *     below it; on equal values the lowest ground-truth slot; NaN is never chosen (what liso_match_greedy_f32 does).
 *   filters [n_filters], jobs [n_jobs]: DEVICE tables.  A job whose filter index or criterion is out of range matches nothing.
 *   iou_bev / iou_3d / dist: the matrices of (1); one that no job names may be NULL (host-checkable only through
 *     `criteria_mask`, bit c set = some job uses criterion c: a set bit with a NULL matrix is LISO_EINVAL).
 *   Outputs, with M = min(G,P) and bytes per frame:
 *     count  int32 [F,J]        4*J       matches of the cell
 *     pairs  int16 [F,J,M,2]    4*J*M     (gt slot, pred slot) in the order found, (-1,-1) after the last
 *     sums   fp64  [F,J,3]      24*J      ATE, ASE, AOE summed over the matches in match order; each term in fp32, after
 *                                         ObjectDetectionMetrics._update_class_threshold (od_metrics.py:489-545):
 *         ATE term: sqrtf(ddx*ddx + ddy*ddy) of the centres
 *         ASE term: 1 - inter / max(union, 1e-6f), inter = (min(dx)*min(dy))*min(dz), union = (dx*dy)*dz + (dx*dy)*dz - inter
 *         AOE term: |d|, d = mod(yaw_gt - yaw_pred + PIf, 2*PIf) - PIf with numpy's sign-of-divisor mod, d - 2*PIf if d > PIf
 *     gt_in  uint8 [F,S,G]      S*G       membership of every slot in every filter set (written by the set's jobs; a set
 *     pred_in uint8 [F,S,P]     S*P       that no job names is left untouched)
 *   The match values themselves are not stored: the metrics never read them. */
int liso_det_val_match_f32(int frames, int n_gt, int n_pred, const float* gt, const uint8_t* gt_valid, const int32_t* gt_class,
                           const float* pred, const uint8_t* pred_valid, const int32_t* pred_class, const int32_t* order,
                           const float* iou_bev, const float* iou_3d, const float* dist, int criteria_mask,
                           const liso_det_val_filter* filters, int n_filters, const liso_det_val_job* jobs, int n_jobs,
                           int32_t* count, int16_t* pairs, double* sums, uint8_t* gt_in, uint8_t* pred_in, void* stream);

/* (4) Assign: a grid of (job, frame) cells, one wavefront each, for the collections that match by optimal assignment
 *     (match_boxes_by_descending_confidence_iou(..., matching_mode="hungarian"), liso/kabsch/box_groundtruth_matching_iou.py:70-118:
 *     the IoU matrix padded to a square with -1, non-finite entries -> -1, scipy's linear_sum_assignment(maximize=True), matches
 *     with IoU >= threshold kept).  The cell applies its job's filter set to both box sets; with V the criterion's matrix:
 *       - either set empty: no matches;
 *       - c(g,p) = V[p][g] if finite, else -1.0f (assignable, never kept);
 *       - every member of the smaller set is assigned to a distinct member of the larger one so that the sum of c is largest (the
 *         reference's padded square problem has the same optima: its number of dummy assignments is fixed at |n_p - n_g|);
 *       - the assigned pairs with c >= threshold are kept, compared in fp32 with the job's fp32 threshold.  fp32(0.4), the
 *         reference's threshold, is the smallest fp32 not below 0.4, so every fp32 value is decided as the reference's fp64
 *         comparison decides it.
 *     Which of several equally good assignments is found is fixed by the method (scipy leaves it unspecified): rows are the smaller
 *     set in ascending slot order (the ground truth when both are equally large), columns the other set in ascending slot order;
 *     rows are inserted one by one by a shortest augmenting path; cost -c, potentials and running minima in fp64, starting at 0; a
 *     search step takes the unvisited column of the smallest reduced distance -- on equal distances a free (unassigned) column
 *     before an assigned one, then the lowest column position -- and shifts the potentials of the visited rows and columns and the minima of the others by that distance.  Additions, subtractions
 *     and comparisons only; liso_amd/eval/det_validation.py::assign_host is the same procedure in numpy and gives the same pairs bit
 *     for bit from the same matrix.
 *   Inputs as (3) without `order`; only the IoU criteria: criteria_mask in [0,3], a set bit with a NULL matrix is LISO_EINVAL, and a
 *     job that names LISO_DET_VAL_DIST (or a filter out of range) matches nothing.
 *   Outputs, with M = min(G,P):
 *     count  int32 [F,J]        kept pairs of the cell
 *     pairs  int16 [F,J,M,2]    (gt slot, pred slot) in ascending ground-truth slot, (-1,-1) after the last
 *     gt_in  uint8 [F,S,G], pred_in uint8 [F,S,P]   as (3) writes them, for THIS call's filter table
 *   No true-positive error sums: these collections never read them.
 *   Cost: one wavefront walks a cell alone; its dependent chain is (rows) x (steps of a row's search), a step being one pass over
 *   the 16 columns a lane owns at most.  Typical cells end a search after one or two steps; the worst case is 1024 rows x up to
 *   1024 steps.  Measured on MI355X: 512 cells of about 22 x 99 boxes 0.033 ms, one 1000 x 1024 cell with about 800 true overlaps
 *   9.4 ms. */
int liso_det_val_assign_f32(int frames, int n_gt, int n_pred, const float* gt, const uint8_t* gt_valid, const int32_t* gt_class,
                            const float* pred, const uint8_t* pred_valid, const int32_t* pred_class, const float* iou_bev,
                            const float* iou_3d, int criteria_mask, const liso_det_val_filter* filters, int n_filters,
                            const liso_det_val_job* jobs, int n_jobs, int32_t* count, int16_t* pairs, uint8_t* gt_in, uint8_t* pred_in,
                            void* stream);

/* The same device body on a caller's batch of plain matrices, no filters: value_pred_major fp32 [batch,n_pred,n_gt] (every slot takes
 * part), 0 <= n_gt, n_pred <= LISO_DET_VAL_MAX_BOXES -> count int32 [batch], pairs int16 [batch,min(n_gt,n_pred),2] as (4). */
int liso_match_assign_f32(const float* value_pred_major, long batch, int n_gt, int n_pred, float threshold, int32_t* count,
                          int16_t* pairs, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LISO_DET_VAL_H */
