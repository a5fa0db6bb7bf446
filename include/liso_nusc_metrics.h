/*
 * liso_nusc_metrics.h -- C ABI of the per-frame part of the nuScenes detection metrics (mAP over centre-distance thresholds, the
 * true-positive errors, NDS) on the device: every frame of a padded batch against every distance threshold in ONE launch, with no
 * host synchronisation and no allocation (graph-capturable).
 *
 * Replaces, per frame, what the reference's run_val does through NuscenesObjectDetectionMetrics.update
 * (liso/eval/nuscenes_metrics_wrapper.py:121-165: the per-class radial filter, the clamp of the predictions' sizes) and the matching
 * loop of the nuScenes devkit's `accumulate` (nuscenes/eval/detection/algo.py:76-120).  That loop walks ALL predictions of a data
 * set by descending confidence but keeps its `taken` set per sample, so it is one greedy walk per frame; the data-set wide sort, the
 * precision / recall curves and the interpolation of the errors stay on the host in float64
 * (liso_amd/eval/nuscenes_metrics.py; liso_amd/eval/od_metrics.py says why).
 *
 * It is a kernel of its own next to liso_det_val_match_f32 (include/liso_det_val.h) because the range rule differs (inclusive, one
 * radius per class), the curves need the errors of every match and not their sum per frame, and the centre distance needs no [P,G]
 * matrix in memory: it is computed on the fly.
 *
 * Conventions (as include/liso_det_val.h): device pointers unless stated, every index a SLOT index, arguments checked before
 * anything is launched, returns LISO_OK, LISO_EINVAL or LISO_ELAUNCH.
 *
 * Inputs: a padded batch of F frames (F >= 0; F == 0 launches nothing).
 *   gt   fp32 [F,G,7] rows (x,y,z,dx,dy,dz,heading), gt_valid   uint8 [F,G], gt_class   int32 [F,G]
 *   pred fp32 [F,P,7],                               pred_valid uint8 [F,P], pred_class int32 [F,P]
 *   order int32 [F,P]: every frame's prediction slots, most confident first -- liso_det_nms_order's sorted_idx (stable: equal
 *        scores keep ascending slot index) on the scores the collection sees.  Entries outside [0,P) are skipped.
 *   radius fp32 [n_classes] (device), n_classes >= 1: the largest distance from the origin at which a box of class c is evaluated.
 *   as_one != 0: every box counts as class 0 with radius[0]; gt_class and pred_class are not read (may be NULL).
 *   thresholds: HOST array of n_thresholds floats, 1 <= n_thresholds <= LISO_NUSC_MAX_THRESHOLDS, copied into the launch.
 *   0 <= G, P <= LISO_DET_VAL_MAX_BOXES.  Holes in the valid masks are allowed; what invalid slots hold is never used.
 *
 * Membership.  A box (x, y) of class c (0 when as_one) is a member iff it is valid, 0 <= c < n_classes and
 *   sqrtf(x*x + y*y) <= radius[c]            (fp32; the bound is INCLUSIVE: the reference drops dist > range; a NaN fails).
 *
 * Cells.  One cell per (frame, threshold), one wavefront each.  The walk visits the member predictions in `order`.  A prediction
 *   p of class c looks at the member ground-truth boxes g of class c that no earlier prediction of this cell has taken, with
 *     d(g,p) = sqrtf(ddx*ddx + ddy*ddy),  ddx = x_g - x_p, ddy = y_g - y_p        (fp32)
 *   and takes the one of the smallest d; on equal d the lowest ground-truth slot; a NaN d is never chosen.  It is a match iff that
 *   d < threshold (strictly); a matched ground-truth box is taken for the rest of the cell.  One walk serves all classes.
 *
 * Outputs, with T = n_thresholds and M = min(G,P):
 *   count   int32 [F,T]        matches of the cell
 *   pairs   int16 [F,T,M,2]    (gt slot, pred slot) in match order, (-1,-1) after the last
 *   err     fp32  [F,T,M,3]    (trans, scale, orient) of every match, 0 after the last; each in fp32, operation by operation:
 *       trans:  d(g,p), the matched distance
 *       scale:  1 - inter / union with s = the prediction's (dx,dy,dz), each component below 1e-4f raised to 1e-4f (a NaN stays;
 *               nuscenes_metrics_wrapper.py:161), the ground truth's sizes as they are,
 *               inter = (min(dx)*min(dy))*min(dz), union = (dx*dy)*dz [gt] + (dx*dy)*dz [pred] - inter; min gives NaN if either
 *               operand is NaN; no clamp on union (the devkit's scale_iou has none)
 *       orient: the AOE term of include/liso_det_val.h: |d|, d = mod(yaw_gt - yaw_pred + PIf, 2*PIf) - PIf with numpy's
 *               sign-of-divisor mod, d - 2*PIf if d > PIf
 *       A scale or orient term that is NaN (a NaN size or heading of a matched box) is stored as the quiet NaN 0x7FC00000.
 *   gt_in   uint8 [F,G], pred_in uint8 [F,P]    the membership (the same for every threshold)
 *   (The velocity and attribute errors of the devkit need nothing from the device: the reference gives every box velocity (0,0)
 *   and no attribute.)
 *
 * Cost: one wavefront walks a cell alone.  A lane keeps x, y, class and a "member and free" bit of the ground-truth slots lane,
 *   lane + 64, ... in registers (16 slots per lane at G = 1024); the member predictions are staged in LDS in visiting order.  A step
 *   is one pass over the lane's slots, one ballot, and for a prediction with a candidate one 64-bit wave maximum.
 */
#ifndef LISO_NUSC_METRICS_H
#define LISO_NUSC_METRICS_H

#include <stddef.h>
#include <stdint.h>

#include "liso_det_val.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LISO_NUSC_MAX_THRESHOLDS 8

int liso_det_val_nusc_f32(int frames, int n_gt, int n_pred, const float* gt, const uint8_t* gt_valid, const int32_t* gt_class,
                          const float* pred, const uint8_t* pred_valid, const int32_t* pred_class, const int32_t* order,
                          const float* radius, int n_classes, int as_one, const float* thresholds, int n_thresholds, int32_t* count,
                          int16_t* pairs, float* err, uint8_t* gt_in, uint8_t* pred_in, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LISO_NUSC_METRICS_H */
