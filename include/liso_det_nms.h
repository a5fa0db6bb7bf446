/*
 * liso_det_nms.h -- C ABI of detector inference post-processing on the device: dense head maps -> post-NMS boxes for a
 * batch, with no host synchronisation (graph-capturable).
 *
 * Replaces, per sample, what the reference does after the detector's forward pass in run_val
 * (liso/eval/eval_ours.py:361-386) and in the sequence tracker (liso/tracker/tracking.py:710-740): drop padding slots and
 * slots below a logit threshold, sort by score, optionally cut to `pre_nms_max`, greedy rotated NMS
 * (liso/utils/nms_iou.py:257-282 + iou3d_nms.cpp:90-136), keep the first `post_nms_max` survivors, index the boxes.
 *
 * Three steps, each one C call on the caller's stream:
 *   (a) liso_det_nms_order   per-sample stable descending order of the participating slots (segmented LSD radix sort)
 *   (b) liso_det_nms_select  survivor-bounded greedy rotated NMS over that order, one launch for the whole batch
 *   (c) liso_det_nms_gather  the kept rows of any number of per-slot fields into padded [B, P] arrays, one launch
 *
 * Conventions (as include/liso_iou3d.h): device pointers, no allocation, no host synchronisation; every entry point checks
 * all of its arguments before it launches anything and returns LISO_OK, LISO_EINVAL, LISO_EWORKSPACE or LISO_ELAUNCH.
 * B (batch) must be >= 1.  N (slots per sample) may be 0; then every input array pointer must be NULL (a non-NULL input
 * with N <= 0 is LISO_EINVAL) and the outputs say "nothing kept".
 */
#ifndef LISO_DET_NMS_H
#define LISO_DET_NMS_H

#include <stddef.h>
#include <stdint.h>

#include "liso_iou3d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LISO_DET_NMS_MAX_POST 1024         /* largest post_nms_max: the kept boxes' geometry lives in LDS */
#define LISO_DET_NMS_MAX_N (1 << 24)       /* largest N (slots per sample) */
#define LISO_DET_NMS_END_KEY 0xFFFFFFFFu   /* sort key of a slot that takes no part; sorted after every other slot */
#define LISO_DET_GATHER_MAX_FIELDS 8

/* bytes of device scratch liso_det_nms_order needs (0 when n == 0). */
size_t liso_det_nms_workspace_bytes(int batch, int n);

/* (a) Order.  Per sample b, slot i takes part iff (valid == NULL || valid[b][i] != 0) and
 *     !(gate[b][i] < logit_threshold) (gate == NULL: compare scores), so a NaN gate takes part as in the reference.
 *   scores fp32 [B,N]: sort key; gate fp32 [B,N] or NULL; valid uint8 [B,N] or NULL.
 *   -> sorted_idx int32 [B,N]: slot indices by DESCENDING score.  The order is STABLE: equal scores keep ascending slot
 *      index.  NaN sorts first (as the device torch.sort(stable=True, descending=True) puts it), -0.0 equals +0.0.
 *      The slots that take no part follow all others.
 *   -> sorted_keys uint32 [B,N]: the order-preserving key of each sorted entry (ascending), LISO_DET_NMS_END_KEY for the
 *      slots that take no part -- liso_det_nms_select stops at the first one.
 *   workspace: liso_det_nms_workspace_bytes(batch, n). */
int liso_det_nms_order(int batch, int n, const float* scores, const float* gate, const uint8_t* valid, float logit_threshold,
                       uint32_t* sorted_keys, int32_t* sorted_idx, void* workspace, size_t workspace_bytes, void* stream);

/* (b) Select.  Per sample: the first min(pre_nms_max, #participating) entries of the order (pre_nms_max <= 0: all of them)
 *     enter the reference's greedy pass -- box j is suppressed iff IoU(kept i, j) > thresh for a kept box i ranked above it,
 *     with the predicate of liso_iou3d_nms_f32 bit for bit (kept box as "box_a") -- which stops once post_nms_max boxes are
 *     kept.  boxes fp32 [B,N,7] = (x,y,z,dx,dy,dz,heading) per slot.  1 <= post_nms_max <= LISO_DET_NMS_MAX_POST.
 *   -> keep int64 [B, post_nms_max]: kept slot indices in keep order, -1 after the last; counts int32 [B]. */
int liso_det_nms_select(int batch, int n, const float* boxes, const uint32_t* sorted_keys, const int32_t* sorted_idx, float thresh,
                        int pre_nms_max, int post_nms_max, int64_t* keep, int32_t* counts, void* stream);

/* One per-slot field for liso_det_nms_gather: src [B,N,row_elems], dst [B,P,row_elems], contiguous, elements of elem_bytes
 * (1, 2, 4 or 8) bytes; rows that are not kept get the low elem_bytes bytes of pad_bits (little-endian). */
typedef struct {
    const void* src;
    void* dst;
    int row_elems;
    int elem_bytes;
    uint64_t pad_bits;
} liso_det_gather_field;

/* (c) Gather.  dst[b][p] <- src[b][keep[b][p]] for p < counts[b], the padding row otherwise; 1 <= n_fields <=
 *     LISO_DET_GATHER_MAX_FIELDS, `fields` is a host array (read during the call). */
int liso_det_nms_gather(int batch, int n, int post_nms_max, const int64_t* keep, const int32_t* counts,
                        const liso_det_gather_field* fields, int n_fields, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LISO_DET_NMS_H */
