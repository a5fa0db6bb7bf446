/*
 * liso_flow_metrics.h -- C ABI of the scene-flow validation metrics (gfx950): per-point flow-error statistics accumulated into a
 * device-resident state across calls.
 *
 * Replaces the host numpy of the reference's SLIM validation pass
 *   liso/slim/experiment.py:580-833   run_eval_on_this_dataset: per batch and per evaluated flow (raw / agg / rig)
 *   liso/slim/utils/metrics.py        compute_scene_flow_metrics_for_points_in_this_mask, get_inlier_outlier_ratios,
 *                                     get_ratio_for_thresh, aggregate_metrics
 *   liso/eval/flow_metrics.py         FlowMetrics.update: AEE per range bin for still / moving / overall points
 * so that the five [B,N,3] arrays of a batch never travel to the host.
 *
 * Per point (f32, the operation order of numpy on f32 arrays; the library compiles this file without FMA contraction):
 *   EPE = sqrt((dx*dx + dy*dy) + dz*dz), d = pred - gt        (np.linalg.norm(pred - gt, axis=-1))
 *   rel = EPE / |gt|                                          (inf / NaN for a zero ground-truth flow, as numpy)
 *   range = |points[:3]|, compared as a double against the f64 bin edges: bin j holds edges[j] <= range < edges[j+1]
 *   ACC3D_0_05: EPE < 0.05f || rel < 0.05f     ACC3D_0_1: EPE < 0.1f || rel < 0.1f
 *   Outliers3D: EPE > 0.3f  || rel > 0.1f      RobustOutliers3D: EPE > 0.3f && rel > 0.3f
 * Categories (valid = pcl_is_valid, mov = moving_mask, lab = point_has_valid_flow_label; lab NULL = all set):
 *   label "moving" = mov & valid & lab, label "still" = ~mov & valid & lab   (experiment.py:622-631; overall = their union)
 *   range "moving" = label "moving", range "still" = valid & ~(label "moving") (FlowMetrics called with mask = pcl_is_valid,
 *                                                                            experiment.py:789-799; overall = valid)
 * Counts are integers.  Sums are f64: per-block partials (a block = 256 threads, a fixed grid for a given row count), then a
 * second launch adds the partials of every slot in a fixed order (one wave per slot: lane l sums blocks l, l + 64, ... in turn,
 * then a fixed butterfly over the lanes) and the result into the state.  Results are bitwise reproducible, eager or replayed
 * from a hipGraph.  `update` neither allocates nor synchronises.
 *
 * The state is ONE device buffer of liso_flow_metrics_state_bytes() bytes, 16-byte aligned; it begins with a
 * liso_flow_metrics_result and continues with the partials scratch.  All entry points return LISO_OK or a negative LISO_E*
 * code (include/liso_iou3d.h); argument errors are reported before anything is launched.
 */
#ifndef LISO_FLOW_METRICS_H
#define LISO_FLOW_METRICS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LISO_FLOW_METRICS_MAX_FLOWS 3
#define LISO_FLOW_METRICS_MAX_BINS 32

/* label-category statistics: count slots, then sum slots */
enum { LISO_FM_N = 0, LISO_FM_ACC3D_0_05 = 1, LISO_FM_ACC3D_0_1 = 2, LISO_FM_OUTLIERS3D = 3, LISO_FM_ROBUST_OUTLIERS3D = 4 };
enum { LISO_FM_SUM_EPE = 0, LISO_FM_SUM_PRED = 1 /* xyz */, LISO_FM_SUM_PRED_LEN = 4, LISO_FM_SUM_GT = 5 /* xyz */,
       LISO_FM_SUM_GT_LEN = 8, LISO_FM_SUM_ERR = 9 /* xyz of pred - gt */ };

typedef struct {
    uint64_t label_count[LISO_FLOW_METRICS_MAX_FLOWS][2][5];  /* [flow][moving, still][LISO_FM_N ..] */
    double label_sum[LISO_FLOW_METRICS_MAX_FLOWS][2][12];     /* [flow][moving, still][LISO_FM_SUM_* ..] */
    /* [flow][still, moving][bin 0 .. n_bins-1 | LISO_FLOW_METRICS_MAX_BINS = every point of the category, in a bin or not] */
    uint64_t range_count[LISO_FLOW_METRICS_MAX_FLOWS][2][LISO_FLOW_METRICS_MAX_BINS + 1];
    double range_sum[LISO_FLOW_METRICS_MAX_FLOWS][2][LISO_FLOW_METRICS_MAX_BINS + 1];  /* EPE sums, same layout */
    uint32_t empty_overall; /* set when an update had no point in the label union (the reference's metric dict is NaN then) */
    uint32_t updates;       /* number of update calls since the last reset */
    uint32_t reserved[2];
} liso_flow_metrics_result;

size_t liso_flow_metrics_state_bytes(void);
size_t liso_flow_metrics_result_bytes(void); /* sizeof(liso_flow_metrics_result) */

/* zero the accumulated result (one launch) */
int liso_flow_metrics_reset(void* state, void* stream);

/* Accumulate `rows` points (= B*N of [B,N] inputs) for `n_flows` (1..3) predicted flows.  points: rows x >= 3 floats,
 * `points_stride` floats apart (may be NULL when n_bins == 0); gt_flow / pred_k: rows x 3 floats, `*_stride` (>= 3) floats apart;
 * the masks are one byte per row (0 / 1): pcl_is_valid, moving_mask, has_flow_label (NULL = every point labelled).
 * bin_edges: HOST array of n_bins + 1 non-decreasing doubles (copied into the launch), 0 <= n_bins <= 32.
 * point_epe (optional, NULL = none): device float [n_flows][rows], receives every row's EPE. */
int liso_flow_metrics_update(void* state, long rows, const float* points, long points_stride, const float* gt_flow, long gt_stride,
                             int n_flows, const float* pred0, long pred0_stride, const float* pred1, long pred1_stride,
                             const float* pred2, long pred2_stride, const uint8_t* pcl_is_valid, const uint8_t* moving_mask,
                             const uint8_t* has_flow_label, const double* bin_edges, int n_bins, float* point_epe, void* stream);

/* copy the accumulated result to the HOST struct `out` and wait for the stream */
int liso_flow_metrics_read(const void* state, liso_flow_metrics_result* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LISO_FLOW_METRICS_H */
