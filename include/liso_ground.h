/*
 * liso_ground.h -- C ABI of ground segmentation on the device: JCP range-image ground removal for a batch of sweeps, the cone
 * test, and the order-preserving removal of the ground points, with no host synchronisation (graph-capturable).
 *
 * Replaces liso/jcp/jcp.py:253-384 (JPCGroundRemove: RangeProjection, RECM, 5x5 cross dilation, JCP),
 * liso/datasets/torch_dataset_commons.py:133-144 (infer_ground_label_using_cone) and the point removal of :1165-1185.
 *
 * The result of liso_ground_jcp_f32 is defined as the reference's JPCGroundRemove applied to the float64 widening of the
 * cloud: all projection, threshold and weight arithmetic is fp64 in the reference's operation order (the source file is
 * compiled without FMA contraction), with the reference's quirks kept (its never-true bounds tests, last-writer-wins pixels,
 * the transposed cloud_index_ read of the candidate filter, raster-order in-place JCP).  Two more follow from its indexing:
 *   - A point with y == -0.0 and x < 0 has the angle -pi and, `y < 0` being false, the negative column trunc(-(W-1)/2).  The
 *     reference keeps it out of the projection (col < 0: no winner, no region_minz update) and reads its label with numpy's
 *     negative index, from pixel (row, W + col).  So do the device and the host path.
 *   - The flat region index col * length + region of a point with r_xy == 70 exactly is the next column's region 0.  In the last
 *     column that is one past the table, where the reference (compiled without bounds checks) writes out of bounds.  Defined
 *     here: such a point leaves region_minz alone, still becomes its pixel's winner, and is classified against the table's
 *     last entry.
 *
 * Stages of liso_ground_jcp_f32, each one or two launches on the caller's stream:
 *   0 init        workspace tables
 *   1 elevation   per-point elevation, min / max of the finite ones per cloud (block reduction + ordered-integer atomics)
 *   2 projection  point -> pixel: atomicMax of the winner index, ordered-key atomicMin of region_minz
 *   3 recm        per-column scans of region_minz (one column per lane), per-pixel ground / obstacle
 *   4 candidates  dilation + candidate filter, per-row candidate lists, the 24 JCP weights of every candidate
 *   5 resolve     the sequential JCP pass as a skewed wavefront, one workgroup per cloud: the lane of row r resolves column
 *                 t - 3r at step t; equal to the raster-order result bit for bit
 *   6 gather      per-point label
 *
 * Conventions (as include/liso_det_nms.h): device pointers, caller-allocated outputs, no allocation, no host synchronisation;
 * every entry point checks its arguments before it launches anything and returns LISO_OK, LISO_EINVAL, LISO_EWORKSPACE,
 * LISO_ELAUNCH or LISO_GROUND_ELENGTH.  Clouds are rows of a [B, n_max, point_stride] fp32 array (x, y, z first); cloud b has
 * counts[b] rows (counts == NULL: n_max each).  A row with a NaN coordinate is invalid: it is labelled 0 and takes no part.
 */
#ifndef LISO_GROUND_H
#define LISO_GROUND_H

#include <stddef.h>
#include <stdint.h>

#include "liso_iou3d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LISO_GROUND_ELENGTH (-4)          /* int(67 / delta_r) > 255: the reference's uint8 region image would wrap */
#define LISO_GROUND_MAX_HEIGHT 1024       /* range-image rows: one lane per row in the resolve workgroup */
#define LISO_GROUND_MAX_PIXELS (1 << 24)  /* width * height */
#define LISO_GROUND_MAX_N (1 << 24)       /* rows per cloud */
#define LISO_GROUND_LDS_BYTES (160 * 1024) /* label images up to this size are resolved in LDS, larger ones in global memory */
#define LISO_GROUND_N_STAGES 7
#define LISO_GROUND_N_LAYOUT 11           /* entries of liso_ground_jcp_workspace_layout */

typedef struct {
    int batch;            /* B >= 1 */
    int n_max;            /* rows per cloud, >= 0 */
    int point_stride;     /* floats per row, >= 3 */
    int width;            /* range_img_width */
    int height;           /* range_img_height, <= LISO_GROUND_MAX_HEIGHT; (height-1)*height + width-1 < width*height */
    double sensor_height;
    double delta_r;       /* > 0 */
} liso_ground_cfg;

/* bytes of device scratch liso_ground_jcp_f32 needs; 0 for a configuration it refuses. */
size_t liso_ground_jcp_workspace_bytes(const liso_ground_cfg* cfg);

/* pcl fp32 [B, n_max, point_stride]; counts int32 [B] or NULL -> is_ground uint8 [B, n_max] (1 = ground). */
int liso_ground_jcp_f32(const liso_ground_cfg* cfg, const float* pcl, const int32_t* counts, uint8_t* is_ground, void* workspace,
                        size_t workspace_bytes, void* stream);

/* Byte offsets of the workspace tables into offsets[LISO_GROUND_N_LAYOUT], from the carver the kernels use, each 256-byte aligned
 * (for tests that look at a stage's tables).  Per cloud b, in order:
 *   0 ele_key  uint64 [B][2]        ordered keys of the min / max finite elevation (key = bits ^ sign-extended mask, see below)
 *   1 ele      fp64   [B][n_max]    elevation of every valid row
 *   2 pix      int32  [B][n_max]    col * H + row of the pixel a row's label is read from, -1 for invalid rows
 *   3 widx     int32  [B][W*H]      winner row per pixel at col * H + row, -1 = none
 *   4 minz_key uint32 [B][W*length] ordered fp32 key of the smallest z per (column, region); the key of 100.0f = untouched
 *   5 minz     fp64   [B][W*length] the same widened, then RECM's thresholds (stage 3)
 *   6 lab0     uint8  [B][S]        labels after RECM, row * W + col; S = W*H rounded up to 16; 0 empty, 1 ground, 2 obstacle
 *   7 lab1     uint8  [B][S]        labels after the candidate filter (3 = candidate, stage 4), then resolved (stage 5)
 *   8 row_cnt  int32  [B][H]        candidates per row
 *   9 cols     int32  [B][H][W]     their columns, ascending, the first row_cnt of each row
 *  10 wts      fp64   [B][H][W][24] their weights in the same slots
 * An ordered key of a value with bits u is ~u for a negative value and u with the sign bit set for the others.
 * LISO_EINVAL for a configuration liso_ground_jcp_workspace_bytes refuses or a null pointer. */
int liso_ground_jcp_workspace_layout(const liso_ground_cfg* cfg, size_t* offsets);

/* the stages [stage_begin, stage_end) only, on a workspace the earlier stages have filled (per-stage timing, stage tests). */
int liso_ground_jcp_stages_f32(const liso_ground_cfg* cfg, const float* pcl, const int32_t* counts, uint8_t* is_ground,
                               void* workspace, size_t workspace_bytes, int stage_begin, int stage_end, void* stream);

/* Cone test in fp64: out[b][i] = (or_with ? or_with[b][i] : 0) | (z < z_threshold + slope * sqrt(x*x + y*y)) for valid rows, 0 for
 * the others.  slope = tan(cone angle), 0 for the flat test; or_with uint8 [B, n_max] or NULL; out may alias or_with. */
int liso_ground_cone_f32(int batch, int n_max, int point_stride, const float* pcl, const int32_t* counts, double z_threshold,
                         double slope, const uint8_t* or_with, uint8_t* out, void* stream);

/* Order-preserving removal: the valid rows of cloud b with drop[b][i] == 0 move, in order, to the front of out[b]; the rows
 * behind them are filled with NaN; out_counts[b] = number of kept rows.  pcl / out fp32 [B, n_max, point_stride]. */
size_t liso_ground_compact_workspace_bytes(int batch, int n_max);
int liso_ground_compact_f32(int batch, int n_max, int point_stride, const float* pcl, const int32_t* counts, const uint8_t* drop,
                            float* out, int32_t* out_counts, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LISO_GROUND_H */
