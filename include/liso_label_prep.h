/*
 * liso_label_prep.h -- C ABI of the label side of a training sample on the device: which boxes hold a point, the box filter with
 * its order-preserving compaction, the object velocity of tracked ground truth, the ignore-region mask, and the full CenterPoint
 * target rendering.  No host synchronisation (graph-capturable).
 *
 * Replaces, in liso/datasets/torch_dataset_commons.py: filter_objects_to_bev_non_empty (:1013-1059) with the
 * use_double_precision=False branch of get_points_in_boxes_mask (:1902-1935) and object_is_in_bev_range (:1228-1231),
 * get_object_velocity_in_obj_coords (:1116-1145), create_true_where_ignore_region_mask (:919-941) with render_hard_kabsch_mask
 * (liso/kabsch/kabsch_mask.py:119-146), and draw_heat_regression_maps (:190-339) in full.
 *
 * Conventions (as include/liso_sample_prep.h): device pointers, caller-allocated outputs, no allocation, no host synchronisation;
 * every entry point checks its arguments before it launches anything and returns LISO_OK, LISO_EINVAL or LISO_ELAUNCH.  Boxes are
 * padded arrays [B, K, .] with valid uint8 [B, K]; box geometry comes in fp64 (pos [B, K, 3], dims [B, K, 3], rot [B, K]).  Clouds
 * are rows of a [B, n_max, point_stride] fp32 array (x, y, z first); cloud b has counts[b] rows (counts == NULL: n_max each), rows
 * behind the count are never read.  The source file is compiled without FMA contraction: every expression below is evaluated
 * operation by operation, in the order written.
 */
#ifndef LISO_LABEL_PREP_H
#define LISO_LABEL_PREP_H

#include <stddef.h>
#include <stdint.h>

#include "liso_iou3d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LISO_LABEL_MAX_N (1 << 24)     /* rows per cloud */
#define LISO_LABEL_MAX_BOXES 65535     /* K */
#define LISO_LABEL_MAX_CELLS (1 << 24) /* h * w */
#define LISO_LABEL_MAX_ATTRS 8         /* attribute arrays per liso_filter_boxes call */

/* 1. flags[b][k] != 0 where box k of sample b contains a row of cloud b.  Every slot is tested, valid or not, as the reference
 *   does.  The inverse pose is built in fp64 in closed form and rounded to fp32:
 *     row0 = (c, s, -(c*x + s*y)), row1 = (-s, c, -(c*y - s*x)), tz = -z,  c = cos(rot), s = sin(rot);
 *   a point is then taken to the box frame in fp32, u = (row0[0]*px + row0[1]*py) + row0[2], v likewise, w = pz + tz, and lies
 *   inside when |u| < 0.5*dx, |v| < 0.5*dy and |w| < 0.5*dz (strict, compared in fp64).  A row with a NaN coordinate is in no
 *   box.  flags is uint32 [B, K]; the call zeroes it first.  n_boxes == 0 or n_max == 0 is fine.
 *   Sized for the tens to hundreds of boxes of a sample: the pass is a brute-force n_max x K test, and every tile of 256 points
 *   rebuilds the frames of all K boxes (an fp64 sin / cos each, next to the tile's 256 tests per box).  LISO_LABEL_MAX_BOXES is
 *   what the launch geometry admits, not a size the pass is tuned for; thousands of boxes want a spatial index first. */
int liso_box_has_points_f32(int batch, int n_boxes, int n_max, int point_stride, const double* box_pos, const double* box_dims,
                            const double* box_rot, const float* pcl, const int32_t* counts, uint32_t* flags, void* stream);

/* 2. The filter and its compaction.  keep[b][k] = valid && has_points && in_bev && in_range with
 *     has_points = flags[b][k] != 0 (flags given) or has_points_in[b][k] != 0 (exactly one of the two is given),
 *     in_bev     = !filter_bev   || (0.5*range_x >= |x| && 0.5*range_y >= |y|),
 *     in_range   = !filter_range || sqrt((x*x + y*y) + z*z) < filter_range_m,        all in fp64.
 *   The kept boxes move, in their input order, to the front of every attribute array: rows of row_bytes bytes (a multiple of 4),
 *   src and dst [B, K, row_bytes] and distinct; the slots behind them are zeroed.  out_valid uint8 [B, K] marks the kept slots.
 *   has_points_out (uint8 [B, K], optional) receives has_points, in the input's slot order. */
typedef struct {
    const void* src;
    void* dst;
    int row_bytes;
} liso_box_attr_job;

typedef struct {
    int batch;    /* B >= 1 */
    int n_boxes;  /* K >= 0 */
    int filter_bev;
    int filter_range;
    double range_x, range_y; /* bev_range_m, > 0 */
    double filter_range_m;
} liso_box_filter_cfg;

int liso_filter_boxes(const liso_box_filter_cfg* cfg, const double* box_pos, const uint8_t* valid, const uint32_t* flags,
                      const uint8_t* has_points_in, const liso_box_attr_job* attrs, int n_attrs, uint8_t* out_valid,
                      uint8_t* has_points_out, void* stream);

/* 3. out[b][k] (fp64 [B, K, 3]) = the first three entries of pose_ta * (f, 0) with
 *     f = ((pose_tb * pose_ta^-1 - I) - (odom_ta_tb^-1 - I)) * (pose_ta[0][3], pose_ta[1][3], 0, 1),
 *   all 4x4 row-major fp64 (odom [B, 16], poses [B, K, 16]); products as ((a0*b0 + a1*b1) + a2*b2) + a3*b3, the inverses in closed
 *   form for an affine matrix (adjugate of the 3x3 block over its determinant, -A^-1 t). */
int liso_object_velocity_f64(int batch, int n_boxes, const double* odom_ta_tb, const double* pose_ta, const double* pose_tb,
                             double* out, void* stream);

/* 4. mask[b][i][j] (uint8 [B, h, w]) = 1 where the centre of cell (i, j),
 *     (((i + 0.5) / h) * range_x - 0.5*range_x, ((j + 0.5) / w) * range_y - 0.5*range_y),
 *   lies strictly inside a valid box in the box frame: u = (c*px + s*py) - (c*x + s*y), v = (c*py - s*px) - (c*y - s*x),
 *   -0.5*dx < u < 0.5*dx and -0.5*dy < v < 0.5*dy, in fp64. */
int liso_ignore_region_mask(int batch, int n_boxes, int h, int w, double range_x, double range_y, const double* box_pos,
                            const double* box_dims, const double* box_rot, const uint8_t* valid, uint8_t* mask, void* stream);

/* 5. The target maps of draw_heat_regression_maps.  Per valid box a rotated gaussian, evaluated in fp64 at the cell centres of
 *   entry 4: u = dx*c + dy*s, v = dy*c - dx*s, heat = exp(-((u*u) / (0.15*len) + (v*v) / (0.15*wid)) / 2), divided by the box's
 *   maximum over the grid clamped at 1e-5 (normalize_gaussian == 0) or by sqrt((2 pi)^2 * (0.15*len) * (0.15*wid))
 *   (normalize_gaussian == 1).  occupied = heat > 0.01; scaled = prob_scale * heat (prob_scale fp64 [B, K] or NULL; must be NULL
 *   with normalize_gaussian).  Per cell: probs = max scaled over the valid boxes; dims / pos / rot / velo = the sum, over the boxes
 *   whose scaled heat equals that maximum and that occupy the cell, of dims (log(dims) with log_dims), pos, (sin, cos) of rot
 *   (rot_channels == 2) or rot itself (rot_channels == 1), and velo; everything rounded once to fp32.  A sample without a valid box
 *   gives zeros.  center_mask uint8 [B, h, w] = 1 in the cell min(max(trunc(((p + 0.5*range) / range) * n), 0), n - 1) of every
 *   valid box centre.  box_max: fp64 [B, K] scratch.  Outputs fp32 [B, h, w, 1 | 3 | 3 | rot_channels | 1]. */
typedef struct {
    int batch, n_boxes, h, w;
    int rot_channels;       /* 2: vector, 1: direct / class_bins */
    int log_dims;           /* predict_log_size */
    int normalize_gaussian;
    int reserved;
    double range_x, range_y;
} liso_targets_ex_cfg;

int liso_render_center_targets_ex_f32(const liso_targets_ex_cfg* cfg, const double* box_pos, const double* box_dims,
                                      const double* box_rot, const double* box_velo, const double* prob_scale,
                                      const uint8_t* box_valid, double* box_max, float* probs, float* dims, float* pos, float* rot,
                                      float* velo, uint8_t* center_mask, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LISO_LABEL_PREP_H */
