/*
 * liso_flow_labels.h -- C ABI of the per-point ground truth the dataset builders derive from annotated, tracked boxes: the scene
 * flow flow_ta_tb, the track id / annotation index and the box slot of every point, the point count of every box, and KITTI's
 * lidar row and column of every point.  No host synchronisation (graph-capturable).
 *
 * Replaces the three statements of one computation in the builders, each with its own overlap rule:
 *   liso/datasets/kitti/create_kitti_tracking.py:14-17, :340-387 (get_points_in_box_mask, extract_lidar_flow_ta_tb): boxes in
 *     order, a later box overwrites an earlier one; the id for every containing box, the flow only for boxes present at tb;
 *   liso/datasets/nuscenes/create.py:229-238, :301-366, :392-429: the same overwrite, the t0 membership gated by the point's
 *     semantic class (:339-342), num_lidar_pts_t0 the ungated count (:374);
 *   liso/datasets/argoverse2/create.py:216-228, :357-383 (update_dynamic_flow): the first containing box wins, once per category
 *     on a flow array updated in place;
 * and liso/datasets/kitti/kitti_range_image_projection_helper.py:4-29 (find_jumps, find_cols).
 *
 * Conventions (as include/liso_label_prep.h): device pointers, caller-allocated outputs, no allocation, no host synchronisation;
 * every entry point checks its arguments before it launches anything and returns LISO_OK, LISO_EINVAL or LISO_ELAUNCH.  Clouds are
 * rows of a [C, n_max, point_stride] fp32 array (x, y, z first); cloud c has counts[c] rows (counts == NULL: n_max each, else
 * clamped to [0, n_max]), rows behind the count are never read.  The source file is compiled without FMA contraction: every
 * expression below is evaluated operation by operation, in the order written.
 */
#ifndef LISO_FLOW_LABELS_H
#define LISO_FLOW_LABELS_H

#include <stddef.h>
#include <stdint.h>

#include "liso_iou3d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LISO_FLOW_LABELS_MAX_N (1 << 24)  /* rows per cloud */
#define LISO_FLOW_LABELS_MAX_JOBS 65535   /* J, and C */
#define LISO_FLOW_LABELS_MAX_BOXES 4096   /* K per job; J * K <= 2^24 */
#define LISO_FLOW_LABELS_CHUNK 128        /* boxes of a job resident in LDS at a time (K may exceed it) */

#define LISO_OVERLAP_LAST 0  /* a later box overwrites an earlier one (KITTI, nuScenes) */
#define LISO_OVERLAP_FIRST 1 /* the first containing box wins (Argoverse 2) */

/* 1. Flow labels of J jobs in one call.  One job is one directed sweep pair (ta -> tb) of one sample; job j reads the cloud
 *   cloud_of[j] (several jobs may share a cloud).  A cloud_of[j] outside [0, C) makes job j a job without rows.
 *
 *   Per job j: odom fp64 [J, 4, 4] (the reference's odom_ta_tb, row-major), and padded box tables [J, K, .]:
 *     pose_a, pose_b fp64 [J, K, 4, 4]  the box pose at ta and at tb: general rigid poses [R | t], not yaw-only
 *     size           fp64 [J, K, 3]     full extents along the box axes
 *     valid, has_b   uint8 [J, K]       the slot holds a box; the box exists at tb
 *     label          int32 [J, K]       track id / annotation index
 *     box_class      int32 [J, K] or NULL, together with point_class int32 [C, n_max] or NULL (both or neither)
 *
 *   With M a rigid pose, rinv(M) = [R^T | -R^T t] is
 *     rinv[r][c] = M[c][r],  rinv[r][3] = -((M[0][r] * M[0][3] + M[1][r] * M[1][3]) + M[2][r] * M[2][3]),   r, c < 3,
 *   and a 3x4 matrix applied to the point p = (x, y, z, 1), widened to fp64, is
 *     (M p)[r] = ((M[r][0] * x + M[r][1] * y) + M[r][2] * z) + M[r][3].
 *   Per box k:   A = rinv(pose_a[k]);
 *                D[r][c] = ((Pb[r][0] * A[0][c] + Pb[r][1] * A[1][c]) + Pb[r][2] * A[2][c]) - (r == c ? 1 : 0)           c < 3,
 *                D[r][3] = (((Pb[r][0] * A[0][3] + Pb[r][1] * A[1][3]) + Pb[r][2] * A[2][3]) + Pb[r][3])                 Pb = pose_b[k];
 *   per job:     S = rinv(odom[j]) with 1 subtracted from its diagonal.
 *
 *   For a row i < counts[cloud_of[j]] with finite x, y, z:
 *     inside_k = valid_k && |(A p)[0]| < size_x / 2 && |(A p)[1]| < size_y / 2 && |(A p)[2]| < size_z / 2     (strict, fp64)
 *     member_k = inside_k && (box_class == NULL || box_class_k < 0 || point_class[cloud][i] == box_class_k)
 *     count[j][k]   = the number of rows with inside_k: geometric, ungated, integer atomics (independent of order)
 *     label winner  = the last (LISO_OVERLAP_LAST) or first (LISO_OVERLAP_FIRST) k with member_k:
 *                     point_label = label_k, point_box = k; none: no_label and -1
 *     flow winner   = the last / first k with member_k && has_b_k: flow = (D_k p)[0:3]; none: flow = (S p)[0:3], or, with
 *                     keep_flow != 0, the value flow already holds (flow is then an in/out array)
 *   each flow component rounded to fp32 once.  The two winners are independent: a point in an unpartnered later box and a
 *   partnered earlier one takes its id from the one and its flow from the other, as KITTI's loop does.
 *   Rows at or behind the count and rows with a non-finite coordinate get flow NaN (whatever keep_flow says), no_label and -1,
 *   and count for no box.
 *
 *   An fp32 sphere around the box centre rejects most (point, box) pairs before the fp64 test.  It is conservative for rigid
 *   poses (R orthonormal to 1e-4) whose translation and points lie within 1e4 m: inside implies |p - t|^2 < |size / 2|^2, and the
 *   sphere's radius carries a margin of 0.1 % + 0.05 m^2 for the fp32 rounding of that distance.
 *
 *   Outputs: flow fp32 [J, n_max, 3]; point_label int32 [J, n_max], point_box int32 [J, n_max], count int32 [J, K] (zeroed by
 *   the call) -- each of the three NULL or given.  Two launches whatever J and K are: one builds A, D, S and the spheres into
 *   the workspace (liso_flow_labels_workspace_bytes(J, K) bytes, 256-byte aligned), one does the points, one thread per point,
 *   the job's boxes staged through LDS in chunks of LISO_FLOW_LABELS_CHUNK.  K == 0 and n_max == 0 are fine.
 *   K > LISO_FLOW_LABELS_MAX_BOXES returns LISO_EINVAL. */
typedef struct {
    int n_jobs;       /* J >= 1 */
    int n_clouds;     /* C >= 1 */
    int n_boxes;      /* K >= 0 */
    int n_max;        /* >= 0 */
    int point_stride; /* >= 3 */
    int overlap;      /* LISO_OVERLAP_* */
    int keep_flow;
    int no_label;
} liso_flow_labels_cfg;

size_t liso_flow_labels_workspace_bytes(int n_jobs, int n_boxes); /* 0 for arguments the call refuses */

int liso_flow_labels_f32(const liso_flow_labels_cfg* cfg, const float* pcl, const int32_t* counts, const int32_t* cloud_of,
                         const double* odom, const double* pose_a, const double* pose_b, const double* size, const uint8_t* valid,
                         const uint8_t* has_b, const int32_t* label, const int32_t* box_class, const int32_t* point_class, float* flow,
                         int32_t* point_label, int32_t* point_box, int32_t* count, void* workspace, size_t workspace_bytes,
                         void* stream);

/* 2. KITTI's lidar row and column of every point of a padded batch [B, n_max, point_stride]: find_jumps and find_cols.  Per cloud,
 *   over its rows in file order:
 *     az[i]   = -(float)atan2((double)y, (double)(-x))
 *     jump[i] = i >= 1 && (az[i] - az[i - 1]) < (float)threshold                       (the difference and the comparison in fp32)
 *     rows[i] = jump[0] + ... + jump[i]; with auto_correct and rows[count - 1] < 63, 63 - rows[count - 1] is added to every row
 *     cols[i] = int32(trunc(((float)(num_columns - 1) * ((float)pi - (float)atan2((double)y, (double)x))) / (float)(2 pi)))  in fp32
 *   rows and cols int32 [B, n_max] (either may be NULL, not both); entries at or behind the count are -1.  One launch, one
 *   workgroup per cloud walking tiles of its rows and carrying the running sum.
 *   The builders call numpy's float32 arctan2; atan2 is evaluated here in fp64 and rounded to fp32, so an azimuth can differ from
 *   numpy's in its last bit.  That changes an output only for a point whose azimuth difference lies within a few ulp of the
 *   threshold or whose column value lies within a few ulp of an integer. */
int liso_kitti_rows_cols_f32(int batch, int n_max, int point_stride, const float* pcl, const int32_t* counts, double threshold,
                             int auto_correct, int num_columns, int32_t* rows, int32_t* cols, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LISO_FLOW_LABELS_H */
