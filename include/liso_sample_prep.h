/*
 * liso_sample_prep.h -- C ABI of the per-sample preparation between ground removal and the collated batch, on the device:
 * the geometric augmentation (one rigid / scaled transform applied to clouds, flows, boxes and odometries), the crop to the BEV
 * range with one order-preserving compaction of everything that rides with the cloud, and the BEV maps and the moving mask of
 * the compacted rows.  No host synchronisation (graph-capturable).
 *
 * Replaces, in liso/datasets/torch_dataset_commons.py: augment_sample_content (:1291-1433), augment_objects_from_category_with_trafo
 * (:1435-1462), transform_pcl_maybe_with_intensity (:1464-1483), pillarize_bev (:1147-1163) with voxelize_sample (:975-987),
 * add_bev_flow (:1200-1213), add_bev_ground_height_occupancy_maps (:1215-1223) and the moving_mask expression of :776-792.
 *
 * Conventions (as include/liso_ground.h): device pointers, caller-allocated outputs, no allocation, no host synchronisation; every
 * entry point checks its arguments before it launches anything and returns LISO_OK, LISO_EINVAL, LISO_EWORKSPACE or LISO_ELAUNCH.
 * Clouds are rows of a [B, n_max, point_stride] fp32 array (x, y, z first); cloud b has counts[b] rows (counts == NULL: n_max
 * each).  A row with a NaN coordinate is invalid and takes no part.  The source file is compiled without FMA contraction: every
 * expression below is evaluated in fp64, operation by operation, in the order written.
 */
#ifndef LISO_SAMPLE_PREP_H
#define LISO_SAMPLE_PREP_H

#include <stddef.h>
#include <stdint.h>

#include "liso_iou3d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LISO_SAMPLE_MAX_N (1 << 24)     /* rows per cloud */
#define LISO_SAMPLE_MAX_JOBS 16         /* box arrays / odometries per liso_sample_transform_poses_f64 call */
#define LISO_SAMPLE_MAX_CELLS (1 << 24) /* grid_x * grid_y */

/* 1. One cloud array and (optionally) its flow under T (fp64 [B, 16], row-major 4x4, device memory).
 *   x' = ((T00*x + T01*y) + T02*z) + T03, likewise y', z', in fp64 from the widened fp32 inputs, rounded once to fp32; channels 3
 *   and up are copied.  flow (fp32 [B, n_max, 3] or NULL) takes the linear part only: fx' = (T00*fx + T01*fy) + T02*fz.
 *   Invalid rows come out with NaN coordinates and NaN flow, rows behind counts[b] with NaN in every channel.
 *   out_pcl may be pcl and out_flow may be flow (in place); any other overlap is refused or undefined. */
int liso_sample_transform_f32(int batch, int n_max, int point_stride, const double* T, const float* pcl, const int32_t* counts,
                              const float* flow, float* out_pcl, float* out_flow, void* stream);

/* 2. The small tensors under T.  Host arrays of jobs, at most LISO_SAMPLE_MAX_JOBS of each kind, one launch.
 *   Boxes [B, k]: pose = (pos, yaw about z); P = T * pose in fp64, each entry a fused multiply-add chain along the row as the
 *   reference's matrix product evaluates it; pos' = P[:, 3] (the first pos_dim entries), yaw' =
 *   atan2(P[1][0], P[0][0]); stored back in the dtype they came in (is_f64 selects fp64 / fp32).  Boxes with valid == 0 stay.
 *   Odometries fp64 [B, 4, 4]: out = T * O * T^-1, out_inv = out^-1, both inverses in closed form for an affine matrix (adjugate
 *   of the 3x3 block, -A^-1 t; last row 0 0 0 1).  out may be in; out_inv may be NULL. */
typedef struct {
    void* pos;            /* [B, k, pos_dim] */
    void* rot;            /* [B, k, 1] */
    const uint8_t* valid; /* [B, k] or NULL (all valid) */
    int k;                /* >= 0 */
    int pos_dim;          /* 2 or 3 */
    int is_f64;           /* 0: fp32, 1: fp64 */
} liso_sample_box_job;

typedef struct {
    const double* in; /* [B, 16] */
    double* out;      /* [B, 16] */
    double* out_inv;  /* [B, 16] or NULL */
} liso_sample_odom_job;

int liso_sample_transform_poses_f64(int batch, const double* T, const liso_sample_box_job* boxes, int n_boxes,
                                    const liso_sample_odom_job* odoms, int n_odoms, void* stream);

/* 3. Pillar coordinates and the crop.  Per valid row, in fp64: c = ((p + 0.5 * range) / range) * grid truncated to int32, with
 *   range_z = 1000 and grid_z = 1; inside = 0 <= c < grid on all three axes and z_min < z < z_max (open; +-infinity allowed).  The
 *   truncation keeps points up to one cell outside the negative edge, with coordinate 0, as the reference does.  A row is kept
 *   when it is inside and drop[b][i] == 0 (drop NULL: none dropped).  Kept rows move, in order, to the front of every output:
 *   out_pcl (NaN behind), out_flow fp32 [.,3] (NaN behind), out_lidar_rows int32 (0 behind), out_attr uint8 (0 behind),
 *   pillar_coors int32 [B, n_max, 2] (-1 behind); out_counts[b] = number of kept rows.  flow / lidar_rows / attr and their outputs
 *   are optional, pairwise.  Not in place. */
typedef struct {
    int batch;        /* B >= 1 */
    int n_max;        /* rows per cloud, >= 0 */
    int point_stride; /* floats per row, >= 3 */
    int grid_x;       /* > 0; pillar_coors[..., 0] */
    int grid_y;       /* > 0; pillar_coors[..., 1] */
    double range_x;   /* > 0, metres */
    double range_y;   /* > 0 */
    double z_min;     /* open height interval; -infinity / +infinity for none */
    double z_max;
} liso_bev_crop_cfg;

size_t liso_bev_crop_workspace_bytes(int batch, int n_max);
int liso_bev_crop_f32(const liso_bev_crop_cfg* cfg, const float* pcl, const int32_t* counts, const uint8_t* drop, const float* flow,
                      const int32_t* lidar_rows, const uint8_t* attr, float* out_pcl, float* out_flow, int32_t* out_lidar_rows,
                      uint8_t* out_attr, int32_t* pillar_coors, int32_t* out_counts, void* workspace, size_t workspace_bytes,
                      void* stream);

/* 4. BEV maps and the moving mask of compacted rows (row i of cloud b takes part when i < counts[b] and its pillar coordinates
 *   lie in the grid).  Every output is optional.
 *   occupancy fp32 [B, 1, grid_x, grid_y]: 1 where a pillar has a point.
 *   flow_bev0 / flow_bev1 fp32 [B, grid_x, grid_y, 3]: per-cell mean of flow0 / flow1 (fp32 [B, n_max, 3]), 0 in empty cells.  The
 *   mean is order-independent and bitwise reproducible: per cell and component the largest magnitude is found with an integer
 *   atomic max, every value is then rounded to a multiple of 2^(E-38) (E = exponent of that maximum) and summed in int64; the
 *   mean is sum / count * 2^(E-38) in fp64, rounded once to fp32.  It lies within 2^-23 * max|v| of the exact mean.  A cell that
 *   holds a non-finite value gets NaN in that component.
 *   moving_mask uint8 [B, n_max]: ||(odom_tb_ta - I) * (x, y, z, 1) - flow0|| > threshold_dt in fp64, 0 behind the count; needs
 *   pcl, flow0 and odom_tb_ta (fp64 [B, 16]). */
size_t liso_bev_point_maps_workspace_bytes(int batch, int grid_x, int grid_y, int n_flows);
int liso_bev_point_maps_f32(int batch, int n_max, int point_stride, int grid_x, int grid_y, const float* pcl, const int32_t* counts,
                            const int32_t* pillar_coors, const float* flow0, const float* flow1, const double* odom_tb_ta,
                            double threshold_dt, float* occupancy, float* flow_bev0, float* flow_bev1, uint8_t* moving_mask,
                            void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LISO_SAMPLE_PREP_H */
