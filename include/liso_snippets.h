/*
 * liso_snippets.h -- C ABI of the box-snippet harvest on the device: the points of a sweep that lie inside a (slightly bloated)
 * tracked box, in box coordinates, for many (sweep, box) jobs in one call.  No host synchronisation (graph-capturable).
 *
 * Replaces the per-track, per-frame Python loops of track_boxes_on_data_sequence in liso/tracker/tracking.py that cut the
 * augmentation database out of a mined sequence: :1568-1610 (tracked branch) and :1848-1891 (NotATracker branch), i.e. per
 * snippet inv(sensor_T_box) times the whole sweep in fp64, a boolean mask over the sweep and a device-to-host copy.
 *
 * Conventions (as include/liso_sample_prep.h): device pointers, caller-allocated outputs, no allocation, no host synchronisation;
 * the entry point checks its arguments before it launches anything and returns LISO_OK, LISO_EINVAL, LISO_EWORKSPACE or
 * LISO_ELAUNCH.  The source file is compiled without FMA contraction: every expression below is evaluated operation by operation,
 * in the order written.
 */
#ifndef LISO_SNIPPETS_H
#define LISO_SNIPPETS_H

#include <stddef.h>
#include <stdint.h>

#include "liso_iou3d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LISO_SNIPPET_MAX_N (1 << 24)    /* rows per sweep */
#define LISO_SNIPPET_MAX_CLOUDS 65535   /* sweeps per call */
#define LISO_SNIPPET_MAX_JOBS (1 << 16) /* snippets per call */

/* Cuts n_jobs snippets.  Job j takes the rows of sweep job_cloud[j] that lie inside box job_boxes[j].
 *
 *   clouds      fp32 [n_clouds, n_max, point_stride]: x, y, z first, intensity LAST, point_stride >= 4.
 *   counts      int32 [n_clouds] or NULL (n_max rows each); clamped to [0, n_max].  A row behind the count, or with a NaN
 *               coordinate, lies in no box.
 *   lidar_rows  int32 [n_clouds, n_max] or NULL; given exactly when out_rows is given.
 *   job_cloud   int32 [n_jobs], device memory.  An index outside [0, n_clouds) yields an empty snippet and reads nothing.
 *   job_boxes   fp32 [n_jobs, 7]: x, y, z, dx, dy, dz, yaw (the dense layout of liso_iou3d.h).  A row that holds NaN contains no
 *               point.
 *
 * Pose: box_T_sensor = inv(sensor_T_box) of the yaw-only pose of Shape.get_poses (liso/kabsch/shape_utils.py:271-319), in closed
 * form in fp64 from the widened fp32 box, c = cos(yaw), s = sin(yaw):
 *     [ c  s  0  -(c*x + s*y) ]
 *     [-s  c  0   (s*x - c*y) ]
 *     [ 0  0  1  -z           ]
 *     [ 0  0  0   1           ]
 * Inside test (tracking.py:1575-1592): per row r of that matrix p_box[r] = ((m0*px + m1*py) + m2*pz) + m3 in fp64 from the widened
 * fp32 point, rounded once to fp32; the point is inside when fabsf(p_box[r]) <= 0.55f * dims[r] on all three axes -- an fp32
 * product, an INCLUSIVE comparison (liso_points_in_boxes_f32 is strict and bloats differently).
 *
 * Outputs:
 *   out_offsets        int64 [n_jobs + 1]: exclusive prefix sum of the per-job point counts; always the TRUE totals, also where they
 *                      exceed `capacity`.
 *   out_points         fp32 [capacity, 4]: p_box x, y, z and the untouched intensity.  Job j owns rows [offsets[j], offsets[j+1]);
 *                      its points keep the order they have in the sweep.  Rows at or beyond `capacity` are never written: a caller
 *                      that sees offsets[n_jobs] > capacity calls again with larger buffers.  NULL with capacity 0: count only.
 *   out_rows           int32 [capacity] or NULL: lidar_rows of the same points, same order.
 *   out_box_T_sensor   fp64 [n_jobs, 16], row-major, or NULL.
 * The result is bit-identical from run to run: positions come from per-chunk counts, a scan and a wave ballot, not from atomics.
 * Every sweep is read once per pass (count, move) for all the jobs that name it. */
size_t liso_snippet_cut_workspace_bytes(int n_clouds, int n_max, int n_jobs);
int liso_snippet_cut_f32(int n_clouds, int n_max, int point_stride, const float* clouds, const int32_t* counts,
                         const int32_t* lidar_rows, int n_jobs, const int32_t* job_cloud, const float* job_boxes, long capacity,
                         int64_t* out_offsets, float* out_points, int32_t* out_rows, double* out_box_T_sensor, void* workspace,
                         size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LISO_SNIPPETS_H */
