/*
 * liso_odometry.h -- C ABI of lidar odometry on the device: KISS-ICP style poses (w_T_lidar) for every frame of many padded
 * sequences of sweeps, with no host synchronisation (graph-capturable).
 *
 * Stands in for the third-party `kiss_icp` package the reference's dataset builders call (liso/datasets/kitti/create_kitti_raw.py:
 * 74-173, create_kitti_tracking.py:64-158, nuscenes/create.py:10-112,527-563) and for its `_correct_kitti_scan`
 * (create_kitti_raw.py:30-36).  Parity with that package is unpinned (its version in the reference's image is not fixed); the
 * formulation is the one stated in DESIGN.md and restated in numpy / fp64 by liso_amd/odometry/host.py, which is the yardstick.
 *
 * Per frame f, in this order on the caller's stream, one workgroup per sequence:
 *   preprocess   range filter on the fp64 norm, then two first-come voxel downsamples (keys floor(p / v) in fp64): frame_ds at
 *                0.5 * voxel_size from the sweep, source at 1.5 * voxel_size from frame_ds; both keep the input order
 *   register     guess from the constant-velocity model, adaptive threshold sigma, then the whole ICP loop in one launch: nearest
 *                map point over 27 voxels, 27 fp64 sums reduced in a fixed order, LDL^T and exp_se3 on one lane; model error
 *   map_update   frame_ds moved by the pose into the sequence's voxel map (<= max_points_per_voxel points per voxel, kept by input
 *                order), voxels whose first point lies beyond max_range of the sensor removed
 * All arithmetic that decides a key, a kept point or a stored value is fp64 evaluated operation by operation (the source file is
 * compiled without FMA contraction); the map stores fp32.
 *
 * The map of a sequence is two fixed-capacity open-addressing tables of `map_voxels` slots (a power of two): frame f builds table
 * f & 1 from the survivors of table (f + 1) & 1 and the frame's points.  A point whose voxel finds no slot (table full, or voxel
 * index outside +-2^20) is not inserted and counted in map_overflow.  Which slot a voxel lands in depends on the race between
 * lanes; the voxels held, their points and the points' order do not.
 *
 * Conventions (as include/liso_ground.h): device pointers, caller-allocated outputs, no allocation, no host synchronisation; every
 * entry point checks its arguments before it launches anything and returns LISO_OK, LISO_EINVAL, LISO_EWORKSPACE or LISO_ELAUNCH.
 * clouds fp32 [S, F, N, C] (x, y, z first), counts int32 [S, F] (NULL: N rows each), n_frames int32 [S]; frames at or beyond
 * n_frames[s] are skipped.  poses fp64 [S, F, 4, 4]; sigma fp64 [S, F]; n_source, n_iterations, converged int32 [S, F];
 * map_overflow int32 [S].
 */
#ifndef LISO_ODOMETRY_H
#define LISO_ODOMETRY_H

#include <stddef.h>
#include <stdint.h>

#include "liso_iou3d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LISO_ODOM_VOXEL_POINTS 20        /* fp32 points a map slot has room for: max_points_per_voxel <= this */
#define LISO_ODOM_MAX_N (1 << 22)        /* rows per sweep */
#define LISO_ODOM_MAX_MAP_VOXELS (1 << 24)
#define LISO_ODOM_KEY_HALF_SPAN (1 << 20) /* voxel indices lie in [-2^20, 2^20) per axis */
#define LISO_ODOM_N_LAYOUT 16            /* entries of liso_odometry_workspace_layout */

typedef struct {
    int n_seq;                /* S >= 0 */
    int max_frames;           /* F >= 1; S * F <= 2^24 */
    int n_max;                /* N >= 1, <= LISO_ODOM_MAX_N */
    int point_stride;         /* C: 3 or 4 */
    int map_voxels;           /* slots per table: a power of two in [64, LISO_ODOM_MAX_MAP_VOXELS] */
    int max_points_per_voxel; /* 1 .. LISO_ODOM_VOXEL_POINTS */
    int max_num_iterations;   /* >= 1 */
    double max_range;         /* > min_range */
    double min_range;         /* >= 0 */
    double voxel_size;        /* > 0; max_range / (0.5 * voxel_size) < LISO_ODOM_KEY_HALF_SPAN */
    double initial_threshold; /* > 0 */
    double min_motion_th;     /* >= 0 */
    double convergence_criterion; /* > 0 */
} liso_odometry_cfg;

/* bytes of device scratch (per-sequence state, tables and maps); 0 for a configuration that is refused. */
size_t liso_odometry_workspace_bytes(const liso_odometry_cfg* cfg);

/* Byte offsets of the workspace's tables, for tests and tools that look at a stage's result: offsets[0..] =
 * frame_ds fp32 [S,N,3], n_ds int32 [S], source fp32 [S,N,3], n_src int32 [S], map_keys uint64 [S,2,V], map_count int32 [S,2,V],
 * map_points fp32 [S,2,V,20,3], n_map_voxels int32 [S], sse fp64 [S], n_err int32 [S]; the rest 0.  A key is bit 63 set, then the
 * three voxel indices + 2^20 in 21 bits each (x highest); 0 is an empty slot. */
int liso_odometry_workspace_layout(const liso_odometry_cfg* cfg, size_t* offsets);

/* Stage 1 of frame `frame`: fills the workspace's frame_ds and source of every sequence, writes n_source[s][frame]. */
int liso_odometry_preprocess(const liso_odometry_cfg* cfg, int frame, const float* clouds, const int32_t* counts, const int32_t* n_frames,
                             int32_t* n_source, void* workspace, size_t workspace_bytes, void* stream);

/* Stage 2: registers the workspace's source against table (frame + 1) & 1 and writes poses / sigma / n_iterations / converged at
 * [s][frame].  guess fp64 [S,4,4] and sigma_given fp64 [S] both NULL: guess and threshold come from poses[s][< frame] and the
 * workspace's error sums, which the call then updates (frame 0 resets them).  Both given: they are used as they are and the sums are
 * left alone. */
int liso_odometry_register(const liso_odometry_cfg* cfg, int frame, const int32_t* n_frames, const double* guess, const double* sigma_given,
                           double* poses, double* sigma, int32_t* n_iterations, int32_t* converged, void* workspace, size_t workspace_bytes,
                           void* stream);

/* Stage 3: builds table frame & 1 from table (frame + 1) & 1 (taken as empty for frame 0) and frame_ds moved by poses[s][frame];
 * adds the points that found no slot to map_overflow[s] (frame 0 sets it). */
int liso_odometry_map_update(const liso_odometry_cfg* cfg, int frame, const int32_t* n_frames, const double* poses, int32_t* map_overflow,
                             void* workspace, size_t workspace_bytes, void* stream);

/* All frames of all sequences: identity poses and zeroed tables first, then the three stages frame by frame. */
int liso_odometry_sequences(const liso_odometry_cfg* cfg, const float* clouds, const int32_t* counts, const int32_t* n_frames, double* poses,
                            double* sigma, int32_t* n_source, int32_t* n_iterations, int32_t* converged, int32_t* map_overflow,
                            void* workspace, size_t workspace_bytes, void* stream);

/* out[k] = inv(a[k]) * b[k] for k < count, 4x4 row-major fp64 affine matrices; out may alias neither. */
int liso_odometry_relative_f64(int count, const double* a, const double* b, double* out, void* stream);

/* KITTI's vertical-angle correction: every row of points fp64 [n, 3] rotated by 0.205 degrees about normalize(p x e_z) (Rodrigues);
 * a row on the z axis (p x e_z == 0) is copied.  out may alias points. */
int liso_correct_kitti_scan_f64(long n, const double* points, double* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LISO_ODOMETRY_H */
