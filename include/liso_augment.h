/* Box-snippet augmentation on the device (second half).
 *
 * Replaces the numpy / scikit-image body of LidarDataset.create_augmented_sample_from_box_snippet_db
 * (liso/datasets/torch_dataset_commons.py:1531-1776), which the reference runs per sample in DataLoader workers:
 *   - the "where may an object centre go" mask: BEV occupancy of the sweep, dilated with a disk, inverted  (:1538-1557)
 *   - picking the drawn free cells out of the row-major list of free cells                                 (:1558-1563)
 *   - pasting the drawn snippets: per-point gather from the snippet database, rigid pose x flip x scale in float64,
 *     artificial per-point flow and the box speed = mean |flow|                                             (:1597-1690)
 * For these three per-sweep entry points the random draws stay with the caller (liso_amd/datasets/box_augmentation.py draws them
 * in the reference's order so seeded runs reproduce the reference).  The batched entries further down make the draws on the device.
 *
 * Plain C ABI: device pointers, sizes, a hipStream_t passed as void*.  Return 0 = LISO_OK, else the codes of liso_iou3d.h.
 */
#ifndef LISO_AUGMENT_H
#define LISO_AUGMENT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* bytes of scratch for liso_bev_free_mask (the occupancy byte map) */
size_t liso_bev_free_mask_workspace_bytes(int h, int w);

/* free_mask[i * w + j] = 1 iff no occupied BEV cell (i', j') has (i - i')^2 + (j - j')^2 <= radius^2
 * (= ~skimage.morphology.binary_dilation(occupancy, disk(radius)); cells outside the grid count as empty).
 *   pillar_coors   int32 [n, 2] (row, col) of every point of the sweep; rows with a coordinate outside the grid are ignored
 *   free_mask      uint8 [h * w]
 *   row_free_prefix int32 [h + 1]: exclusive prefix sum of the free cells per row; row_free_prefix[h] = number of free cells
 */
int liso_bev_free_mask(const int32_t* pillar_coors, long n, int h, int w, int radius, uint8_t* free_mask,
                       int32_t* row_free_prefix, void* workspace, size_t workspace_bytes, void* stream);

/* flat_cell[q] = i * w + j of the compact_idx[q]-th free cell in row-major order (what indexing
 * `pcl_bev_center_coords_homog_np[valid_mask][idx]` selects, :1558-1563); -1 when compact_idx[q] is out of range */
int liso_bev_select_free_cells(const uint8_t* free_mask, const int32_t* row_free_prefix, int h, int w,
                               const int64_t* compact_idx, int k, int32_t* flat_cell, void* stream);

/* Paste k snippets.  Object i owns the output rows [out_offsets[i], out_offsets[i + 1]).
 *   db_points    float32 [T, 4]   all snippets of the database, box coordinates + intensity, concatenated
 *   src_index    int64 [n_out]    database row of every output point (the caller's point drop-out / ray-drop selection)
 *   pose         float64 [k, 12]  rows 0..2 of sensor_T_box x diag(flip_x scale_x, flip_y scale_y, scale_z, 1)
 *   flow_rand    float64 [n_out, 3] uniform [0, 1) draws: flow = vmin + rand * (vmax - vmin)                (:1672-1677)
 *   out_points   float32 [n_out, 4] (float64 arithmetic, rounded once, like the reference's .astype(np.float32))
 *   out_flow     float32 [n_out, 3] or null
 *   box_velo     float32 [k]      mean over the object's points of |flow| (:1678-1682), fixed summation order
 */
int liso_snippet_paste(const float* db_points, long db_rows, const int64_t* src_index, const int64_t* out_offsets,
                       const double* pose, const double* flow_rand, double vmin, double vmax, int k, float* out_points,
                       float* out_flow, float* box_velo, void* stream);

/* ---- The batched call: B sweeps at once, every draw made on the device ------------------------------------------------------------
 * (liso_amd/csrc/box_augment_batch.hip; the draws, their packing into Philox4x32-10 counters and the sine / cosine routine are
 * written down in liso_amd/csrc/philox_draws.h, the whole call is restated in numpy by
 * liso_amd/datasets/batch_augmentation.py: paste_snippets_batch_host, and the two are equal bit for bit.)
 *
 * Six launches whatever the batch size and the number of drawn objects, no host read, no allocation, no memset node: capturable in a
 * hipGraph.  The generator state is read from DEVICE memory and the call's last launch adds 1 to its call counter, so every replay
 * of a captured call draws afresh. */
#define LISO_AUGMENT_MAX_OBJS 64     /* slots K of a sample: max_num_objs <= 64 (one lane per earlier object in the draw kernel) */
#define LISO_AUGMENT_MAX_ATTEMPTS 32 /* location attempts of one object */
#define LISO_AUGMENT_DRAW_COLS 16    /* columns of the `draws` record */

/* how the pasted rows of a snippet are chosen (reference :1598-1650) */
#define LISO_AUGMENT_SELECT_ALL 0
#define LISO_AUGMENT_SELECT_DROPOUT 1 /* a uniform random subset of num_keep rows, in database order */
#define LISO_AUGMENT_SELECT_RAYDROP 2 /* rows whose LiDAR row r has (r - start) mod nth == 0; all rows if that keeps none */

/* draws[b, slot, 15]: what became of the slot */
#define LISO_AUGMENT_SLOT_UNUSED 0      /* slot >= the drawn object count */
#define LISO_AUGMENT_SLOT_PASTED 1
#define LISO_AUGMENT_SLOT_NO_LOCATION 2 /* no free cell, or 32 attempts all hit an earlier object's cell */
#define LISO_AUGMENT_SLOT_OVERFLOW 3    /* the kept rows did not fit behind the earlier objects within extra_capacity */

typedef struct {
    int batch;                /* B >= 1 */
    int n_max;                /* rows per sample of pillar_coors */
    int h, w, radius;         /* BEV grid (first axis = x) and the dilation radius in cells */
    int max_num_objs;         /* K, 1..LISO_AUGMENT_MAX_OBJS: the object count is 1 + int(u K) */
    int num_snippets;         /* M >= 1 */
    long db_rows;             /* P */
    int extra_capacity;       /* E: rows per sample of extra_points */
    int selection;            /* LISO_AUGMENT_SELECT_* */
    double range_x, range_y;  /* bev_range_m (the fp32 values, widened) */
    double cell_x, cell_y;    /* size of one pillar in metres (the fp32 values, widened) */
    double max_scale_delta, max_points_dropout; /* max_points_dropout in [0, 1] */
    double vmin, vmax;        /* artificial object speed per flow component */
} liso_augment_batch_cfg;

/* the free masks of B sweeps: pillar_coors int32 [B, n_max, 2], of which the first counts[b] rows count (device memory);
 * free_mask uint8 [B, h, w], row_free_prefix int32 [B, h + 1]; per sample exactly liso_bev_free_mask.  4 launches. */
size_t liso_bev_free_mask_batch_workspace_bytes(int batch, int h, int w);
int liso_bev_free_mask_batch(const int32_t* pillar_coors, const int32_t* counts, int batch, int n_max, int h, int w, int radius,
                             uint8_t* free_mask, int32_t* row_free_prefix, void* workspace, size_t workspace_bytes, void* stream);

/* 0 for a configuration the call refuses */
size_t liso_snippet_augment_batch_workspace_bytes(const liso_augment_batch_cfg* cfg);

/* Free mask, draws, point selection and paste for B sweeps.
 *   pillar_coors, counts   as above (the clouds themselves are not read: liso_cloud_append_batch puts the pasted rows behind them)
 *   db_points   float32 [P, 4], db_offsets int64 [M + 1], db_dims float32 [M, 3], db_pos_z float32 [M],
 *   db_lidar_rows int32 [P] (needed by LISO_AUGMENT_SELECT_RAYDROP, else may be null)
 *   state       int64 [2] = (seed, calls) in device memory; calls += 1 by the last launch
 *   sample_ids  int64 [B]: the low 20 bits key the sample's draws
 * writes
 *   extra_points float32 [B, E, 4] (NaN behind extra_counts[b]), extra_flow float32 [B, E, 3] or null (likewise)
 *   extra_counts int32 [B], object_offsets int32 [B, K + 1]: slot s owns the rows [offsets[s], offsets[s + 1]) of its sample
 *   box_pos / box_dims float32 [B, K, 3], box_rot / box_velo float32 [B, K], box_valid uint8 [B, K] (zeros in a slot that is not pasted)
 *   draws       float64 [B, K, 16]: 0 flat cell (-1: none), 1 snippet, 2 theta, 3 z, 4 flip_x, 5 flip_y, 6..8 scales, 9 num_keep (drop-
 *               out) or nth (ray-drop), 10 start (ray-drop), 11 attempts, 12 x, 13 y (before rounding to fp32), 14 kept rows,
 *               15 LISO_AUGMENT_SLOT_*
 *   overflow    int32 [B]: objects dropped WHOLE because their kept rows did not fit within E behind the earlier objects
 *   kept_rows   int64 [B, E] or null: the database row of every pasted point
 * Arguments are checked before anything is launched. */
int liso_snippet_augment_batch(const liso_augment_batch_cfg* cfg, const int32_t* pillar_coors, const int32_t* counts, const float* db_points,
                               const int64_t* db_offsets, const float* db_dims, const float* db_pos_z, const int32_t* db_lidar_rows,
                               int64_t* state, const int64_t* sample_ids, float* extra_points, float* extra_flow, int32_t* extra_counts,
                               int32_t* object_offsets, float* box_pos, float* box_dims, float* box_rot, float* box_velo, uint8_t* box_valid,
                               double* draws, int32_t* overflow, int64_t* kept_rows, void* workspace, size_t workspace_bytes, void* stream);

/* out[b] = the first counts[b] rows of cloud[b], then the first extra_counts[b] rows of extra[b], then NaN rows; out_counts[b] = their
 * sum.  cloud float32 [B, n_max, cols], extra float32 [B, E, cols], out float32 [B, n_max + E, cols] (points: cols 4, flow: cols 3). */
int liso_cloud_append_batch(const float* cloud, const int32_t* counts, const float* extra, const int32_t* extra_counts, int batch, int n_max,
                            int extra_capacity, int cols, float* out, int32_t* out_counts, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LISO_AUGMENT_H */
