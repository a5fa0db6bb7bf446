// Box-snippet augmentation kernels for gfx950.  C ABI + reference lines: include/liso_augment.h.
//
// The per-sweep entry points: one launch geometry around the bodies of box_augment_bodies.h (the batched call with device draws,
// box_augment_batch.hip, runs the same bodies).  Free mask: HBM traffic = the n coordinate pairs once + h * w mask bytes once (the
// byte map and its 2r + 1-fold re-reads stay in L2: 256 KB at 512^2).  Paste: one block per pasted object (<= 15 per sample, a few
// hundred points each) -- the work is tiny, the point is that it happens where the sweep already lives.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/liso_augment.h"
#include "../../include/liso_iou3d.h"
#include "box_augment_bodies.h"
#include "zero_fill.h"
#include "per_device.h"

namespace {

using namespace liso_augment_dev;

__global__ __launch_bounds__(kThreads) void occupancy_bytes_kernel(const int32_t* __restrict__ coors, long n, int h, int w, int wp,
                                                                   uint8_t* __restrict__ occ) {
    const long i = (long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    mark_occupied(coors, i, h, w, wp, occ);
}

__global__ __launch_bounds__(kThreads) void free_mask_kernel(const uint8_t* __restrict__ occ, int h, int w, int words, int radius,
                                                             uint8_t* __restrict__ free_mask, int* __restrict__ row_count) {
    extern __shared__ unsigned long long lds_bits[];  // [(2r + 1) rows][words]
    free_mask_row(occ, h, w, words, radius, blockIdx.x, lds_bits, free_mask, row_count);
}

__global__ __launch_bounds__(kThreads) void row_prefix_kernel(int* __restrict__ prefix, int h) { row_prefix_block(prefix, h); }

// one wavefront per query
__global__ __launch_bounds__(64) void select_free_cells_kernel(const uint8_t* __restrict__ free_mask, const int* __restrict__ prefix, int h,
                                                               int w, const int64_t* __restrict__ compact_idx, int k,
                                                               int* __restrict__ flat_cell) {
    const int q = blockIdx.x, lane = threadIdx.x;
    const int cell = select_free_cell_wave(free_mask, prefix, h, w, compact_idx[q], lane);
    if (lane == 0) flat_cell[q] = cell;
}

// one block per pasted object
__global__ __launch_bounds__(kThreads) void snippet_paste_kernel(const float4* __restrict__ db_points, long db_rows,
                                                                 const int64_t* __restrict__ src_index, const int64_t* __restrict__ out_offsets,
                                                                 const double* __restrict__ pose, const double* __restrict__ flow_rand,
                                                                 double vmin, double vmax, float4* __restrict__ out_points,
                                                                 float* __restrict__ out_flow, float* __restrict__ box_velo) {
    const int obj = blockIdx.x;
    paste_object(db_points, db_rows, src_index, out_offsets[obj], out_offsets[obj + 1], pose + obj * 12, FlowRandTable{flow_rand}, vmin, vmax,
                 out_points, out_flow, box_velo + obj);
}

}  // namespace

extern "C" {

size_t liso_bev_free_mask_workspace_bytes(int h, int w) {
    if (h <= 0 || w <= 0) return 0;
    return (size_t)h * words_per_row(w) * 64;  // the occupancy byte map, rows padded to 64 cells
}

int liso_bev_free_mask(const int32_t* pillar_coors, long n, int h, int w, int radius, uint8_t* free_mask, int32_t* row_free_prefix,
                       void* workspace, size_t workspace_bytes, void* stream) {
    if (h <= 0 || w <= 0 || n < 0 || radius < 0 || radius > kMaxRadius || !free_mask || !row_free_prefix || !workspace) return LISO_EINVAL;
    if (n > 0 && !pillar_coors) return LISO_EINVAL;
    if (((uintptr_t)pillar_coors & 7) || ((uintptr_t)workspace & 7)) return LISO_EINVAL;
    if (workspace_bytes < liso_bev_free_mask_workspace_bytes(h, w)) return LISO_EWORKSPACE;
    const int words = words_per_row(w);
    const size_t lds = (size_t)(2 * radius + 1) * words * sizeof(unsigned long long);
    if (lds > 120 * 1024) return LISO_EINVAL;  // (radius 255 on a 1024-wide grid = 65 KB)
    hipStream_t st = (hipStream_t)stream;
    static liso_dev::PerDeviceFlag attr_set;
    if (!liso_dev::lds_opt_in(attr_set, (const void*)free_mask_kernel, 120 * 1024)) return LISO_ELAUNCH;
    uint8_t* occ = (uint8_t*)workspace;
    if (liso_zero::zero_async(occ, liso_bev_free_mask_workspace_bytes(h, w), st) != hipSuccess) return LISO_ELAUNCH;
    if (n > 0) occupancy_bytes_kernel<<<(unsigned)((n + kThreads - 1) / kThreads), kThreads, 0, st>>>(pillar_coors, n, h, w, words * 64, occ);
    free_mask_kernel<<<h, kThreads, lds, st>>>(occ, h, w, words, radius, free_mask, row_free_prefix + 1);
    row_prefix_kernel<<<1, kThreads, 0, st>>>(row_free_prefix, h);
    return hipGetLastError() == hipSuccess ? LISO_OK : LISO_ELAUNCH;
}

int liso_bev_select_free_cells(const uint8_t* free_mask, const int32_t* row_free_prefix, int h, int w, const int64_t* compact_idx, int k,
                               int32_t* flat_cell, void* stream) {
    if (h <= 0 || w <= 0 || k < 0 || !free_mask || !row_free_prefix) return LISO_EINVAL;
    if (k == 0) return LISO_OK;
    if (!compact_idx || !flat_cell) return LISO_EINVAL;
    select_free_cells_kernel<<<k, 64, 0, (hipStream_t)stream>>>(free_mask, row_free_prefix, h, w, compact_idx, k, flat_cell);
    return hipGetLastError() == hipSuccess ? LISO_OK : LISO_ELAUNCH;
}

int liso_snippet_paste(const float* db_points, long db_rows, const int64_t* src_index, const int64_t* out_offsets, const double* pose,
                       const double* flow_rand, double vmin, double vmax, int k, float* out_points, float* out_flow, float* box_velo,
                       void* stream) {
    if (k < 0 || db_rows < 0) return LISO_EINVAL;
    if (k == 0) return LISO_OK;
    if (!db_points || !src_index || !out_offsets || !pose || !flow_rand || !out_points || !box_velo) return LISO_EINVAL;
    if (((uintptr_t)db_points | (uintptr_t)out_points) & 15) return LISO_EINVAL;
    snippet_paste_kernel<<<k, kThreads, 0, (hipStream_t)stream>>>((const float4*)db_points, db_rows, src_index, out_offsets, pose, flow_rand,
                                                                   vmin, vmax, (float4*)out_points, out_flow, box_velo);
    return hipGetLastError() == hipSuccess ? LISO_OK : LISO_ELAUNCH;
}

}  // extern "C"
