// Rotated-BEV IoU / overlap matrices and NMS for gfx950 (MI355X), C ABI in include/liso_iou3d.h.
//
// Semantics follow the reference's iou3d_nms (host twin iou3d_nms/src/iou3d_cpu.cpp:59-229,
// CUDA kernels iou3d_nms/src/iou3d_nms_kernel.cu:236-372, host greedy iou3d_nms/src/iou3d_nms.cpp:113-132);
// the structure is CDNA4-first and not a translation of those kernels:
//
//   * one wavefront == one 64-bit suppression word: a wave owns (row, 64 consecutive columns), each lane
//     tests one pair, __ballot() is the mask word.  The IoU/overlap matrices use the same mapping so the
//     64 results of a wave are one coalesced 256-B store.
//   * per-box work (sin/cos, rotated corners, in-box limits, a conservative bounding radius) is done once
//     per tile by one thread per box and parked in LDS, not once per pair.
//   * an exact early-out (bounding circles disjoint => the reference would find 0 polygon vertices and
//     return 0) removes the divergent polygon path for non-overlapping pairs.
//   * polygon vertices live in LDS laid out [slot][thread] (bank = thread, conflict-free for any slot), the
//     polar angle of each vertex is computed once, then the reference's bubble sort runs on the keys.
//   * the greedy sweep runs on the device: row-blocks of the bit-matrix are staged through LDS, one wave
//     resolves the 64-row diagonal dependency on scalar registers, all waves OR the kept rows into `remv`.
//     No D2H copy, no host loop, graph-capturable.
//
// The per-box geometry and the pair overlap live in rbev_geom.h (shared with det_nms.hip).
// Built with -ffp-contract=off: the geometry must round like the reference's host code (no FMA).
// sin/cos are evaluated in double and rounded to float, which matches glibc's sinf/cosf in practice.
#include <hip/hip_runtime.h>
#include "zero_fill.h"
#include "dev_common.h"
#include "rbev_geom.h"
#include "rbev_geom_host.h"
#include <math.h>
#include <stdint.h>

#include "../../include/liso_iou3d.h"

namespace {

using liso_dev::check_launch;

constexpr int kCols = 64;        // columns per tile == wavefront width == bits per mask word
constexpr int kRows = 16;        // rows per tile
constexpr int kThreads = 256;    // 4 waves, each owns kRows/4 rows

using namespace liso_rbev;
static_assert(kThreads == kPolyThreads, "PolyLds holds one column per thread");

// iou3d_nms_kernel.cu:314-326
__device__ __forceinline__ float iou_normal_dev(const float* a, const float* b) {
    const float left = fmaxf(a[0] - a[3] / 2, b[0] - b[3] / 2), right = fminf(a[0] + a[3] / 2, b[0] + b[3] / 2);
    const float top = fmaxf(a[1] - a[4] / 2, b[1] - b[4] / 2), bottom = fminf(a[1] + a[4] / 2, b[1] + b[4] / 2);
    const float w = fmaxf(right - left, 0.f), h = fmaxf(bottom - top, 0.f);
    const float inter = w * h;
    const float sa = a[3] * a[4], sb = b[3] * b[4];
    return inter / fmaxf(sa + sb - inter, kEps);
}

struct TileLds {
    float col[G_N][kCols];
    float row[G_N][kCols];  // only kRows used; same shape keeps one load_geo
    PolyLds poly;
};

__device__ __forceinline__ void stage_tile(TileLds& L, const float* __restrict__ boxes_r, int nr, int r0,
                                           const float* __restrict__ boxes_c, int nc, int c0) {
    const int t = threadIdx.x;
    if (t < kCols) {
        const int c = c0 + t;
        if (c < nc) store_geo(L.col, t, make_geo(boxes_c + (size_t)c * 7));
    } else if (t < kCols + kRows) {
        const int r = r0 + (t - kCols);
        if (r < nr) store_geo(L.row, t - kCols, make_geo(boxes_r + (size_t)r * 7));
    }
    __syncthreads();
}

// MODE 0: overlap area (boxes_overlap_kernel, .cu:236-249); MODE 1: IoU (boxes_iou_bev_kernel, .cu:251-265)
template <int MODE>
__global__ __launch_bounds__(kThreads) void pair_matrix_kernel(const float* __restrict__ a, int n,
                                                                const float* __restrict__ b, int m,
                                                                float* __restrict__ out) {
    __shared__ TileLds L;
    const int c0 = blockIdx.x * kCols, r0 = blockIdx.y * kRows;
    stage_tile(L, a, n, r0, b, m, c0);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = c0 + lane;
    if (c >= m) return;
    const Geo B = load_geo(L.col, lane);
#pragma unroll 1
    for (int rr = wave; rr < kRows; rr += kThreads / 64) {
        const int r = r0 + rr;
        if (r >= n) break;
        const Geo A = load_geo(L.row, rr);
        const float ov = box_overlap_dev(A, B, &L.poly, threadIdx.x);
        out[(size_t)r * m + c] = MODE == 0 ? ov : iou_from_overlap(A, B, ov);
    }
}

// suppression words, nms_kernel (.cu:267-311): bit i of mask[row][cb] <=> iou(row, cb*64+i) > thresh and col > row
__global__ __launch_bounds__(kThreads) void nms_mask_kernel(const float* __restrict__ boxes, int n, float thresh,
                                                             unsigned long long* __restrict__ mask, int col_blocks) {
    const int c0 = blockIdx.x * kCols, r0 = blockIdx.y * kRows;
    if (c0 + kCols - 1 <= r0) return;  // tile entirely on/below the diagonal: never read by the greedy pass
    __shared__ TileLds L;
    stage_tile(L, boxes, n, r0, boxes, n, c0);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = c0 + lane;
    Geo B;
    if (c < n) B = load_geo(L.col, lane);
#pragma unroll 1
    for (int rr = wave; rr < kRows; rr += kThreads / 64) {
        const int r = r0 + rr;
        if (r >= n) break;
        bool hit = false;
        if (c < n && c > r) {
            const Geo A = load_geo(L.row, rr);
            const float ov = box_overlap_dev(A, B, &L.poly, threadIdx.x);
            hit = iou_from_overlap(A, B, ov) > thresh;
        }
        const unsigned long long word = __ballot(hit);
        if (lane == 0) mask[(size_t)r * col_blocks + blockIdx.x] = word;
    }
}

// nms_normal_kernel (.cu:328-372)
__global__ __launch_bounds__(kThreads) void nms_normal_mask_kernel(const float* __restrict__ boxes, int n, float thresh,
                                                                    unsigned long long* __restrict__ mask,
                                                                    int col_blocks) {
    const int c0 = blockIdx.x * kCols, r0 = blockIdx.y * kRows;
    if (c0 + kCols - 1 <= r0) return;
    __shared__ float cb[kCols][7];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int i = threadIdx.x; i < kCols * 7; i += kThreads) {
        const int g = c0 * 7 + i;
        cb[i / 7][i % 7] = g < n * 7 ? boxes[g] : 0.f;
    }
    __syncthreads();
    const int c = c0 + lane;
    for (int rr = wave; rr < kRows; rr += kThreads / 64) {
        const int r = r0 + rr;
        if (r >= n) break;
        bool hit = false;
        if (c < n && c > r) hit = iou_normal_dev(boxes + (size_t)r * 7, cb[lane]) > thresh;
        const unsigned long long word = __ballot(hit);
        if (lane == 0) mask[(size_t)r * col_blocks + blockIdx.x] = word;
    }
}

// Device twin of the host greedy sweep (iou3d_nms.cpp:113-132).  One workgroup.
//   remv[]   : LDS, one word per column block
//   per row-block b: stage mask rows [64b, 64b+64) x words [b, col_blocks) into LDS; wave 0 walks the 64 rows
//   serially on the diagonal word (the only true dependency), then every thread ORs the kept rows' words
//   into remv for the column blocks to the right.
constexpr int kGreedyThreads = 256;
constexpr int kGreedyMaxLdsWords = 6 * 1024;  // 48 KiB of tile: col_blocks <= 96 (n <= 6144) staged via LDS, else L2 reads

__global__ __launch_bounds__(kGreedyThreads) void nms_greedy_kernel(const unsigned long long* __restrict__ mask, int n,
                                                                    int col_blocks, long long* __restrict__ keep,
                                                                    int* __restrict__ num_out) {
    extern __shared__ unsigned long long lds[];
    unsigned long long* remv = lds;                 // [col_blocks]
    unsigned long long* tile = lds + col_blocks;    // [64][w] with w = col_blocks - b, or unused when !use_lds
    __shared__ unsigned long long kept_word;
    const bool use_lds = (size_t)col_blocks * 64 <= (size_t)kGreedyMaxLdsWords;
    const int tid = threadIdx.x, lane = tid & 63;
    for (int i = tid; i < col_blocks; i += kGreedyThreads) remv[i] = 0ULL;
    int total = 0;  // meaningful in wave 0 only
    __syncthreads();
    for (int b = 0; b < col_blocks; b++) {
        const int w = col_blocks - b;
        const int rbase = b * 64;
        if (use_lds) {
            for (int idx = tid; idx < 64 * w; idx += kGreedyThreads) {
                const int r = idx / w, cw = idx - r * w;
                const int row = rbase + r;
                tile[idx] = row < n ? mask[(size_t)row * col_blocks + b + cw] : 0ULL;
            }
            __syncthreads();
        }
        if (tid < 64) {
            const int row = rbase + lane;
            unsigned long long diag = 0ULL;
            if (row < n) diag = use_lds ? tile[lane * w] : mask[(size_t)row * col_blocks + b];
            const unsigned long long cur_v = remv[b];
            // wave-uniform: keep the serial chain on the scalar unit
            // (readfirstlane returns int: go through unsigned int so bit 31 is not sign-extended)
            const unsigned int cur_lo = (unsigned int)__builtin_amdgcn_readfirstlane((unsigned int)cur_v);
            const unsigned int cur_hi = (unsigned int)__builtin_amdgcn_readfirstlane((unsigned int)(cur_v >> 32));
            unsigned long long cur = ((unsigned long long)cur_hi << 32) | (unsigned long long)cur_lo;
            const int valid = n - rbase;  // rows >= n are never kept
            if (valid < 64) cur |= ~0ULL << valid;
            unsigned long long kept = 0ULL;
#pragma unroll
            for (int t = 0; t < 64; t++) {
                const unsigned int lo = (unsigned int)__builtin_amdgcn_readlane((unsigned int)diag, t);
                const unsigned int hi = (unsigned int)__builtin_amdgcn_readlane((unsigned int)(diag >> 32), t);
                const unsigned long long d = ((unsigned long long)hi << 32) | lo;
                if (!((cur >> t) & 1ULL)) {
                    kept |= 1ULL << t;
                    cur |= d;
                }
            }
            if ((kept >> lane) & 1ULL) keep[total + __popcll(kept & ((1ULL << lane) - 1ULL))] = row;
            total += __popcll(kept);
            if (lane == 0) kept_word = kept;
        }
        __syncthreads();
        const unsigned long long kept = kept_word;
        for (int cw = 1 + tid; cw < w; cw += kGreedyThreads) {
            unsigned long long acc = remv[b + cw];
            unsigned long long k = kept;
            while (k) {
                const int t = __ffsll((long long)k) - 1;
                k &= k - 1;
                acc |= use_lds ? tile[t * w + cw] : mask[(size_t)(rbase + t) * col_blocks + b + cw];
            }
            remv[b + cw] = acc;
        }
        __syncthreads();
    }
    if (tid == 0) *num_out = total;
}

template <int MODE>
int launch_pair_matrix(const float* a, int n, const float* b, int m, float* out, void* stream) {
    if (n < 0 || m < 0) return LISO_EINVAL;
    if (n == 0 || m == 0) return LISO_OK;
    if (!a || !b || !out) return LISO_EINVAL;
    dim3 grid((m + kCols - 1) / kCols, (n + kRows - 1) / kRows);
    hipLaunchKernelGGL(pair_matrix_kernel<MODE>, grid, dim3(kThreads), 0, (hipStream_t)stream, a, n, b, m, out);
    return check_launch();
}

int launch_nms(bool normal, const float* boxes, int n, float thresh, int64_t* keep, int* num_out, void* ws,
               size_t ws_bytes, void* stream) {
    if (n < 0 || !num_out) return LISO_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        if (liso_zero::zero_async(num_out, sizeof(int), st) != hipSuccess) return LISO_ELAUNCH;
        return LISO_OK;
    }
    if (!boxes || !keep || !ws) return LISO_EINVAL;
    if (ws_bytes < liso_iou3d_nms_workspace_bytes(n)) return LISO_EWORKSPACE;
    const int cb = (n + 63) / 64;
    auto* mask = (unsigned long long*)ws;
    dim3 grid(cb, (n + kRows - 1) / kRows);
    if (normal)
        hipLaunchKernelGGL(nms_normal_mask_kernel, grid, dim3(kThreads), 0, st, boxes, n, thresh, mask, cb);
    else
        hipLaunchKernelGGL(nms_mask_kernel, grid, dim3(kThreads), 0, st, boxes, n, thresh, mask, cb);
    if (check_launch() != LISO_OK) return LISO_ELAUNCH;
    const bool use_lds = (size_t)cb * 64 <= (size_t)kGreedyMaxLdsWords;
    const size_t lds_bytes = ((size_t)cb + (use_lds ? (size_t)cb * 64 : 0)) * sizeof(unsigned long long);
    hipLaunchKernelGGL(nms_greedy_kernel, dim3(1), dim3(kGreedyThreads), lds_bytes, st, mask, n, cb, (long long*)keep,
                       num_out);
    return check_launch();
}

// ---- host twin of boxes_iou_bev_cpu (iou3d_cpu.cpp:232-252): an explicitly-CPU entry point of the
// reference module, not a fallback for the device path.  The geometry lives in rbev_geom_host.h (shared with det_val.hip). ----
using liso_rbev_host::h_iou_bev;

}  // namespace

extern "C" {

int liso_iou3d_iou_bev_cpu_f32(const float* a, int n, const float* b, int m, float* out) {
    if (n < 0 || m < 0) return LISO_EINVAL;
    if (n == 0 || m == 0) return LISO_OK;
    if (!a || !b || !out) return LISO_EINVAL;
    for (int i = 0; i < n; i++)
        for (int j = 0; j < m; j++) out[(size_t)i * m + j] = h_iou_bev(a + (size_t)i * 7, b + (size_t)j * 7);
    return LISO_OK;
}

int liso_iou3d_overlap_bev_f32(const float* a, int n, const float* b, int m, float* out, void* stream) {
    return launch_pair_matrix<0>(a, n, b, m, out, stream);
}

int liso_iou3d_iou_bev_f32(const float* a, int n, const float* b, int m, float* out, void* stream) {
    return launch_pair_matrix<1>(a, n, b, m, out, stream);
}

size_t liso_iou3d_nms_workspace_bytes(int n) {
    if (n <= 0) return 0;
    return (size_t)n * (size_t)((n + 63) / 64) * sizeof(unsigned long long);
}

int liso_iou3d_nms_f32(const float* boxes, int n, float thresh, int64_t* keep_dev, int* num_out_dev, void* workspace,
                       size_t workspace_bytes, void* stream) {
    return launch_nms(false, boxes, n, thresh, keep_dev, num_out_dev, workspace, workspace_bytes, stream);
}

int liso_iou3d_nms_normal_f32(const float* boxes, int n, float thresh, int64_t* keep_dev, int* num_out_dev,
                              void* workspace, size_t workspace_bytes, void* stream) {
    return launch_nms(true, boxes, n, thresh, keep_dev, num_out_dev, workspace, workspace_bytes, stream);
}

}  // extern "C"
