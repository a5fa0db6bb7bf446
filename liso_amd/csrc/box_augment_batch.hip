// Box-snippet augmentation of a whole batch with the draws made on the device.  C ABI: include/liso_augment.h (the batched entries).
//
// SIX launches for any batch size B and any number of drawn objects, no host read, no allocation, no memset node, no library scan or
// sort (utils/graph_capture.py, zero_fill.h): capturable, and every replay draws afresh because the generator state is read from
// device memory and advanced by the last launch.
//   1 zero the B occupancy byte maps          2 scatter the B sweeps' pillar coordinates (counts from device memory)
//   3 free mask, one block per (sample, row)  4 row prefix, one block per sample                  -- bodies of box_augment_bodies.h
//   5 draws: one WAVEFRONT per sample.  Object count, then slot by slot (location acceptance is sequential: an attempt is taken when
//     its index among the free cells differs from every earlier object's): 32 attempts drawn by 32 lanes, one ballot; the accepted
//     index -> cell through select_free_cell_wave; snippet, height, heading (own sine / cosine, philox_draws.h), flips, scales,
//     the point selection's parameters and its kept count (ray-drop: the lanes count the snippet's LiDAR rows); the fit test against
//     the capacity E and the running offset; pose, box table and the `draws` record.
//   6 selection + paste: one block per (sample, slot).  Drop-out keeps the num_keep smallest (key, j) pairs, key = Philox(j): a radix
//     SELECT on the key (four 8-bit LDS histograms over keys that are recomputed, not stored, so no cap on the snippet size) gives
//     the threshold key and how many of its ties to take, a stable ballot compaction writes the kept database rows in database
//     order, and paste_object (the per-sweep body) pastes them with Philox flow draws.  The tail behind the sample's count is filled
//     with NaN by the same blocks, and block (0, 0) advances the call counter: nothing in this launch reads the state tensor
//     (launch 5 left a copy of it in the workspace).
// All fp64 expressions are evaluated operation by operation (-ffp-contract=off; the paste body names its fused operations) and
// restated in numpy by liso_amd/datasets/batch_augmentation.py: paste_snippets_batch_host equals this file bit for bit.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/liso_augment.h"
#include "../../include/liso_iou3d.h"
#include "box_augment_bodies.h"
#include "per_device.h"
#include "philox_draws.h"
#include "zero_fill.h"

namespace {

using namespace liso_augment_dev;
namespace D = liso_draws;

constexpr int kMaxObjs = LISO_AUGMENT_MAX_OBJS;
constexpr int kAttempts = LISO_AUGMENT_MAX_ATTEMPTS;
constexpr int kDrawCols = LISO_AUGMENT_DRAW_COLS;
constexpr int kLdsLimit = 120 * 1024;

size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

// ---- launches 2-4: the free mask of every sample -------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void occupancy_batch_kernel(const int32_t* __restrict__ coors, const int32_t* __restrict__ counts,
                                                                   int n_max, int h, int w, int wp, uint8_t* __restrict__ occ) {
    const int b = blockIdx.y;
    const long i = (long)blockIdx.x * kThreads + threadIdx.x;
    int n = counts[b];
    n = n < 0 ? 0 : (n > n_max ? n_max : n);
    if (i >= n) return;
    mark_occupied(coors + (size_t)b * n_max * 2, i, h, w, wp, occ + (size_t)b * h * wp);
}

__global__ __launch_bounds__(kThreads) void free_mask_batch_kernel(const uint8_t* __restrict__ occ, int h, int w, int words, int radius,
                                                                   uint8_t* __restrict__ free_mask, int* __restrict__ prefix) {
    extern __shared__ unsigned long long lds_bits[];  // [(2r + 1) rows][words]
    const int b = blockIdx.y;
    free_mask_row(occ + (size_t)b * h * words * 64, h, w, words, radius, blockIdx.x, lds_bits, free_mask + (size_t)b * h * w,
                  prefix + (size_t)b * (h + 1) + 1);
}

__global__ __launch_bounds__(kThreads) void row_prefix_batch_kernel(int* __restrict__ prefix, int h) {
    row_prefix_block(prefix + (size_t)blockIdx.x * (h + 1), h);
}

int launch_free_mask_batch(const int32_t* coors, const int32_t* counts, int B, int n_max, int h, int w, int radius, uint8_t* free_mask,
                           int32_t* prefix, uint8_t* occ, hipStream_t st) {
    const int words = words_per_row(w);
    const size_t lds = (size_t)(2 * radius + 1) * words * sizeof(unsigned long long);
    static liso_dev::PerDeviceFlag attr_set;
    if (!liso_dev::lds_opt_in(attr_set, (const void*)free_mask_batch_kernel, kLdsLimit)) return LISO_ELAUNCH;
    if (liso_zero::zero_async(occ, (size_t)B * h * words * 64, st) != hipSuccess) return LISO_ELAUNCH;
    const unsigned gx = (unsigned)((n_max + kThreads - 1) / kThreads);
    occupancy_batch_kernel<<<dim3(gx < 1 ? 1 : gx, B), kThreads, 0, st>>>(coors, counts, n_max, h, w, words * 64, occ);
    free_mask_batch_kernel<<<dim3(h, B), kThreads, lds, st>>>(occ, h, w, words, radius, free_mask, prefix);
    row_prefix_batch_kernel<<<B, kThreads, 0, st>>>(prefix, h);
    return hipGetLastError() == hipSuccess ? LISO_OK : LISO_ELAUNCH;
}

bool mask_geometry_ok(int B, int n_max, int h, int w, int radius) {
    if (B < 1 || B > 65535 || n_max < 0 || h <= 0 || w <= 0 || radius < 0 || radius > kMaxRadius) return false;
    if ((size_t)h * (size_t)w > ((size_t)1 << 30)) return false;  // flat cells are int32
    return (size_t)(2 * radius + 1) * words_per_row(w) * sizeof(unsigned long long) <= (size_t)kLdsLimit;
}

// ---- launch 5: the draws -------------------------------------------------------------------------------------------------------
struct Tables {
    liso_augment_batch_cfg c;
    const uint8_t* free_mask;    // [B, h, w]
    const int32_t* prefix;       // [B, h + 1]
    const int64_t* db_offsets;   // [M + 1]
    const float* db_dims;        // [M, 3]
    const float* db_z;           // [M]
    const int32_t* db_rows_lidar;  // [P] or null
    int64_t* state;              // (seed, calls)
    const int64_t* sample_ids;   // [B]
    int64_t* frozen;             // workspace copy of the state, read by launch 6
    double* pose;                // workspace [B, K, 12]
    int32_t* sel;                // workspace [B, K, 4]: snippet, p1 (num_keep | nth), p2 (start), flags (1 pasted, 2 keep all rows)
    int32_t* extra_counts;       // [B]
    int32_t* object_offsets;     // [B, K + 1]
    float *box_pos, *box_dims, *box_rot, *box_velo;
    uint8_t* box_valid;
    double* draws;               // [B, K, 16]
    int32_t* overflow;           // [B]
};

__global__ __launch_bounds__(64) void augment_draw_kernel(Tables t) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const liso_augment_batch_cfg& c = t.c;
    const int K = c.max_num_objs, h = c.h, w = c.w, E = c.extra_capacity;
    const int64_t seed = t.state[0], calls = t.state[1];
    if (lane == 0) t.frozen[0] = seed, t.frozen[1] = calls;  // (every block stores the same pair)
    const D::Stream s = D::make_stream(seed, calls, t.sample_ids[b]);
    const uint8_t* fm = t.free_mask + (size_t)b * h * w;
    const int32_t* pf = t.prefix + (size_t)b * (h + 1);
    const int num_free = pf[h];
    const int k = 1 + (int)D::below(D::uniform(s, D::kCount, 0, 0), K);
    int my_idx = -1;  // lane i: the accepted free-cell index of slot i
    int offset = 0, overflow = 0;
    if (lane == 0) t.object_offsets[(size_t)b * (K + 1)] = 0;
    for (int slot = 0; slot < K; slot++) {
        const size_t o = (size_t)b * K + slot;
        int attempts = 0, idx = -1, cell = -1;
        if (slot < k && num_free > 0) {
            int cand = -1;
            bool ok = false;
            if (lane < kAttempts) {
                cand = (int)D::below(D::uniform(s, D::kLocation, slot, lane), num_free);
                ok = true;
            }
            for (int j = 0; j < slot; j++)
                if (__shfl(my_idx, j, 64) == cand) ok = false;
            const unsigned long long taken = __ballot(ok);
            if (taken) {
                const int first = __ffsll((long long)taken) - 1;
                attempts = first + 1;
                idx = __shfl(cand, first, 64);
            } else {
                attempts = kAttempts;
            }
        }
        if (idx >= 0) {
            if (lane == slot) my_idx = idx;
            cell = select_free_cell_wave(fm, pf, h, w, idx, lane);
        }
        double rec[kDrawCols];
#pragma unroll
        for (int e = 0; e < kDrawCols; e++) rec[e] = 0.0;
        rec[0] = -1.0;
        rec[11] = (double)attempts;
        rec[15] = slot < k ? (double)LISO_AUGMENT_SLOT_NO_LOCATION : (double)LISO_AUGMENT_SLOT_UNUSED;
        float pos[3] = {0.f, 0.f, 0.f}, dims[3] = {0.f, 0.f, 0.f}, rot = 0.f;
        int flags = 0, snippet = 0, p1 = 0, p2 = 0;
        if (cell >= 0) {
            const int ci = cell / w, cj = cell - ci * w;
            // the cell centre as get_voxel_center_coords_m forms it (fp64, stored fp32), then the jitter inside the cell
            const float cx = (float)((((double)ci + 0.5) / (double)h) * c.range_x + (-0.5 * c.range_x));
            const float cy = (float)((((double)cj + 0.5) / (double)w) * c.range_y + (-0.5 * c.range_y));
            const double x = (double)cx + (0.5 - D::uniform(s, D::kJitter, slot, 0)) * c.cell_x;
            const double y = (double)cy + (0.5 - D::uniform(s, D::kJitter, slot, 1)) * c.cell_y;
            snippet = (int)D::below(D::uniform(s, D::kSnippet, slot, 0), c.num_snippets);
            const int64_t row0 = t.db_offsets[snippet];
            int64_t n64 = t.db_offsets[snippet + 1] - row0;
            if (row0 < 0 || n64 < 0 || row0 + n64 > c.db_rows) n64 = 0;  // (a broken offsets table pastes nothing)
            const int n = n64 > 0x7fffffff ? 0x7fffffff : (int)n64;
            const double z = 0.5 * (D::uniform(s, D::kHeight, slot, 0) - 0.5) + (double)t.db_z[snippet];
            const double ut = D::uniform(s, D::kHeading, slot, 0);
            const double theta = 6.283185307179586 * (ut - 0.5);
            double sn, cs;
            D::sincos_turn(ut, &sn, &cs);
            const double flip_x = D::uniform(s, D::kFlip, slot, 0) < 0.5 ? 1.0 : -1.0;
            const double flip_y = D::uniform(s, D::kFlip, slot, 1) < 0.5 ? 1.0 : -1.0;
            const double sx = 1.0 - c.max_scale_delta * (2.0 * D::uniform(s, D::kScale, slot, 0) - 1.0);
            const double sy = 1.0 - c.max_scale_delta * (2.0 * D::uniform(s, D::kScale, slot, 1) - 1.0);
            const double sz = 1.0 - c.max_scale_delta * (2.0 * D::uniform(s, D::kScale, slot, 2) - 1.0);
            int kept = n;
            if (c.selection == LISO_AUGMENT_SELECT_RAYDROP) {
                p1 = 1 + (int)D::below(D::uniform(s, D::kNth, slot, 0), 3);
                p2 = (int)D::below(D::uniform(s, D::kStart, slot, 0), p1);
                int mine = 0;
                for (int j = lane; j < n; j += 64) mine += ((t.db_rows_lidar[row0 + j] - p2) % p1 == 0) ? 1 : 0;
                for (int sft = 32; sft > 0; sft >>= 1) mine += __shfl_xor(mine, sft, 64);
                if (mine == 0) flags |= 2; else kept = mine;
            } else if (c.selection == LISO_AUGMENT_SELECT_DROPOUT) {
                const double share = 1.0 - D::uniform(s, D::kKeep, slot, 0) * c.max_points_dropout;
                const double want = (double)n * share;
                p1 = want >= 1.0 ? (want < 2147483647.0 ? (int)want : 0x7fffffff) : 1;
                kept = p1 < n ? p1 : n;
            }
            pos[0] = (float)x, pos[1] = (float)y, pos[2] = (float)z;
            rot = (float)theta;
            dims[0] = t.db_dims[3 * snippet + 0], dims[1] = t.db_dims[3 * snippet + 1], dims[2] = t.db_dims[3 * snippet + 2];
            const bool fits = (long)offset + kept <= (long)E;
            if (fits) flags |= 1; else overflow++;
            rec[0] = (double)cell, rec[1] = (double)snippet, rec[2] = theta, rec[3] = z, rec[4] = flip_x, rec[5] = flip_y;
            rec[6] = sx, rec[7] = sy, rec[8] = sz, rec[9] = (double)p1, rec[10] = (double)p2, rec[12] = x, rec[13] = y;
            rec[14] = (double)kept;
            rec[15] = fits ? (double)LISO_AUGMENT_SLOT_PASTED : (double)LISO_AUGMENT_SLOT_OVERFLOW;
            if (lane == 0) {
                const double ax = flip_x * sx, ay = flip_y * sy, tx = (double)pos[0], ty = (double)pos[1];
                double* m = t.pose + o * 12;
                m[0] = cs * ax, m[1] = -sn * ay, m[2] = 0.0, m[3] = tx;
                m[4] = sn * ax, m[5] = cs * ay, m[6] = 0.0, m[7] = ty;
                m[8] = 0.0, m[9] = 0.0, m[10] = sz, m[11] = 0.0;
            }
            if (fits) offset += kept;
        }
        if (lane == 0) {
            const bool pasted = (flags & 1) != 0;
            t.sel[o * 4 + 0] = snippet, t.sel[o * 4 + 1] = p1, t.sel[o * 4 + 2] = p2, t.sel[o * 4 + 3] = flags;
            t.object_offsets[(size_t)b * (K + 1) + slot + 1] = offset;
            for (int e = 0; e < 3; e++) {
                t.box_pos[o * 3 + e] = pasted ? pos[e] : 0.f;
                t.box_dims[o * 3 + e] = pasted ? dims[e] : 0.f;
            }
            t.box_rot[o] = pasted ? rot : 0.f;
            t.box_velo[o] = 0.f;  // (launch 6 writes the speed of a pasted object)
            t.box_valid[o] = pasted ? 1 : 0;
            for (int e = 0; e < kDrawCols; e++) t.draws[o * kDrawCols + e] = rec[e];
        }
    }
    if (lane == 0) {
        t.extra_counts[b] = offset;
        t.overflow[b] = overflow;
    }
}

// ---- launch 6: point selection and paste -----------------------------------------------------------------------------------------
struct PasteArgs {
    liso_augment_batch_cfg c;
    const float4* db_points;
    const int64_t* db_offsets;
    const int32_t* db_rows_lidar;
    int64_t* state;
    const int64_t* frozen;
    const int64_t* sample_ids;
    const double* pose;
    const int32_t* sel;
    const int32_t* extra_counts;
    const int32_t* object_offsets;
    int64_t* kept_rows;  // [B, E] database row of every pasted point
    float4* extra_points;
    float* extra_flow;
    float* box_velo;
};

struct FlowRandPhilox {
    D::Stream s;
    uint32_t slot;
    int64_t row0;
    __device__ __forceinline__ double operator()(long, int64_t src, int c) const {
        return D::uniform(s, D::kFlow, slot, 3u * (uint32_t)(src - row0) + (uint32_t)c);
    }
};

// Stable compaction by one block: row j of the snippet is kept when code(j) = 1, or when code(j) = 2 and fewer than `ties` rows with
// code 2 precede it; the kept rows go to dst[0 .. cap) in ascending j as database rows row0 + j.
template <class Code>
__device__ __forceinline__ void compact_rows(int n, Code code, int ties, int64_t row0, int64_t* __restrict__ dst, int cap) {
    __shared__ int wave_keep[kThreads / 64], wave_tie[kThreads / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long below_me = (1ull << lane) - 1ull;
    int carry_keep = 0, carry_tie = 0;
    for (int base = 0; base < n; base += kThreads) {
        const int j = base + threadIdx.x;
        const int cd = j < n ? code(j) : 0;
        const unsigned long long tie_mask = __ballot(cd == 2);
        if (lane == 0) wave_tie[wave] = __popcll(tie_mask);
        __syncthreads();
        int tie_rank = carry_tie + __popcll(tie_mask & below_me), tie_total = 0;
        for (int q = 0; q < kThreads / 64; q++) {
            if (q < wave) tie_rank += wave_tie[q];
            tie_total += wave_tie[q];
        }
        const bool keep = cd == 1 || (cd == 2 && tie_rank < ties);
        const unsigned long long keep_mask = __ballot(keep);
        if (lane == 0) wave_keep[wave] = __popcll(keep_mask);
        __syncthreads();
        int at = carry_keep + __popcll(keep_mask & below_me), keep_total = 0;
        for (int q = 0; q < kThreads / 64; q++) {
            if (q < wave) at += wave_keep[q];
            keep_total += wave_keep[q];
        }
        if (keep && at < cap) dst[at] = row0 + j;
        carry_keep += keep_total, carry_tie += tie_total;
        __syncthreads();
    }
}

__global__ __launch_bounds__(kThreads) void augment_select_paste_kernel(PasteArgs a) {
    __shared__ int hist[256];
    __shared__ unsigned sel_prefix;
    __shared__ int sel_rank;
    const liso_augment_batch_cfg& c = a.c;
    const int slot = blockIdx.x, b = blockIdx.y, K = c.max_num_objs, E = c.extra_capacity;
    const int64_t seed = a.frozen[0], calls = a.frozen[1];
    if (slot == 0 && b == 0 && threadIdx.x == 0) a.state[1] = calls + 1;  // the next call, or the next replay, draws afresh
    float4* out_points = a.extra_points + (size_t)b * E;
    float* out_flow = a.extra_flow ? a.extra_flow + (size_t)b * E * 3 : nullptr;
    int count = a.extra_counts[b];
    count = count < 0 ? 0 : (count > E ? E : count);
    const float nanf_ = __int_as_float(0x7fc00000);
    for (long r = (long)count + (long)slot * kThreads + threadIdx.x; r < E; r += (long)K * kThreads) {
        out_points[r] = make_float4(nanf_, nanf_, nanf_, nanf_);
        if (out_flow) out_flow[3 * r + 0] = nanf_, out_flow[3 * r + 1] = nanf_, out_flow[3 * r + 2] = nanf_;
    }
    const size_t o = (size_t)b * K + slot;
    const int snippet = a.sel[o * 4 + 0], p1 = a.sel[o * 4 + 1], p2 = a.sel[o * 4 + 2], flags = a.sel[o * 4 + 3];
    if (!(flags & 1)) return;  // (uniform over the block)
    const int begin = a.object_offsets[(size_t)b * (K + 1) + slot], end = a.object_offsets[(size_t)b * (K + 1) + slot + 1];
    if (begin < 0 || end < begin || end > E) return;
    const int kept = end - begin;
    const int64_t row0 = a.db_offsets[snippet];
    const int64_t n64 = a.db_offsets[snippet + 1] - row0;
    const int n = n64 > 0x7fffffff ? 0x7fffffff : (int)n64;  // (launch 5 gave a broken table kept = 0)
    const D::Stream s = D::make_stream(seed, calls, a.sample_ids[b]);
    int64_t* rows = a.kept_rows + (size_t)b * E + begin;
    if (kept > 0) {
        if (c.selection == LISO_AUGMENT_SELECT_DROPOUT && kept < n) {
            // radix select: the kept-th smallest (key, j) pair has key sel_prefix, and sel_rank of the rows with that key are kept
            if (threadIdx.x == 0) sel_prefix = 0u, sel_rank = kept;
            unsigned known = 0u;
            for (int shift = 24; shift >= 0; shift -= 8) {
                hist[threadIdx.x] = 0;
                __syncthreads();
                const unsigned want = sel_prefix;
                for (int j = threadIdx.x; j < n; j += kThreads) {
                    const unsigned key = D::key32(s, D::kKey, slot, (uint32_t)j);
                    if ((key & known) == want) atomicAdd(&hist[(key >> shift) & 255u], 1);
                }
                __syncthreads();
                if (threadIdx.x == 0) {
                    int rank = sel_rank, bin = 0;
                    while (bin < 255 && rank > hist[bin]) rank -= hist[bin++];
                    sel_rank = rank;
                    sel_prefix = want | ((unsigned)bin << shift);
                }
                known |= 255u << shift;
                __syncthreads();
            }
            const unsigned threshold = sel_prefix;
            const int ties = sel_rank;
            compact_rows(n, [&](int j) {
                const unsigned key = D::key32(s, D::kKey, slot, (uint32_t)j);
                return key < threshold ? 1 : (key == threshold ? 2 : 0);
            }, ties, row0, rows, kept);
        } else if (c.selection == LISO_AUGMENT_SELECT_RAYDROP && !(flags & 2)) {
            const int32_t* lidar = a.db_rows_lidar + row0;
            compact_rows(n, [&](int j) { return (lidar[j] - p2) % p1 == 0 ? 1 : 0; }, 0, row0, rows, kept);
        } else {
            for (int j = threadIdx.x; j < kept; j += kThreads) rows[j] = row0 + j;
        }
    }
    __syncthreads();  // (the rows above were written by other threads of this block)
    paste_object(a.db_points, c.db_rows, a.kept_rows + (size_t)b * E, begin, end, a.pose + o * 12, FlowRandPhilox{s, (uint32_t)slot, row0},
                 c.vmin, c.vmax, out_points, out_flow, a.box_velo + o);
}

// ---- appending the pasted rows behind a cloud ------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void cloud_append_kernel(const float* __restrict__ src, const int32_t* __restrict__ counts, int n_max,
                                                                const float* __restrict__ extra, const int32_t* __restrict__ extra_counts, int E,
                                                                int cols, float* __restrict__ out, int32_t* __restrict__ out_counts) {
    const int b = blockIdx.y;
    const long r = (long)blockIdx.x * kThreads + threadIdx.x;
    int n = counts[b], e = extra_counts[b];
    n = n < 0 ? 0 : (n > n_max ? n_max : n);
    e = e < 0 ? 0 : (e > E ? E : e);
    if (r == 0) out_counts[b] = n + e;
    if (r >= (long)n_max + E) return;
    float* dst = out + ((size_t)b * ((size_t)n_max + E) + r) * cols;
    if (r < n) {
        const float* p = src + ((size_t)b * n_max + r) * cols;
        for (int q = 0; q < cols; q++) dst[q] = p[q];
    } else if (r < (long)n + e) {
        const float* p = extra + ((size_t)b * E + (r - n)) * cols;
        for (int q = 0; q < cols; q++) dst[q] = p[q];
    } else {
        for (int q = 0; q < cols; q++) dst[q] = __int_as_float(0x7fc00000);
    }
}

struct Layout {
    size_t occ, free_mask, prefix, frozen, pose, sel, rows, total;
};

Layout layout_of(const liso_augment_batch_cfg& c) {
    Layout l;
    const size_t B = (size_t)c.batch, K = (size_t)c.max_num_objs;
    size_t at = 0;
    l.occ = at, at += up16(B * c.h * words_per_row(c.w) * 64);
    l.free_mask = at, at += up16(B * c.h * c.w);
    l.prefix = at, at += up16(B * ((size_t)c.h + 1) * sizeof(int32_t));
    l.frozen = at, at += 16;
    l.pose = at, at += up16(B * K * 12 * sizeof(double));
    l.sel = at, at += up16(B * K * 4 * sizeof(int32_t));
    l.rows = at, at += up16(B * (size_t)c.extra_capacity * sizeof(int64_t));
    l.total = at;
    return l;
}

bool cfg_ok(const liso_augment_batch_cfg* c) {
    if (!c || !mask_geometry_ok(c->batch, c->n_max, c->h, c->w, c->radius)) return false;
    if (c->max_num_objs < 1 || c->max_num_objs > kMaxObjs || c->num_snippets < 1 || c->db_rows < 0 || c->extra_capacity < 0) return false;
    if (c->selection != LISO_AUGMENT_SELECT_ALL && c->selection != LISO_AUGMENT_SELECT_DROPOUT && c->selection != LISO_AUGMENT_SELECT_RAYDROP)
        return false;
    // (negated comparisons: a NaN fails them)
    if (!(c->range_x > 0.0) || !(c->range_y > 0.0) || !(c->cell_x > 0.0) || !(c->cell_y > 0.0)) return false;
    if (!(c->max_points_dropout >= 0.0 && c->max_points_dropout <= 1.0) || !(c->max_scale_delta >= 0.0) || !(c->vmin <= c->vmax)) return false;
    return true;
}

}  // namespace

extern "C" {

size_t liso_bev_free_mask_batch_workspace_bytes(int batch, int h, int w) {
    if (batch < 1 || h <= 0 || w <= 0) return 0;
    return (size_t)batch * h * words_per_row(w) * 64;
}

int liso_bev_free_mask_batch(const int32_t* pillar_coors, const int32_t* counts, int batch, int n_max, int h, int w, int radius,
                             uint8_t* free_mask, int32_t* row_free_prefix, void* workspace, size_t workspace_bytes, void* stream) {
    if (!mask_geometry_ok(batch, n_max, h, w, radius) || !counts || !free_mask || !row_free_prefix || !workspace) return LISO_EINVAL;
    if (n_max > 0 && !pillar_coors) return LISO_EINVAL;
    if (((uintptr_t)pillar_coors & 7) || ((uintptr_t)workspace & 7)) return LISO_EINVAL;
    if (workspace_bytes < liso_bev_free_mask_batch_workspace_bytes(batch, h, w)) return LISO_EWORKSPACE;
    return launch_free_mask_batch(pillar_coors, counts, batch, n_max, h, w, radius, free_mask, row_free_prefix, (uint8_t*)workspace,
                                  (hipStream_t)stream);
}

size_t liso_snippet_augment_batch_workspace_bytes(const liso_augment_batch_cfg* cfg) {
    if (!cfg_ok(cfg)) return 0;
    return layout_of(*cfg).total;
}

int liso_snippet_augment_batch(const liso_augment_batch_cfg* cfg, const int32_t* pillar_coors, const int32_t* counts, const float* db_points,
                               const int64_t* db_offsets, const float* db_dims, const float* db_pos_z, const int32_t* db_lidar_rows,
                               int64_t* state, const int64_t* sample_ids, float* extra_points, float* extra_flow, int32_t* extra_counts,
                               int32_t* object_offsets, float* box_pos, float* box_dims, float* box_rot, float* box_velo, uint8_t* box_valid,
                               double* draws, int32_t* overflow, int64_t* kept_rows, void* workspace, size_t workspace_bytes, void* stream) {
    if (!cfg_ok(cfg)) return LISO_EINVAL;
    const liso_augment_batch_cfg& c = *cfg;
    if (!counts || !db_points || !db_offsets || !db_dims || !db_pos_z || !state || !sample_ids || !extra_points || !extra_counts ||
        !object_offsets || !box_pos || !box_dims || !box_rot || !box_velo || !box_valid || !draws || !overflow || !workspace)
        return LISO_EINVAL;
    if (c.n_max > 0 && !pillar_coors) return LISO_EINVAL;
    if (c.selection == LISO_AUGMENT_SELECT_RAYDROP && !db_lidar_rows) return LISO_EINVAL;
    if (((uintptr_t)db_points | (uintptr_t)extra_points | (uintptr_t)workspace) & 15) return LISO_EINVAL;
    if (((uintptr_t)pillar_coors | (uintptr_t)db_offsets | (uintptr_t)state | (uintptr_t)sample_ids | (uintptr_t)draws | (uintptr_t)kept_rows) & 7)
        return LISO_EINVAL;
    const Layout l = layout_of(c);
    if (workspace_bytes < l.total) return LISO_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    uint8_t* ws = (uint8_t*)workspace;
    uint8_t* free_mask = ws + l.free_mask;
    int32_t* prefix = (int32_t*)(ws + l.prefix);
    const int rc = launch_free_mask_batch(pillar_coors, counts, c.batch, c.n_max, c.h, c.w, c.radius, free_mask, prefix, ws + l.occ, st);
    if (rc != LISO_OK) return rc;
    Tables t;
    t.c = c;
    t.free_mask = free_mask, t.prefix = prefix, t.db_offsets = db_offsets, t.db_dims = db_dims, t.db_z = db_pos_z;
    t.db_rows_lidar = db_lidar_rows, t.state = state, t.sample_ids = sample_ids, t.frozen = (int64_t*)(ws + l.frozen);
    t.pose = (double*)(ws + l.pose), t.sel = (int32_t*)(ws + l.sel), t.extra_counts = extra_counts, t.object_offsets = object_offsets;
    t.box_pos = box_pos, t.box_dims = box_dims, t.box_rot = box_rot, t.box_velo = box_velo, t.box_valid = box_valid;
    t.draws = draws, t.overflow = overflow;
    augment_draw_kernel<<<c.batch, 64, 0, st>>>(t);
    PasteArgs p;
    p.c = c;
    p.db_points = (const float4*)db_points, p.db_offsets = db_offsets, p.db_rows_lidar = db_lidar_rows, p.state = state;
    p.frozen = t.frozen, p.sample_ids = sample_ids, p.pose = t.pose, p.sel = t.sel, p.extra_counts = extra_counts;
    p.object_offsets = object_offsets, p.kept_rows = kept_rows ? kept_rows : (int64_t*)(ws + l.rows);
    p.extra_points = (float4*)extra_points, p.extra_flow = extra_flow, p.box_velo = box_velo;
    augment_select_paste_kernel<<<dim3(c.max_num_objs, c.batch), kThreads, 0, st>>>(p);
    return hipGetLastError() == hipSuccess ? LISO_OK : LISO_ELAUNCH;
}

int liso_cloud_append_batch(const float* cloud, const int32_t* counts, const float* extra, const int32_t* extra_counts, int batch, int n_max,
                            int extra_capacity, int cols, float* out, int32_t* out_counts, void* stream) {
    if (batch < 1 || batch > 65535 || n_max < 0 || extra_capacity < 0 || cols < 1 || cols > 64) return LISO_EINVAL;
    if (!counts || !extra_counts || !out_counts) return LISO_EINVAL;
    if ((n_max > 0 && !cloud) || (extra_capacity > 0 && !extra) || ((long)n_max + extra_capacity > 0 && !out)) return LISO_EINVAL;
    const long rows = (long)n_max + extra_capacity;
    const unsigned gx = (unsigned)((rows + kThreads - 1) / kThreads);
    cloud_append_kernel<<<dim3(gx < 1 ? 1 : gx, batch), kThreads, 0, (hipStream_t)stream>>>(cloud, counts, n_max, extra, extra_counts,
                                                                                           extra_capacity, cols, out, out_counts);
    return hipGetLastError() == hipSuccess ? LISO_OK : LISO_ELAUNCH;
}

}  // extern "C"
