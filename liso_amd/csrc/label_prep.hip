// The label side of a training sample on gfx950: contained-point flags, the box filter with its compaction, object velocities, the
// ignore-region mask and the full target rendering.  C ABI and semantics: include/liso_label_prep.h.  Compiled without FMA
// contraction: every expression is the header's expression, operation by operation.
//
// Contained points: one block per (sample, tile of 256 points); the boxes of the sample pass through LDS in chunks, every wave
// ballots "inside" per box and its first lane ORs one bit into the box's flag word (a vector atomic on a uint32).
// Filter: one block per sample; per chunk of 256 slots a ballot per wave, a prefix over the four waves and a running base give
// every kept slot its place.  Rendering: one thread per cell, boxes in LDS, one pass that keeps the running maximum and restarts
// the attribute sums whenever a hotter box appears.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "../../include/liso_label_prep.h"
#include "dev_common.h"
#include "zero_fill.h"

namespace {

using liso_dev::affine_inv;
using liso_dev::check_launch;
using liso_dev::cloud_rows;
using liso_dev::distinct;
using liso_dev::mat4_mul;
using liso_dev::to_i32;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kChunk = 256;  // boxes resident in LDS at a time

__device__ __forceinline__ double cell_center(int i, int n, double range) { return (((double)i + 0.5) / (double)n) * range - 0.5 * range; }

// ---- 1. contained points --------------------------------------------------------------------------------------------------------
struct BoxFrame {
    float r0[3], r1[3], tz;  // fp32 inverse pose: rows 0 and 1 as (a, b, t), row 2 as its translation
    double hx, hy, hz;       // half extents
};

__global__ __launch_bounds__(kThreads) void has_points_kernel(int K, int N, int stride, const double* __restrict__ box_pos,
                                                              const double* __restrict__ box_dims, const double* __restrict__ box_rot,
                                                              const float* __restrict__ pcl, const int32_t* __restrict__ counts,
                                                              uint32_t* __restrict__ flags) {
    __shared__ BoxFrame frames[kChunk];
    const int b = blockIdx.y, i = blockIdx.x * kThreads + threadIdx.x;
    const int rows = cloud_rows(counts, b, N);
    if ((int)(blockIdx.x * kThreads) >= rows) return;  // the whole tile lies behind the count (uniform per block)
    const bool live = i < rows;
    float px = NAN, py = NAN, pz = NAN;
    if (live) {
        const float* p = pcl + ((size_t)b * N + i) * stride;
        px = p[0], py = p[1], pz = p[2];
    }
    for (int k0 = 0; k0 < K; k0 += kChunk) {
        const int n = min(kChunk, K - k0);
        __syncthreads();
        for (int j = threadIdx.x; j < n; j += kThreads) {
            const size_t at = (size_t)b * K + k0 + j;
            const double x = box_pos[at * 3], y = box_pos[at * 3 + 1], z = box_pos[at * 3 + 2];
            const double c = cos(box_rot[at]), s = sin(box_rot[at]);
            BoxFrame f;
            f.r0[0] = (float)c, f.r0[1] = (float)s, f.r0[2] = (float)(-(c * x + s * y));
            f.r1[0] = (float)(-s), f.r1[1] = (float)c, f.r1[2] = (float)(-(c * y - s * x));
            f.tz = (float)(-z);
            f.hx = 0.5 * box_dims[at * 3], f.hy = 0.5 * box_dims[at * 3 + 1], f.hz = 0.5 * box_dims[at * 3 + 2];
            frames[j] = f;
        }
        __syncthreads();
        for (int j = 0; j < n; ++j) {
            const BoxFrame& f = frames[j];
            const float u = (f.r0[0] * px + f.r0[1] * py) + f.r0[2];
            const float v = (f.r1[0] * px + f.r1[1] * py) + f.r1[2];
            const float w = pz + f.tz;
            const bool inside = live && fabs((double)u) < f.hx && fabs((double)v) < f.hy && fabs((double)w) < f.hz;
            const unsigned long long hit = __ballot(inside);
            if (hit != 0ull && (threadIdx.x & 63) == 0) atomicOr(&flags[(size_t)b * K + k0 + j], 1u);
        }
    }
}

// ---- 2. filter and compaction -----------------------------------------------------------------------------------------------------
struct AttrJobs {
    liso_box_attr_job job[LISO_LABEL_MAX_ATTRS];
    int n;
};

__global__ __launch_bounds__(kThreads) void filter_boxes_kernel(liso_box_filter_cfg c, const double* __restrict__ box_pos,
                                                                const uint8_t* __restrict__ valid, const uint32_t* __restrict__ flags,
                                                                const uint8_t* __restrict__ has_in, AttrJobs jobs,
                                                                uint8_t* __restrict__ out_valid, uint8_t* __restrict__ has_out) {
    __shared__ int wave_count[kWaves];
    const int b = blockIdx.x, K = c.n_boxes, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t base = (size_t)b * K;
    int placed = 0;  // kept boxes of the chunks before this one (the same in every thread)
    for (int k0 = 0; k0 < K; k0 += kThreads) {
        const int k = k0 + threadIdx.x;
        bool keep = false;
        if (k < K) {
            const bool has = flags ? flags[base + k] != 0u : has_in[base + k] != 0;
            if (has_out) has_out[base + k] = has ? 1 : 0;
            const double x = box_pos[(base + k) * 3], y = box_pos[(base + k) * 3 + 1], z = box_pos[(base + k) * 3 + 2];
            const bool in_bev = !c.filter_bev || (0.5 * c.range_x >= fabs(x) && 0.5 * c.range_y >= fabs(y));
            const bool in_range = !c.filter_range || sqrt((x * x + y * y) + z * z) < c.filter_range_m;
            keep = valid[base + k] != 0 && has && in_bev && in_range;
        }
        const unsigned long long kept = __ballot(keep);
        __syncthreads();  // the previous chunk's wave_count has been read
        if (lane == 0) wave_count[wave] = __popcll(kept);
        __syncthreads();
        int before = placed, total = placed;
        for (int w = 0; w < kWaves; ++w) {
            if (w < wave) before += wave_count[w];
            total += wave_count[w];
        }
        if (keep) {
            const size_t to = base + before + __popcll(kept & ((1ull << lane) - 1ull));
            for (int a = 0; a < jobs.n; ++a) {
                const int words = jobs.job[a].row_bytes / 4;
                const uint32_t* src = (const uint32_t*)jobs.job[a].src + (base + k) * words;
                uint32_t* dst = (uint32_t*)jobs.job[a].dst + to * words;
                for (int q = 0; q < words; ++q) dst[q] = src[q];
            }
            out_valid[to] = 1;
        }
        placed = total;
    }
    for (int k = placed + threadIdx.x; k < K; k += kThreads) {
        for (int a = 0; a < jobs.n; ++a) {
            const int words = jobs.job[a].row_bytes / 4;
            uint32_t* dst = (uint32_t*)jobs.job[a].dst + (base + k) * words;
            for (int q = 0; q < words; ++q) dst[q] = 0u;
        }
        out_valid[base + k] = 0;
    }
}

// ---- 3. object velocity -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void velocity_kernel(int K, const double* __restrict__ odom, const double* __restrict__ pose_ta,
                                                      const double* __restrict__ pose_tb, double* __restrict__ out) {
    const int b = blockIdx.y, k = blockIdx.x * 64 + threadIdx.x;
    if (k >= K) return;
    const size_t at = (size_t)b * K + k;
    double A[16], Bm[16], Ai[16], D[16], O[16], Oi[16];
    for (int q = 0; q < 16; ++q) A[q] = pose_ta[at * 16 + q], Bm[q] = pose_tb[at * 16 + q], O[q] = odom[(size_t)b * 16 + q];
    affine_inv(A, Ai);
    affine_inv(O, Oi);
    mat4_mul(Bm, Ai, D);
    const double p[4] = {A[3], A[7], 0.0, 1.0};
    double f[3];
    for (int r = 0; r < 3; ++r) {
        double m[4];
        for (int q = 0; q < 4; ++q) {
            const double eye = r == q ? 1.0 : 0.0;
            m[q] = (D[4 * r + q] - eye) - (Oi[4 * r + q] - eye);
        }
        f[r] = ((m[0] * p[0] + m[1] * p[1]) + m[2] * p[2]) + m[3] * p[3];
    }
    for (int r = 0; r < 3; ++r) out[at * 3 + r] = ((A[4 * r] * f[0] + A[4 * r + 1] * f[1]) + A[4 * r + 2] * f[2]) + A[4 * r + 3] * 0.0;
}

// ---- 4. ignore-region mask --------------------------------------------------------------------------------------------------------
struct FlatBox {
    double c, s, tu, tv, hx, hy;
};

__global__ __launch_bounds__(kThreads) void ignore_mask_kernel(int K, int H, int W, double rx, double ry, const double* __restrict__ box_pos,
                                                               const double* __restrict__ box_dims, const double* __restrict__ box_rot,
                                                               const uint8_t* __restrict__ valid, uint8_t* __restrict__ mask) {
    __shared__ FlatBox boxes[kChunk];
    __shared__ int n_live;
    const int b = blockIdx.y, cell = blockIdx.x * kThreads + threadIdx.x;
    const bool live = cell < H * W;
    const int i = live ? cell / W : 0, j = live ? cell - i * W : 0;
    const double px = cell_center(i, H, rx), py = cell_center(j, W, ry);
    bool hit = false;
    for (int k0 = 0; k0 < K; k0 += kChunk) {
        const int n = min(kChunk, K - k0);
        __syncthreads();
        if (threadIdx.x == 0) n_live = 0;
        __syncthreads();
        for (int q = threadIdx.x; q < n; q += kThreads) {
            const size_t at = (size_t)b * K + k0 + q;
            if (!valid[at]) continue;
            const double x = box_pos[at * 3], y = box_pos[at * 3 + 1];
            const double c = cos(box_rot[at]), s = sin(box_rot[at]);
            boxes[atomicAdd(&n_live, 1)] = {c, s, c * x + s * y, c * y - s * x, 0.5 * box_dims[at * 3], 0.5 * box_dims[at * 3 + 1]};
        }
        __syncthreads();
        for (int q = 0; q < n_live; ++q) {
            const FlatBox& f = boxes[q];
            const double u = (f.c * px + f.s * py) - f.tu, v = (f.c * py - f.s * px) - f.tv;
            hit |= -f.hx < u && u < f.hx && -f.hy < v && v < f.hy;
        }
    }
    if (live) mask[(size_t)b * H * W + cell] = hit ? 1 : 0;
}

// ---- 5. target rendering ----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double gauss(double cx, double cy, double bx, double by, double c, double s, double vl, double vw) {
    const double dx = cx - bx, dy = cy - by;
    const double u = dx * c + dy * s, v = dy * c - dx * s;
    return exp(-((u * u) / vl + (v * v) / vw) / 2.0);
}

// one block per (sample, box): the divisor of the box's gaussian
__global__ __launch_bounds__(kThreads) void targets_ex_norm_kernel(liso_targets_ex_cfg t, const double* __restrict__ box_pos,
                                                                   const double* __restrict__ box_dims, const double* __restrict__ box_rot,
                                                                   const uint8_t* __restrict__ box_valid, double* __restrict__ box_max) {
    __shared__ double red[kWaves];
    const size_t at = blockIdx.x;
    if (!box_valid[at]) {  // uniform per block
        if (threadIdx.x == 0) box_max[at] = 1.0;
        return;
    }
    const double vl = 0.15 * box_dims[at * 3], vw = 0.15 * box_dims[at * 3 + 1];
    if (t.normalize_gaussian) {
        const double two_pi = 2.0 * 3.141592653589793;
        if (threadIdx.x == 0) box_max[at] = sqrt((two_pi * two_pi) * (vl * vw));
        return;
    }
    const double bx = box_pos[at * 3], by = box_pos[at * 3 + 1], c = cos(box_rot[at]), s = sin(box_rot[at]);
    double m = 0.0;
    for (int cell = threadIdx.x; cell < t.h * t.w; cell += kThreads) {
        const int i = cell / t.w, j = cell - i * t.w;
        m = fmax(m, gauss(cell_center(i, t.h, t.range_x), cell_center(j, t.w, t.range_y), bx, by, c, s, vl, vw));
    }
    for (int o = 32; o >= 1; o >>= 1) m = fmax(m, __shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kWaves; ++w) m = fmax(m, red[w]);
        box_max[at] = fmax(fmax(m, red[0]), 1e-5);
    }
}

struct HeatBox {
    double x, y, c, s, vl, vw, div, scale;
    int ci, cj;  // the cell of the centre
    int slot;    // k
    int pad;
};

// the attributes a box gives to the cells it wins, in fp64: dims 3, pos 3, rot 2 (or 1), velo 1
__device__ __forceinline__ void add_attributes(const liso_targets_ex_cfg& t, size_t at, const double* box_pos, const double* box_dims,
                                               const double* box_rot, const double* box_velo, double* acc) {
    for (int a = 0; a < 3; ++a) {
        const double d = box_dims[at * 3 + a];
        acc[a] += t.log_dims ? log(d) : d;
        acc[3 + a] += box_pos[at * 3 + a];
    }
    const double r = box_rot[at];
    if (t.rot_channels == 2) acc[6] += sin(r), acc[7] += cos(r);
    else acc[6] += r;
    acc[8] += box_velo[at];
}

__global__ __launch_bounds__(kThreads) void targets_ex_render_kernel(liso_targets_ex_cfg t, const double* __restrict__ box_pos,
                                                                     const double* __restrict__ box_dims, const double* __restrict__ box_rot,
                                                                     const double* __restrict__ box_velo, const double* __restrict__ prob_scale,
                                                                     const uint8_t* __restrict__ box_valid, const double* __restrict__ box_max,
                                                                     float* __restrict__ probs, float* __restrict__ dims, float* __restrict__ pos,
                                                                     float* __restrict__ rot, float* __restrict__ velo,
                                                                     uint8_t* __restrict__ center_mask) {
    constexpr int kBoxes = 128;
    __shared__ HeatBox boxes[kBoxes];
    __shared__ int n_live;
    const int b = blockIdx.y, cell = blockIdx.x * kThreads + threadIdx.x, K = t.n_boxes;
    const bool live = cell < t.h * t.w;
    const int i = live ? cell / t.w : 0, j = live ? cell - i * t.w : 0;
    const double cx = cell_center(i, t.h, t.range_x), cy = cell_center(j, t.w, t.range_y);
    double best = -INFINITY;
    double acc[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    bool any_box = false, center = false;
    for (int k0 = 0; k0 < K; k0 += kBoxes) {
        const int n = min(kBoxes, K - k0);
        __syncthreads();  // the previous chunk has been read
        // one wave lays the valid boxes of the chunk into LDS in box order (a prefix over its ballots), so that the sums of tying
        // boxes are added in the same order in every run
        if (threadIdx.x < 64) {
            int filled = 0;
            for (int q0 = 0; q0 < n; q0 += 64) {
                const int q = q0 + (int)threadIdx.x;
                const size_t at = (size_t)b * K + k0 + (q < n ? q : 0);
                const bool ok = q < n && box_valid[at] != 0;
                const unsigned long long m = __ballot(ok);
                if (ok) {
                    HeatBox h;
                    h.x = box_pos[at * 3], h.y = box_pos[at * 3 + 1];
                    const double r = box_rot[at];
                    h.c = cos(r), h.s = sin(r);
                    h.vl = 0.15 * box_dims[at * 3], h.vw = 0.15 * box_dims[at * 3 + 1];
                    h.div = box_max[at];
                    h.scale = prob_scale ? prob_scale[at] : 1.0;
                    h.ci = min(max(to_i32(((h.x + 0.5 * t.range_x) / t.range_x) * (double)t.h), 0), t.h - 1);
                    h.cj = min(max(to_i32(((h.y + 0.5 * t.range_y) / t.range_y) * (double)t.w), 0), t.w - 1);
                    h.slot = k0 + q, h.pad = 0;
                    boxes[filled + __popcll(m & ((1ull << threadIdx.x) - 1ull))] = h;
                }
                filled += __popcll(m);
            }
            if (threadIdx.x == 0) n_live = filled;
        }
        __syncthreads();
        const int nl = n_live;
        for (int q = 0; q < nl; ++q) {
            const HeatBox& h = boxes[q];
            const double heat = gauss(cx, cy, h.x, h.y, h.c, h.s, h.vl, h.vw) / h.div;
            const bool occupied = heat > 0.01;
            const double scaled = prob_scale ? h.scale * heat : heat;
            any_box = true;
            center |= h.ci == i && h.cj == j;
            if (scaled > best) {
                best = scaled;
                for (int a = 0; a < 9; ++a) acc[a] = 0.0;
            }
            if (scaled == best && occupied) add_attributes(t, (size_t)b * K + h.slot, box_pos, box_dims, box_rot, box_velo, acc);
        }
    }
    if (!live) return;
    const size_t at = (size_t)b * t.h * t.w + cell;
    probs[at] = any_box ? (float)best : 0.f;
    for (int a = 0; a < 3; ++a) dims[at * 3 + a] = (float)acc[a], pos[at * 3 + a] = (float)acc[3 + a];
    for (int a = 0; a < t.rot_channels; ++a) rot[at * t.rot_channels + a] = (float)acc[6 + a];
    velo[at] = (float)acc[8];
    center_mask[at] = center ? 1 : 0;
}

}  // namespace

extern "C" {

int liso_box_has_points_f32(int batch, int n_boxes, int n_max, int point_stride, const double* box_pos, const double* box_dims,
                            const double* box_rot, const float* pcl, const int32_t* counts, uint32_t* flags, void* stream) {
    if (batch < 1 || batch > 65535 || n_boxes < 0 || n_boxes > LISO_LABEL_MAX_BOXES || n_max < 0 || n_max > LISO_LABEL_MAX_N || point_stride < 3)
        return LISO_EINVAL;
    if (n_boxes == 0) return LISO_OK;
    if (!box_pos || !box_dims || !box_rot || !flags || (n_max > 0 && !pcl)) return LISO_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (liso_zero::zero_async(flags, (size_t)batch * n_boxes * sizeof(uint32_t), st) != hipSuccess) return LISO_ELAUNCH;
    if (n_max > 0)
        has_points_kernel<<<dim3((unsigned)((n_max + kThreads - 1) / kThreads), batch), kThreads, 0, st>>>(n_boxes, n_max, point_stride, box_pos,
                                                                                                        box_dims, box_rot, pcl, counts, flags);
    return check_launch();
}

int liso_filter_boxes(const liso_box_filter_cfg* cfg, const double* box_pos, const uint8_t* valid, const uint32_t* flags,
                      const uint8_t* has_points_in, const liso_box_attr_job* attrs, int n_attrs, uint8_t* out_valid,
                      uint8_t* has_points_out, void* stream) {
    if (!cfg || cfg->batch < 1 || cfg->batch > 65535 || cfg->n_boxes < 0 || cfg->n_boxes > LISO_LABEL_MAX_BOXES) return LISO_EINVAL;
    if (n_attrs < 0 || n_attrs > LISO_LABEL_MAX_ATTRS || (n_attrs > 0 && !attrs)) return LISO_EINVAL;
    if (cfg->filter_bev && (!(cfg->range_x > 0.0) || !(cfg->range_y > 0.0))) return LISO_EINVAL;
    if (cfg->filter_range && isnan(cfg->filter_range_m)) return LISO_EINVAL;
    if (cfg->n_boxes == 0) return LISO_OK;
    if (!box_pos || !valid || !out_valid || (flags == nullptr) == (has_points_in == nullptr)) return LISO_EINVAL;
    const size_t slots = (size_t)cfg->batch * cfg->n_boxes;
    if (!distinct(valid, out_valid, slots) || (has_points_out && has_points_in && !distinct(has_points_in, has_points_out, slots)))
        return LISO_EINVAL;
    AttrJobs jobs = {};
    for (int a = 0; a < n_attrs; ++a) {
        const liso_box_attr_job& q = attrs[a];
        if (!q.src || !q.dst || q.row_bytes < 4 || q.row_bytes > 1024 || q.row_bytes % 4 != 0) return LISO_EINVAL;
        if ((((uintptr_t)q.src) | ((uintptr_t)q.dst)) & 3) return LISO_EINVAL;
        if (!distinct(q.src, q.dst, slots * q.row_bytes)) return LISO_EINVAL;
        jobs.job[a] = q;
    }
    jobs.n = n_attrs;
    filter_boxes_kernel<<<cfg->batch, kThreads, 0, (hipStream_t)stream>>>(*cfg, box_pos, valid, flags, has_points_in, jobs, out_valid,
                                                                         has_points_out);
    return check_launch();
}

int liso_object_velocity_f64(int batch, int n_boxes, const double* odom_ta_tb, const double* pose_ta, const double* pose_tb,
                             double* out, void* stream) {
    if (batch < 1 || batch > 65535 || n_boxes < 0 || n_boxes > LISO_LABEL_MAX_BOXES) return LISO_EINVAL;
    if (n_boxes == 0) return LISO_OK;
    if (!odom_ta_tb || !pose_ta || !pose_tb || !out) return LISO_EINVAL;
    velocity_kernel<<<dim3((unsigned)((n_boxes + 63) / 64), batch), 64, 0, (hipStream_t)stream>>>(n_boxes, odom_ta_tb, pose_ta, pose_tb, out);
    return check_launch();
}

int liso_ignore_region_mask(int batch, int n_boxes, int h, int w, double range_x, double range_y, const double* box_pos,
                            const double* box_dims, const double* box_rot, const uint8_t* valid, uint8_t* mask, void* stream) {
    if (batch < 1 || batch > 65535 || n_boxes < 0 || n_boxes > LISO_LABEL_MAX_BOXES || h < 1 || w < 1 || (long)h * w > LISO_LABEL_MAX_CELLS)
        return LISO_EINVAL;
    if (!(range_x > 0.0) || !(range_y > 0.0) || !isfinite(range_x) || !isfinite(range_y) || !mask) return LISO_EINVAL;
    if (n_boxes > 0 && (!box_pos || !box_dims || !box_rot || !valid)) return LISO_EINVAL;
    ignore_mask_kernel<<<dim3((unsigned)((h * w + kThreads - 1) / kThreads), batch), kThreads, 0, (hipStream_t)stream>>>(
        n_boxes, h, w, range_x, range_y, box_pos, box_dims, box_rot, valid, mask);
    return check_launch();
}

int liso_render_center_targets_ex_f32(const liso_targets_ex_cfg* cfg, const double* box_pos, const double* box_dims,
                                      const double* box_rot, const double* box_velo, const double* prob_scale,
                                      const uint8_t* box_valid, double* box_max, float* probs, float* dims, float* pos, float* rot,
                                      float* velo, uint8_t* center_mask, void* stream) {
    if (!cfg || cfg->batch < 1 || cfg->batch > 65535 || cfg->n_boxes < 0 || cfg->n_boxes > LISO_LABEL_MAX_BOXES || cfg->h < 1 || cfg->w < 1 ||
        (long)cfg->h * cfg->w > LISO_LABEL_MAX_CELLS)
        return LISO_EINVAL;
    if (cfg->rot_channels != 1 && cfg->rot_channels != 2) return LISO_EINVAL;
    if ((long)cfg->batch * cfg->n_boxes > INT_MAX) return LISO_EINVAL;  // one block per (sample, box)
    if (!(cfg->range_x > 0.0) || !(cfg->range_y > 0.0) || !isfinite(cfg->range_x) || !isfinite(cfg->range_y)) return LISO_EINVAL;
    if (cfg->normalize_gaussian && prob_scale) return LISO_EINVAL;
    if (!probs || !dims || !pos || !rot || !velo || !center_mask) return LISO_EINVAL;
    if (cfg->n_boxes > 0 && (!box_pos || !box_dims || !box_rot || !box_velo || !box_valid || !box_max)) return LISO_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (cfg->n_boxes > 0)
        targets_ex_norm_kernel<<<(unsigned)(cfg->batch * cfg->n_boxes), kThreads, 0, st>>>(*cfg, box_pos, box_dims, box_rot, box_valid, box_max);
    targets_ex_render_kernel<<<dim3((unsigned)((cfg->h * cfg->w + kThreads - 1) / kThreads), cfg->batch), kThreads, 0, st>>>(
        *cfg, box_pos, box_dims, box_rot, box_velo, prob_scale, box_valid, box_max, probs, dims, pos, rot, velo, center_mask);
    return check_launch();
}

}  // extern "C"
