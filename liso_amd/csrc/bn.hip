// Fused BatchNorm2d(+ReLU) for channels-last feature maps on gfx950.  C ABI + reference lines: include/liso_bn.h.
//
// HBM-bound elementwise/reduction passes.  Every thread moves 16 B per access (4 fp32 / 8 bf16 channels of one
// pixel); a 256-thread block covers 256/(C/V) pixel rows per step, so a wave-instruction reads whole 128/256-B
// channel rows back to back (fully coalesced).  Statistics: every block accumulates sums shifted by its own first row
// (so they stay well conditioned), emits (mean_b, M2_b), and the grid-level merge is the two-pass form over the block
// means in fp64 and a fixed order: the variance never suffers the E[x^2]-E[x]^2 cancellation and results are bitwise
// reproducible.
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <math.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/liso_bn.h"
#include "../../include/liso_iou3d.h"
#include "chain_bodies.h"
#include "dev_common.h"
#include "elem16.h"

namespace {

using liso_dev::check_launch;

constexpr int kThreads = 256;
constexpr int kRowsPerBlock = 128;
constexpr int kMaxBlocks = 4096;

template <typename T> struct Vec;
template <> struct Vec<float> {
    static constexpr int V = 4;
    static __device__ __forceinline__ void load(const float* p, float (&v)[4]) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    }
    static __device__ __forceinline__ void store(float* p, const float (&v)[4]) {
        *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    }
};
template <> struct Vec<__hip_bfloat16> {
    static constexpr int V = 8;
    static __device__ __forceinline__ void load(const __hip_bfloat16* p, float (&v)[8]) {
        const uint4 t = *reinterpret_cast<const uint4*>(p);
        const unsigned w[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
        for (int i = 0; i < 4; i++) {
            v[2 * i] = __uint_as_float(w[i] << 16);
            v[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
        }
    }
    static __device__ __forceinline__ void store(__hip_bfloat16* p, const float (&v)[8]) {
        unsigned w[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const __hip_bfloat16 lo = __float2bfloat16(v[2 * i]), hi = __float2bfloat16(v[2 * i + 1]);
            w[i] = (unsigned)(*reinterpret_cast<const unsigned short*>(&lo)) |
                   ((unsigned)(*reinterpret_cast<const unsigned short*>(&hi)) << 16);
        }
        *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[2], w[3]);
    }
};

template <> struct Vec<_Float16> {  // fp16: the bf16 layout, 8 channels per lane; stores round to nearest even
    static constexpr int V = 8;
    static __device__ __forceinline__ void load(const _Float16* p, float (&v)[8]) {
        const uint4 t = *reinterpret_cast<const uint4*>(p);
        const unsigned w[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
        for (int i = 0; i < 4; i++) {
            v[2 * i] = liso_e16::F16::lo(w[i]);
            v[2 * i + 1] = liso_e16::F16::hi(w[i]);
        }
    }
    static __device__ __forceinline__ void store(_Float16* p, const float (&v)[8]) {
        unsigned w[4];
#pragma unroll
        for (int i = 0; i < 4; i++) w[i] = liso_e16::F16::pack(v[2 * i], v[2 * i + 1]);
        *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[2], w[3]);
    }
};

// element code of the entry points (include/liso_conv.h: LISO_ELEM_F32 / BF16 / F16)
static inline bool elem_ok(int e) { return e == LISO_ELEM_F32 || e == LISO_ELEM_BF16 || e == LISO_ELEM_F16; }

struct Geom {
    int cg;        // column groups = C / V
    int rl;        // row lanes per block = 256 / cg
    long rows_per_block;
    long xs, gs, ds;  // backward passes: elements between consecutive rows of x, dy and dx (C for dense [M, C] rows; wider when the
                      // rows are a channel slice of a wider channels-last tensor)
};

// ---- forward statistics ------------------------------------------------------------------------------------------------
// All threads of a block shift by the block's FIRST row (K[c] = x[r0][c]), so their shifted sums add directly; the
// block then emits (mean_b, M2_b) per channel.  partial layout per block: mean[C], m2[C] (floats); the row count of a
// block is implied by its index.
template <typename T>
__global__ __launch_bounds__(kThreads) void bn_stats_kernel(const T* __restrict__ x, long m, int c, Geom g,
                                                            float* __restrict__ partial) {
    constexpr int V = Vec<T>::V;
    __shared__ float s_1[kThreads][V + 1];
    __shared__ float s_2[kThreads][V + 1];
    x += (size_t)blockIdx.y * m * c;                        // blockIdx.y = group (InstanceNorm: sample), 0 for BatchNorm
    partial += (size_t)blockIdx.y * gridDim.x * 2 * c;
    const int tid = threadIdx.x;
    const int col = tid % g.cg, rlane = tid / g.cg;
    const long r0 = (long)blockIdx.x * g.rows_per_block;
    const long r1 = r0 + g.rows_per_block < m ? r0 + g.rows_per_block : m;
    float K[V], s1[V], s2[V];
    Vec<T>::load(x + r0 * c + col * V, K);
#pragma unroll
    for (int j = 0; j < V; j++) { s1[j] = 0.f; s2[j] = 0.f; }
#pragma unroll 8
    for (long r = rlane < g.rl ? r0 + rlane : r1; r < r1; r += g.rl) {  // (rlane >= rl: C / V does not divide the block, idle lanes)
        float v[V];
        Vec<T>::load(x + r * c + col * V, v);
#pragma unroll
        for (int j = 0; j < V; j++) { const float d = v[j] - K[j]; s1[j] += d; s2[j] = fmaf(d, d, s2[j]); }
    }
#pragma unroll
    for (int j = 0; j < V; j++) { s_1[tid][j] = s1[j]; s_2[tid][j] = s2[j]; }
    __syncthreads();
    // one thread per channel finishes the block: tid -> (col2, j2)
    if (tid < c) {
        const int col2 = tid / V, j2 = tid % V;
        float a = 0.f, b2 = 0.f;
        for (int q = 0; q < g.rl; q++) { a += s_1[q * g.cg + col2][j2]; b2 += s_2[q * g.cg + col2][j2]; }
        const float n = (float)(r1 - r0);
        // K of this channel: re-read the first row (L1/L2 hit)
        float Kv[V];
        Vec<T>::load(x + r0 * c + col2 * V, Kv);
        float kk = 0.f;
#pragma unroll
        for (int j = 0; j < V; j++) if (j == j2) kk = Kv[j];
        float* p = partial + (size_t)blockIdx.x * 2 * c;
        p[tid] = kk + a / n;
        p[c + tid] = fmaxf(b2 - a * a / n, 0.f);
    }
}

// merge block partials: mean = sum n_b mean_b / N ; M2 = sum (M2_b + n_b (mean_b - mean)^2)   (two passes over the tiny
// partial array, fp64, fixed order) -> scale | shift | mean | invstd, running stats
__global__ __launch_bounds__(1024) void bn_finalize_kernel(const float* __restrict__ partial, int nblk, long m, int c,
                                                           long rows_per_block, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, float* __restrict__ running_mean,
                                                           float* __restrict__ running_var, float momentum, float eps,
                                                           float* __restrict__ stats) {
    __shared__ double sh[1024];
    __shared__ double sh_mean[512];
    partial += (size_t)blockIdx.x * nblk * 2 * c;           // blockIdx.x = group
    stats += (size_t)blockIdx.x * 4 * c;
    const int tid = threadIdx.x;
    const int chunks = 1024 / c > 0 ? 1024 / c : 1;
    const int ch = tid % c, chunk = tid / c;
    const int per = (nblk + chunks - 1) / chunks;
    const int lo = chunk * per, hi = (chunk < chunks) ? (lo + per < nblk ? lo + per : nblk) : lo;
    const double last_n = (double)(m - (long)(nblk - 1) * rows_per_block);
    // the partial rows are read 8 at a time (independent loads in flight) and added in the original order
    double acc = 0.0;
    {
        int b = lo;
        for (; b + 8 <= hi; b += 8) {
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; j++) v[j] = partial[(size_t)(b + j) * 2 * c + ch];
#pragma unroll
            for (int j = 0; j < 8; j++) acc += (b + j == nblk - 1 ? last_n : (double)rows_per_block) * (double)v[j];
        }
        for (; b < hi; b++) acc += (b == nblk - 1 ? last_n : (double)rows_per_block) * (double)partial[(size_t)b * 2 * c + ch];
    }
    sh[tid] = acc;
    __syncthreads();
    if (tid < c) {
        double t = 0.0;
        for (int q = 0; q < chunks; q++) t += sh[q * c + tid];
        sh_mean[tid] = t / (double)m;
    }
    __syncthreads();
    const double mean = sh_mean[ch];
    acc = 0.0;
    {
        int b = lo;
        for (; b + 8 <= hi; b += 8) {
            float v[8], q2[8];
#pragma unroll
            for (int j = 0; j < 8; j++) { v[j] = partial[(size_t)(b + j) * 2 * c + ch]; q2[j] = partial[(size_t)(b + j) * 2 * c + c + ch]; }
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const double d = (double)v[j] - mean;
                acc += (double)q2[j] + (b + j == nblk - 1 ? last_n : (double)rows_per_block) * d * d;
            }
        }
        for (; b < hi; b++) {
            const double d = (double)partial[(size_t)b * 2 * c + ch] - mean;
            acc += (double)partial[(size_t)b * 2 * c + c + ch] + (b == nblk - 1 ? last_n : (double)rows_per_block) * d * d;
        }
    }
    __syncthreads();
    sh[tid] = acc;
    __syncthreads();
    if (tid < c) {
        double m2 = 0.0;
        for (int q = 0; q < chunks; q++) m2 += sh[q * c + tid];
        const double cnt = (double)m;
        const double var = m2 / cnt;
        const double invstd = 1.0 / sqrt(var + (double)eps);
        stats[tid] = (float)((double)gamma[tid] * invstd);
        stats[c + tid] = (float)((double)beta[tid] - mean * (double)gamma[tid] * invstd);
        stats[2 * c + tid] = (float)mean;
        stats[3 * c + tid] = (float)invstd;
        if (running_mean && cnt > 1.0) {
            running_mean[tid] = (1.f - momentum) * running_mean[tid] + momentum * (float)mean;
            running_var[tid] = (1.f - momentum) * running_var[tid] + momentum * (float)(m2 / (cnt - 1.0));
        }
    }
}

__global__ void bn_eval_stats_kernel(int c, const float* __restrict__ gamma, const float* __restrict__ beta,
                                     const float* __restrict__ running_mean, const float* __restrict__ running_var,
                                     float eps, float* __restrict__ stats) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= c) return;
    const float invstd = 1.f / sqrtf(running_var[i] + eps);
    stats[i] = gamma[i] * invstd;
    stats[c + i] = beta[i] - running_mean[i] * gamma[i] * invstd;
    stats[2 * c + i] = running_mean[i];
    stats[3 * c + i] = invstd;
}

template <typename T, bool RELU>
__global__ __launch_bounds__(kThreads) void bn_apply_kernel(const T* __restrict__ x, long m, int c, Geom g,
                                                            const float* __restrict__ stats, T* __restrict__ y) {
    constexpr int V = Vec<T>::V;
    const int col = threadIdx.x % g.cg, rlane = threadIdx.x / g.cg;
    x += (size_t)blockIdx.y * m * c; y += (size_t)blockIdx.y * m * c; stats += (size_t)blockIdx.y * 4 * c;
    float sc[V], sh[V];
#pragma unroll
    for (int j = 0; j < V; j++) { sc[j] = stats[col * V + j]; sh[j] = stats[c + col * V + j]; }
    const long stride = (long)gridDim.x * g.rl;
    for (long r = rlane < g.rl ? (long)blockIdx.x * g.rl + rlane : m; r < m; r += stride) {
        float v[V];
        Vec<T>::load(x + r * c + col * V, v);
#pragma unroll
        for (int j = 0; j < V; j++) {
            v[j] = fmaf(v[j], sc[j], sh[j]);
            if (RELU) v[j] = fmaxf(v[j], 0.f);
        }
        Vec<T>::store(y + r * c + col * V, v);
    }
}

// ---- backward ------------------------------------------------------------------------------------------------------------
// One copy of each pass's body, as in chain_bodies.h: the single calls (liso_bn_relu_bwd*, the InstanceNorm backward) and the grouped
// call (liso_bn_relu_bwd_multi) wrap the SAME reduce and dx bodies, so a (group, gradient) pair of the grouped call has the geometry,
// the per-thread row order, the LDS summation order and the instructions of the single call on that group's channels alone -- its
// results are the bits of the separate calls by construction.  NG = upstream gradients (1, or 2 for a map with two consumers: x and the
// ReLU mask are read once per row for both).  The kernels only find their block's pointers.

// rows [r0, r1) of one group: per gradient n, sum(dz) and sum(dz * xhat) per channel -> partial[n] = sums a [c] | sums b [c]
template <typename T, bool RELU, int NG>
__device__ __forceinline__ void bn_bwd_reduce_body(const T* __restrict__ x, const T* const (&dy)[NG], long xs, const long (&gs)[NG], int c,
                                                   int cg, int rl, const float* __restrict__ stats, long r0, long r1,
                                                   float (*s_a)[Vec<T>::V + 1], float (*s_b)[Vec<T>::V + 1], float* const (&partial)[NG]) {
    constexpr int V = Vec<T>::V;
    const int tid = threadIdx.x;
    const int col = tid % cg, rlane = tid / cg;
    float sc[V], sh[V], mu[V], is[V], a[NG][V], b[NG][V];
#pragma unroll
    for (int j = 0; j < V; j++) {
        sc[j] = stats[col * V + j]; sh[j] = stats[c + col * V + j];
        mu[j] = stats[2 * c + col * V + j]; is[j] = stats[3 * c + col * V + j];
#pragma unroll
        for (int n = 0; n < NG; n++) { a[n][j] = 0.f; b[n][j] = 0.f; }
    }
#pragma unroll 4
    for (long r = rlane < rl ? r0 + rlane : r1; r < r1; r += rl) {  // (rlane >= rl: C / V does not divide the block, idle lanes)
        float vx[V], vg[NG][V];
        Vec<T>::load(x + r * xs + col * V, vx);
#pragma unroll
        for (int n = 0; n < NG; n++) Vec<T>::load(dy[n] + r * gs[n] + col * V, vg[n]);
#pragma unroll
        for (int j = 0; j < V; j++) {
            const bool off = RELU && !(fmaf(vx[j], sc[j], sh[j]) > 0.f);  // ReLU mask recomputed from x
            const float xh = (vx[j] - mu[j]) * is[j];
#pragma unroll
            for (int n = 0; n < NG; n++) {
                const float dz = off ? 0.f : vg[n][j];
                a[n][j] += dz;
                b[n][j] = fmaf(dz, xh, b[n][j]);
            }
        }
    }
#pragma unroll
    for (int n = 0; n < NG; n++) {
        if (n) __syncthreads();  // (the previous gradient's reads of s_a / s_b)
#pragma unroll
        for (int j = 0; j < V; j++) { s_a[tid][j] = a[n][j]; s_b[tid][j] = b[n][j]; }
        __syncthreads();
        if (tid < c) {  // one thread per channel finishes the block: tid -> (col2, j2)
            const int col2 = tid / V, j2 = tid % V;
            float sa = 0.f, sb = 0.f;
            for (int q = 0; q < rl; q++) { sa += s_a[q * cg + col2][j2]; sb += s_b[q * cg + col2][j2]; }
            partial[n][tid] = sa;
            partial[n][c + tid] = sb;
        }
    }
}

// the value a store of T keeps, widened back (fp32: the value itself, made opaque so that the product in front of it is rounded
// before the sum of the two gradients' dx is formed -- never a fused multiply-add of one into the other)
template <typename T> __device__ __forceinline__ float stored(float v);
template <> __device__ __forceinline__ float stored<float>(float v) { asm volatile("" : "+v"(v)); return v; }
template <> __device__ __forceinline__ float stored<__hip_bfloat16>(float v) { return __bfloat162float(__float2bfloat16(v)); }
template <> __device__ __forceinline__ float stored<_Float16>(float v) { return liso_e16::F16::round(v); }

// rows blockIdx.x * rl + rlane, + gridDim.x * rl, ... < m of one group: dx = A * (dz - B - xhat * C) per gradient (coef[n] = A | B | C).
// Two gradients: each dx rounded to T as its own store would, then their sum rounded once more (the elementwise add of the two stored
// maps).
template <typename T, bool RELU, int NG>
__device__ __forceinline__ void bn_bwd_dx_body(const T* __restrict__ x, const T* const (&dy)[NG], long xs, const long (&gs)[NG], long m, int c,
                                               int cg, int rl, const float* __restrict__ stats, const float* const (&coef)[NG],
                                               T* __restrict__ dx, long ds) {
    constexpr int V = Vec<T>::V;
    const int col = threadIdx.x % cg, rlane = threadIdx.x / cg;
    float sc[V], sh[V], mu[V], is[V], A[NG][V], Bc[NG][V], Cc[NG][V];
#pragma unroll
    for (int j = 0; j < V; j++) {
        const int ch = col * V + j;
        sc[j] = stats[ch]; sh[j] = stats[c + ch]; mu[j] = stats[2 * c + ch]; is[j] = stats[3 * c + ch];
#pragma unroll
        for (int n = 0; n < NG; n++) { A[n][j] = coef[n][ch]; Bc[n][j] = coef[n][c + ch]; Cc[n][j] = coef[n][2 * c + ch]; }
    }
    const long stride = (long)gridDim.x * rl;
    for (long r = rlane < rl ? (long)blockIdx.x * rl + rlane : m; r < m; r += stride) {
        float vx[V], vg[NG][V];
        Vec<T>::load(x + r * xs + col * V, vx);
#pragma unroll
        for (int n = 0; n < NG; n++) Vec<T>::load(dy[n] + r * gs[n] + col * V, vg[n]);
#pragma unroll
        for (int j = 0; j < V; j++) {
#pragma unroll
            for (int n = 0; n < NG; n++) {
                float dz = vg[n][j];
                // (the test is spelled per gradient: hoisted out of this loop, the bf16 / ReLU / NG = 1 kernels get 88 registers for 80)
                if (RELU && !(fmaf(vx[j], sc[j], sh[j]) > 0.f)) dz = 0.f;
                vg[n][j] = A[n][j] * (dz - Bc[n][j] - (vx[j] - mu[j]) * is[j] * Cc[n][j]);
            }
            if constexpr (NG == 2) vg[0][j] = stored<T>(vg[0][j]) + stored<T>(vg[1][j]);
        }
        Vec<T>::store(dx + r * ds + col * V, vg[0]);
    }
}

// one BatchNorm (blockIdx.y = 0) or one InstanceNorm sample per blockIdx.y, one gradient
template <typename T, bool RELU>
__global__ __launch_bounds__(kThreads) void bn_bwd_reduce_kernel(const T* __restrict__ dy, const T* __restrict__ x, long m,
                                                                 int c, Geom g, const float* __restrict__ stats,
                                                                 float* partial) {
    constexpr int V = Vec<T>::V;
    __shared__ float s_a[kThreads][V + 1];
    __shared__ float s_b[kThreads][V + 1];
    const T* const dys[1] = {dy + (size_t)blockIdx.y * m * g.gs};
    const long gs[1] = {g.gs};
    float* const parts[1] = {partial + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 2 * c};
    const long r0 = (long)blockIdx.x * g.rows_per_block;
    const long r1 = r0 + g.rows_per_block < m ? r0 + g.rows_per_block : m;
    bn_bwd_reduce_body<T, RELU, 1>(x + (size_t)blockIdx.y * m * g.xs, dys, g.xs, gs, c, g.cg, g.rl, stats + (size_t)blockIdx.y * 4 * c, r0, r1,
                                   s_a, s_b, parts);
}

template <typename T, bool RELU>
__global__ __launch_bounds__(kThreads) void bn_bwd_dx_kernel(const T* __restrict__ dy, const T* __restrict__ x, long m, int c,
                                                             Geom g, const float* __restrict__ stats,
                                                             const float* __restrict__ coef, T* __restrict__ dx) {
    const T* const dys[1] = {dy + (size_t)blockIdx.y * m * g.gs};
    const long gs[1] = {g.gs};
    const float* const coefs[1] = {coef + (size_t)blockIdx.y * 3 * c};
    bn_bwd_dx_body<T, RELU, 1>(x + (size_t)blockIdx.y * m * g.xs, dys, g.xs, gs, m, c, g.cg, g.rl, stats + (size_t)blockIdx.y * 4 * c, coefs,
                               dx + (size_t)blockIdx.y * m * g.ds, g.ds);
}

// sums -> grad_beta, grad_gamma and the three dx coefficients per channel (chain_bodies.h: bn_bwd_finalize_segment)
// blockIdx.x = group (InstanceNorm sample), blockIdx.y = channel segment of `cw` channels (cw = c: one block per group)
__global__ __launch_bounds__(1024) void bn_bwd_finalize_kernel(liso_chain::BnBwdFinalizeArgs f) {
    __shared__ double sh_a[1024], sh_b[1024];
    liso_chain::bn_bwd_finalize_segment(f, blockIdx.x, blockIdx.y, sh_a, sh_b);
}

// A finalize launch's workgroups behind its segment blocks: the slab reduction of a deferred weight gradient, four of the reduction's
// 256-thread blocks per workgroup (`first`: this workgroup's first block of job j).  Nothing reads the weight gradient before the
// optimizer, but as a launch of its own the reduction (~8 us, bandwidth-bound) sat on the backward pass's dependent chain in front of
// the layer's data gradient; here the finalize (~5 us of dependent latency in a few blocks, dispatched first) runs in its shadow.  The
// roles share the launch and its 16 KB of LDS (finalize: 2 x 1024 doubles; reduction: 4 x (16 x 16 float4)) and nothing else: no flag,
// fence or atomic, and a block's role depends on blockIdx only.  PARTS: 16 / 1 as the launch was instantiated, 0: from the job's splits.
template <int PARTS>
__device__ __forceinline__ void ride_wgrad_reduce(const liso_wgrad_reduce_job& j, long first, long n_red, double* sh) {
    const int quarter = threadIdx.x >> 8;
    const long bid = first + quarter;
    float4(*red)[16] = reinterpret_cast<float4(*)[16]>(sh) + quarter * 16;
    if (PARTS == 16 || (PARTS == 0 && j.splits > 16)) liso_chain::wgrad_reduce_block<16>(j, bid, threadIdx.x & 255, red, bid < n_red);
    else liso_chain::wgrad_reduce_block<1>(j, bid, threadIdx.x & 255, red, bid < n_red);
}

// the finalize of ONE BatchNorm (blocks [0, n_fin): the channel segments) with one riding reduction
template <int PARTS>
__global__ __launch_bounds__(1024) void bn_bwd_finalize_reduce_kernel(liso_chain::BnBwdFinalizeArgs f, int n_fin,
                                                                      liso_wgrad_reduce_job j, long n_red) {
    __shared__ double sh[2048];
    if ((int)blockIdx.x < n_fin) liso_chain::bn_bwd_finalize_segment(f, 0, blockIdx.x, sh, sh + 1024);
    else ride_wgrad_reduce<PARTS>(j, (long)(blockIdx.x - n_fin) * 4, n_red, sh);
}

// channel segment of the finalize launch: 32 where the channel count allows and there are enough partial sums to spread
inline int finalize_segment(int c, int nblk) { return (c % 32 == 0 && c > 32 && nblk >= 64) ? 32 : c; }

// InstanceNorm: the affine parameters are shared by all samples -> one block walks the groups (samples) in order, writes every
// group's dx coefficients and the SUM of the per-sample parameter gradients (fixed order): no [groups, C] intermediate and no
// reduction launches behind the call
__global__ __launch_bounds__(1024) void in_bwd_finalize_sum_kernel(const float* __restrict__ partial, int groups, int nblk, long m, int c,
                                                                   const float* __restrict__ gamma, const float* __restrict__ stats,
                                                                   float* __restrict__ grad_gamma, float* __restrict__ grad_beta,
                                                                   float* __restrict__ coef) {
    __shared__ double sh_a[1024], sh_b[1024];
    const int tid = threadIdx.x;
    const int chunks = 1024 / c > 0 ? 1024 / c : 1;
    const int ch = tid % c, chunk = tid / c;
    double sum_a = 0.0, sum_b = 0.0;
    for (int g = 0; g < groups; g++) {
        const float* part = partial + (size_t)g * nblk * 2 * c;
        double a = 0.0, b = 0.0;
        if (chunk < chunks) {
            const int per = (nblk + chunks - 1) / chunks;
            const int lo = chunk * per, hi = lo + per < nblk ? lo + per : nblk;
            int q = lo;
            for (; q + 8 <= hi; q += 8) {
                float va[8], vb[8];
#pragma unroll
                for (int j = 0; j < 8; j++) { va[j] = part[(size_t)(q + j) * 2 * c + ch]; vb[j] = part[(size_t)(q + j) * 2 * c + c + ch]; }
#pragma unroll
                for (int j = 0; j < 8; j++) { a += (double)va[j]; b += (double)vb[j]; }
            }
            for (; q < hi; q++) { a += (double)part[(size_t)q * 2 * c + ch]; b += (double)part[(size_t)q * 2 * c + c + ch]; }
        }
        __syncthreads();  // (the previous group's reads of sh_a / sh_b)
        sh_a[tid] = a; sh_b[tid] = b;
        __syncthreads();
        if (tid < c) {
            a = 0.0; b = 0.0;
            for (int q = 0; q < chunks; q++) { a += sh_a[q * c + tid]; b += sh_b[q * c + tid]; }
            // (the per-sample values rounded to fp32 first, then added: what `grad[groups, C].sum(0)` of the three-step form computes)
            sum_a += (double)(float)a; sum_b += (double)(float)b;
            float* cf = coef + (size_t)g * 3 * c;
            cf[tid] = gamma[tid] * stats[(size_t)g * 4 * c + 3 * c + tid];
            cf[c + tid] = (float)(a / (double)m);
            cf[2 * c + tid] = (float)(b / (double)m);
        }
    }
    if (tid < c) { grad_beta[tid] = (float)sum_a; grad_gamma[tid] = (float)sum_b; }
}

inline bool geom(int c, int v, long m, Geom* g, int* nblk) {
    if (c <= 0 || c % v != 0 || c > kThreads) return false;
    const int cg = c / v;
    if (cg > kThreads) return false;
    g->cg = cg;
    g->rl = kThreads / cg;
    // ~256 blocks (1 per CU) keeps the single-block finalize short; never fewer than kRowsPerBlock rows per block
    long rpb = (m + 255) / 256;
    if (rpb < kRowsPerBlock) rpb = kRowsPerBlock;
    long nb = (m + rpb - 1) / rpb;
    if (nb > kMaxBlocks) { rpb = (m + kMaxBlocks - 1) / kMaxBlocks; nb = (m + rpb - 1) / rpb; }
    g->rows_per_block = rpb;
    g->xs = g->gs = g->ds = c;
    *nblk = (int)(nb > 0 ? nb : 1);
    return true;
}

inline int stream_grid(long m, const Geom& g) {
    long nb = (m + g.rl - 1) / g.rl;
    return (int)(nb < 8192 ? (nb > 0 ? nb : 1) : 8192);
}

// ---- grouped backward with one or two upstream gradients (include/liso_bn.h: liso_bn_relu_bwd_multi) -----------------------------
// Up to four BatchNorms over channel ranges of ONE raw tensor, and up to two gradients arriving at it (a map with two consumers), in the
// three launches of a single call: blockIdx.y = group, whose geometry and pointers come from the table.
struct MultiGroup {
    int c_off, c;          // channel range inside a row of x / dy / dx
    int cg, rl;            // Geom of this group's channel count
    int cw, seg0;          // finalize: channels per segment, first block of this group's segments
    const float* gamma;
    const float* stats;
    float *grad_gamma, *grad_beta;
    float* partial[2];     // per gradient: [nblk][2 * c]
    float* coef[2];        // per gradient: [3 * c]
    float* pgrad[2];       // two gradients: this gradient's grad_gamma | grad_beta [2 * c], added by the block that wrote both
};
struct MultiArgs {
    MultiGroup g[LISO_BN_MAX_GROUPS];
    int n_groups, nblk, training;
    long m, rows_per_block;
    long xs, gs[2], ds;
};

template <typename T, bool RELU, int NG>
__global__ __launch_bounds__(kThreads) void bn_bwd_multi_reduce_kernel(const T* __restrict__ dy_a, const T* __restrict__ dy_b,
                                                                       const T* __restrict__ x, MultiArgs A) {
    constexpr int V = Vec<T>::V;
    __shared__ float s_a[kThreads][V + 1];
    __shared__ float s_b[kThreads][V + 1];
    const MultiGroup& G = A.g[blockIdx.y];
    const T* dys[NG];
    long gs[NG];
    float* parts[NG];
#pragma unroll
    for (int n = 0; n < NG; n++) {
        dys[n] = (n ? dy_b : dy_a) + G.c_off; gs[n] = A.gs[n];
        parts[n] = G.partial[n] + (size_t)blockIdx.x * 2 * G.c;
    }
    const long r0 = (long)blockIdx.x * A.rows_per_block;
    const long r1 = r0 + A.rows_per_block < A.m ? r0 + A.rows_per_block : A.m;
    bn_bwd_reduce_body<T, RELU, NG>(x + G.c_off, dys, A.xs, gs, G.c, G.cg, G.rl, G.stats, r0, r1, s_a, s_b, parts);
}

// blocks [0, n_fin): one channel segment of one group each -- bn_bwd_finalize_segment per gradient; with two gradients each writes its
// parameter gradients to scratch and the thread that wrote both adds them (fp32: what autograd's add of the second contribution onto
// the first gives).  Behind them the workgroups of up to two riding reductions, job 0's first.
template <int NG>
__global__ __launch_bounds__(1024) void bn_bwd_multi_finalize_kernel(MultiArgs A, int n_fin, liso_wgrad_reduce_job j0, long n_red0,
                                                                     liso_wgrad_reduce_job j1, long n_red1) {
    __shared__ double sh[2048];
    if ((int)blockIdx.x < n_fin) {
        int k = 0;
        while (k + 1 < A.n_groups && (int)blockIdx.x >= A.g[k + 1].seg0) k++;
        const MultiGroup& G = A.g[k];
        const int seg = (int)blockIdx.x - G.seg0;
#pragma unroll
        for (int n = 0; n < NG; n++) {
            if (n) __syncthreads();  // (the previous gradient's reads of sh)
            const liso_chain::BnBwdFinalizeArgs f{G.partial[n], A.nblk, A.m, G.c, G.cw, G.gamma, G.stats, A.training,
                                                  NG == 2 ? G.pgrad[n] : G.grad_gamma, NG == 2 ? G.pgrad[n] + G.c : G.grad_beta, G.coef[n]};
            liso_chain::bn_bwd_finalize_segment(f, 0, seg, sh, sh + 1024);
        }
        if (NG == 2 && (int)threadIdx.x < G.cw) {  // (this thread's own stores above)
            const int ch = seg * G.cw + threadIdx.x;
            G.grad_gamma[ch] = G.pgrad[0][ch] + G.pgrad[1][ch];
            G.grad_beta[ch] = G.pgrad[0][G.c + ch] + G.pgrad[1][G.c + ch];
        }
        return;
    }
    // (job 0's workgroups are whole: a workgroup serves one job, its barriers stay uniform)
    const long wg = (long)(blockIdx.x - n_fin), wg0 = (n_red0 + 3) / 4;
    if (wg < wg0) ride_wgrad_reduce<0>(j0, wg * 4, n_red0, sh);
    else ride_wgrad_reduce<0>(j1, (wg - wg0) * 4, n_red1, sh);
}

template <typename T, bool RELU, int NG>
__global__ __launch_bounds__(kThreads) void bn_bwd_multi_dx_kernel(const T* __restrict__ dy_a, const T* __restrict__ dy_b,
                                                                   const T* __restrict__ x, MultiArgs A, T* __restrict__ dx) {
    const MultiGroup& G = A.g[blockIdx.y];
    const T* dys[NG];
    long gs[NG];
    const float* coefs[NG];
#pragma unroll
    for (int n = 0; n < NG; n++) { dys[n] = (n ? dy_b : dy_a) + G.c_off; gs[n] = A.gs[n]; coefs[n] = G.coef[n]; }
    bn_bwd_dx_body<T, RELU, NG>(x + G.c_off, dys, A.xs, gs, A.m, G.c, G.cg, G.rl, G.stats, coefs, dx + G.c_off, A.ds);
}

// the three kernel templates of an entry point are instantiated per element type and ReLU flag: f(T{}, std::bool_constant<RELU>{})
template <typename F>
inline void with_elem_relu(int elem, int relu, F&& f) {
    auto r = [&](auto t) { if (relu) f(t, std::true_type{}); else f(t, std::false_type{}); };
    if (elem == LISO_ELEM_F16) r(_Float16{});
    else if (elem) r(__hip_bfloat16{});
    else r(float{});
}

}  // namespace

extern "C" {

size_t liso_bn_workspace_bytes(int c) {
    if (c <= 0) return 0;
    return ((size_t)kMaxBlocks * 2 * c + 3 * (size_t)c) * sizeof(float);
}

int liso_bn_relu_fwd(const void* x, int is_bf16, long m, int c, const float* gamma, const float* beta,
                     float* running_mean, float* running_var, float momentum, float eps, int training, int relu,
                     void* y, float* stats, void* workspace, size_t workspace_bytes, void* stream) {
    Geom g;
    int nblk;
    if (!elem_ok(is_bf16) || m < 0 || !geom(c, is_bf16 ? 8 : 4, m, &g, &nblk)) return LISO_EINVAL;
    if (!gamma || !beta || !running_mean || !running_var || !stats || !workspace || (m > 0 && (!x || !y))) return LISO_EINVAL;
    if (workspace_bytes < liso_bn_workspace_bytes(c)) return LISO_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    float* partial = (float*)workspace;
    if (training) {
        if (m == 0) return LISO_EINVAL;
        if (is_bf16 == LISO_ELEM_F16)
            bn_stats_kernel<_Float16><<<nblk, kThreads, 0, st>>>((const _Float16*)x, m, c, g, partial);
        else if (is_bf16)
            bn_stats_kernel<__hip_bfloat16><<<nblk, kThreads, 0, st>>>((const __hip_bfloat16*)x, m, c, g, partial);
        else
            bn_stats_kernel<float><<<nblk, kThreads, 0, st>>>((const float*)x, m, c, g, partial);
        bn_finalize_kernel<<<1, 1024, 0, st>>>(partial, nblk, m, c, g.rows_per_block, gamma, beta, running_mean, running_var,
                                               momentum, eps, stats);
    } else {
        bn_eval_stats_kernel<<<(c + 255) / 256, 256, 0, st>>>(c, gamma, beta, running_mean, running_var, eps, stats);
    }
    if (m > 0) {
        const int grid = stream_grid(m, g);
        with_elem_relu(is_bf16, relu, [&](auto t, auto r) {
            using T = decltype(t);
            bn_apply_kernel<T, decltype(r)::value><<<grid, kThreads, 0, st>>>((const T*)x, m, c, g, stats, (T*)y);
        });
    }
    return check_launch();
}

static int bn_relu_bwd(const void* dy, const void* x, int is_bf16, long m, int c, const float* gamma, const float* stats,
                       int training, int relu, void* dx, float* grad_gamma, float* grad_beta, void* workspace,
                       size_t workspace_bytes, void* stream, long dy_stride = 0, long x_stride = 0, long dx_stride = 0,
                       const liso_wgrad_reduce_job* job = nullptr) {
    Geom g;
    int nblk;
    if (!elem_ok(is_bf16) || m <= 0 || !geom(c, is_bf16 ? 8 : 4, m, &g, &nblk)) return LISO_EINVAL;
    if (dy_stride || x_stride || dx_stride) {  // rows that are channel slices of wider channels-last tensors
        const int v = is_bf16 ? 8 : 4;
        if (dy_stride < c || x_stride < c || dx_stride < c || dy_stride % v || x_stride % v || dx_stride % v) return LISO_EINVAL;
        if ((((uintptr_t)dy | (uintptr_t)x | (uintptr_t)dx) & 15) != 0) return LISO_EINVAL;
        g.gs = dy_stride; g.xs = x_stride; g.ds = dx_stride;
    }
    if (!dy || !x || !gamma || !stats || !dx || !grad_gamma || !grad_beta || !workspace) return LISO_EINVAL;
    if (workspace_bytes < liso_bn_workspace_bytes(c)) return LISO_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    float* partial = (float*)workspace;
    float* coef = partial + (size_t)kMaxBlocks * 2 * c;
    const int grid = stream_grid(m, g);
    const int cw = finalize_segment(c, nblk);
    const liso_chain::BnBwdFinalizeArgs fa{partial, nblk, m, c, cw, gamma, stats, training, grad_gamma, grad_beta, coef};
    const int n_fin = c / cw;
    const long n_red = job ? liso_chain::wgrad_reduce_blocks(*job) : 0;
    const unsigned grid_fr = (unsigned)(n_fin + (n_red + 3) / 4);
    with_elem_relu(is_bf16, relu, [&](auto t, auto r) {
        using T = decltype(t);
        constexpr bool R = decltype(r)::value;
        bn_bwd_reduce_kernel<T, R><<<nblk, kThreads, 0, st>>>((const T*)dy, (const T*)x, m, c, g, stats, partial);
        if (job && job->splits > 16)
            bn_bwd_finalize_reduce_kernel<16><<<grid_fr, 1024, 0, st>>>(fa, n_fin, *job, n_red);
        else if (job)
            bn_bwd_finalize_reduce_kernel<1><<<grid_fr, 1024, 0, st>>>(fa, n_fin, *job, n_red);
        else
            bn_bwd_finalize_kernel<<<dim3(1, c / cw), 1024, 0, st>>>(fa);
        bn_bwd_dx_kernel<T, R><<<grid, kThreads, 0, st>>>((const T*)dy, (const T*)x, m, c, g, stats, coef, (T*)dx);
    });
    return check_launch();
}

int liso_bn_relu_bwd(const void* dy, const void* x, int is_bf16, long m, int c, const float* gamma, const float* stats,
                     int training, int relu, void* dx, float* grad_gamma, float* grad_beta, void* workspace,
                     size_t workspace_bytes, void* stream) {
    return bn_relu_bwd(dy, x, is_bf16, m, c, gamma, stats, training, relu, dx, grad_gamma, grad_beta, workspace, workspace_bytes,
                       stream);
}

int liso_bn_relu_bwd_strided(const void* dy, long dy_stride, const void* x, long x_stride, int is_bf16, long m, int c, const float* gamma,
                             const float* stats, int training, int relu, void* dx, long dx_stride, float* grad_gamma, float* grad_beta,
                             void* workspace, size_t workspace_bytes, void* stream) {
    if (dy_stride <= 0 || x_stride <= 0 || dx_stride <= 0) return LISO_EINVAL;
    return bn_relu_bwd(dy, x, is_bf16, m, c, gamma, stats, training, relu, dx, grad_gamma, grad_beta, workspace, workspace_bytes,
                       stream, dy_stride, x_stride, dx_stride);
}

int liso_bn_relu_bwd_chained(const void* dy, long dy_stride, const void* x, long x_stride, int is_bf16, long m, int c, const float* gamma,
                             const float* stats, int training, int relu, void* dx, long dx_stride, float* grad_gamma, float* grad_beta,
                             void* workspace, size_t workspace_bytes, const liso_wgrad_reduce_job* job, void* stream) {
    if (dy_stride < 0 || x_stride < 0 || dx_stride < 0 || ((dy_stride == 0) != (x_stride == 0)) || ((dy_stride == 0) != (dx_stride == 0)))
        return LISO_EINVAL;
    if (job && !liso_chain::wgrad_reduce_job_ok(job)) return LISO_EINVAL;
    return bn_relu_bwd(dy, x, is_bf16, m, c, gamma, stats, training, relu, dx, grad_gamma, grad_beta, workspace, workspace_bytes,
                       stream, dy_stride, x_stride, dx_stride, job);
}

// floats of workspace per (group, gradient): partial sums | dx coefficients | this gradient's parameter gradients
static inline size_t multi_pair_floats(int c) { return (size_t)kMaxBlocks * 2 * c + 5 * (size_t)c; }

size_t liso_bn_multi_workspace_bytes(const liso_bn_group* groups, int n_groups, int n_grads) {
    if (!groups || n_groups < 1 || n_groups > LISO_BN_MAX_GROUPS || n_grads < 1 || n_grads > 2) return 0;
    size_t n = 0;
    for (int k = 0; k < n_groups; k++) {
        if (groups[k].c <= 0 || groups[k].c > kThreads) return 0;
        n += (size_t)n_grads * multi_pair_floats(groups[k].c);
    }
    return n * sizeof(float);
}

// the table of a grouped call: geometry per group, finalize segments in group order.  Host only; liso_bn_relu_bwd_multi_check exposes
// its refusals.
static int multi_table(const liso_bn_group* groups, int n_groups, int n_grads, int elem, long m, long x_stride, long dy_a_stride,
                       long dy_b_stride, long dx_stride, MultiArgs* A, int* n_fin, int* grid_dx) {
    if (!elem_ok(elem) || m <= 0 || !groups || n_groups < 1 || n_groups > LISO_BN_MAX_GROUPS || n_grads < 1 || n_grads > 2)
        return LISO_EINVAL;
    const int v = elem ? 8 : 4;
    const long strides[4] = {x_stride, dy_a_stride, dx_stride, n_grads == 2 ? dy_b_stride : dy_a_stride};
    for (long s : strides)
        if (s <= 0 || s % v) return LISO_EINVAL;
    int seg = 0, gdx = 1, end = 0;
    for (int k = 0; k < n_groups; k++) {
        const liso_bn_group& g = groups[k];
        Geom ge;
        int nblk;
        if (!geom(g.c, v, m, &ge, &nblk)) return LISO_EINVAL;  // (c <= 256, whole 16-B lanes)
        if (g.c_off < end || g.c_off % v) return LISO_EINVAL;   // ascending, disjoint channel ranges on 16-B boundaries
        end = g.c_off + g.c;
        for (long s : strides)
            if (end > s) return LISO_EINVAL;
        if (!g.gamma || !g.stats || !g.grad_gamma || !g.grad_beta) return LISO_EINVAL;
        MultiGroup& G = A->g[k];
        G.c_off = g.c_off; G.c = g.c; G.cg = ge.cg; G.rl = ge.rl;
        G.cw = finalize_segment(g.c, nblk); G.seg0 = seg;
        G.gamma = g.gamma; G.stats = g.stats; G.grad_gamma = g.grad_gamma; G.grad_beta = g.grad_beta;
        seg += g.c / G.cw;
        const int sg = stream_grid(m, ge);
        if (sg > gdx) gdx = sg;
        A->nblk = nblk; A->rows_per_block = ge.rows_per_block;  // (functions of m alone: the same for every group)
    }
    A->n_groups = n_groups; A->m = m;
    A->xs = x_stride; A->gs[0] = dy_a_stride; A->gs[1] = n_grads == 2 ? dy_b_stride : 0; A->ds = dx_stride;
    *n_fin = seg; *grid_dx = gdx;
    return LISO_OK;
}

int liso_bn_relu_bwd_multi_check(const liso_bn_group* groups, int n_groups, int n_grads, int elem, long m, long x_stride,
                                 long dy_a_stride, long dy_b_stride, long dx_stride, int* n_finalize_blocks) {
    MultiArgs A{};
    int n_fin = 0, gdx = 0;
    const int rc = multi_table(groups, n_groups, n_grads, elem, m, x_stride, dy_a_stride, dy_b_stride, dx_stride, &A, &n_fin, &gdx);
    if (rc == LISO_OK && n_finalize_blocks) *n_finalize_blocks = n_fin;
    return rc;
}

int liso_bn_relu_bwd_multi(const void* dy_a, long dy_a_stride, const void* dy_b, long dy_b_stride, const void* x, long x_stride, int elem,
                           long m, const liso_bn_group* groups, int n_groups, int training, int relu, void* dx, long dx_stride,
                           void* workspace, size_t workspace_bytes, const liso_wgrad_reduce_job* job_a, const liso_wgrad_reduce_job* job_b,
                           void* stream) {
    const int ng = dy_b ? 2 : 1;
    MultiArgs A{};
    int n_fin = 0, gdx = 0;
    const int rc = multi_table(groups, n_groups, ng, elem, m, x_stride, dy_a_stride, dy_b_stride, dx_stride, &A, &n_fin, &gdx);
    if (rc != LISO_OK) return rc;
    if (!dy_a || !x || !dx || !workspace) return LISO_EINVAL;
    if ((((uintptr_t)dy_a | (uintptr_t)dy_b | (uintptr_t)x | (uintptr_t)dx) & 15) != 0) return LISO_EINVAL;
    if (!job_a && job_b) { job_a = job_b; job_b = nullptr; }
    if ((job_a && !liso_chain::wgrad_reduce_job_ok(job_a)) || (job_b && !liso_chain::wgrad_reduce_job_ok(job_b))) return LISO_EINVAL;
    if (workspace_bytes < liso_bn_multi_workspace_bytes(groups, n_groups, ng)) return LISO_EWORKSPACE;
    float* w = (float*)workspace;
    for (int k = 0; k < n_groups; k++)
        for (int n = 0; n < ng; n++) {
            MultiGroup& G = A.g[k];
            G.partial[n] = w;
            G.coef[n] = w + (size_t)kMaxBlocks * 2 * G.c;
            G.pgrad[n] = G.coef[n] + 3 * (size_t)G.c;
            w += multi_pair_floats(G.c);
        }
    A.training = training;
    hipStream_t st = (hipStream_t)stream;
    const liso_wgrad_reduce_job none{};
    const long n_red0 = job_a ? liso_chain::wgrad_reduce_blocks(*job_a) : 0, n_red1 = job_b ? liso_chain::wgrad_reduce_blocks(*job_b) : 0;
    const unsigned grid_f = (unsigned)(n_fin + (n_red0 + 3) / 4 + (n_red1 + 3) / 4);
    const dim3 grid_r((unsigned)A.nblk, (unsigned)n_groups), grid_d((unsigned)gdx, (unsigned)n_groups);
    with_elem_relu(elem, relu, [&](auto t, auto r) {
        using T = decltype(t);
        constexpr bool R = decltype(r)::value;
        auto launch = [&](auto n) {
            constexpr int N = decltype(n)::value;
            bn_bwd_multi_reduce_kernel<T, R, N><<<grid_r, kThreads, 0, st>>>((const T*)dy_a, (const T*)dy_b, (const T*)x, A);
            bn_bwd_multi_finalize_kernel<N><<<grid_f, 1024, 0, st>>>(A, n_fin, job_a ? *job_a : none, n_red0, job_b ? *job_b : none, n_red1);
            bn_bwd_multi_dx_kernel<T, R, N><<<grid_d, kThreads, 0, st>>>((const T*)dy_a, (const T*)dy_b, (const T*)x, A, (T*)dx);
        };
        if (ng == 2) launch(std::integral_constant<int, 2>{});
        else launch(std::integral_constant<int, 1>{});
    });
    return check_launch();
}

size_t liso_in_workspace_bytes(int groups, int c) {
    if (groups <= 0 || c <= 0) return 0;
    return (size_t)groups * liso_bn_workspace_bytes(c);
}

int liso_in_relu_fwd(const void* x, int is_bf16, int groups, long m, int c, const float* gamma, const float* beta, float eps, int relu,
                     void* y, float* stats, void* workspace, size_t workspace_bytes, void* stream) {
    Geom g;
    int nblk;
    if ((is_bf16 != LISO_ELEM_F32 && is_bf16 != LISO_ELEM_BF16) || groups < 1 || m <= 0 || !geom(c, is_bf16 ? 8 : 4, m, &g, &nblk))
        return LISO_EINVAL;  // (InstanceNorm: SLIM's encoders, fp32 / bf16 only)
    if (!gamma || !beta || !stats || !workspace || !x || !y) return LISO_EINVAL;
    if (workspace_bytes < liso_in_workspace_bytes(groups, c)) return LISO_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    float* partial = (float*)workspace;
    const dim3 gs((unsigned)nblk, (unsigned)groups), ga((unsigned)stream_grid(m, g), (unsigned)groups);
    if (is_bf16)
        bn_stats_kernel<__hip_bfloat16><<<gs, kThreads, 0, st>>>((const __hip_bfloat16*)x, m, c, g, partial);
    else
        bn_stats_kernel<float><<<gs, kThreads, 0, st>>>((const float*)x, m, c, g, partial);
    bn_finalize_kernel<<<groups, 1024, 0, st>>>(partial, nblk, m, c, g.rows_per_block, gamma, beta, nullptr, nullptr, 0.f, eps, stats);
    with_elem_relu(is_bf16, relu, [&](auto t, auto r) {  // (fp32 / bf16: checked above)
        using T = decltype(t);
        bn_apply_kernel<T, decltype(r)::value><<<ga, kThreads, 0, st>>>((const T*)x, m, c, g, stats, (T*)y);
    });
    return check_launch();
}

static int in_relu_bwd(const void* dy, const void* x, int is_bf16, int groups, long m, int c, const float* gamma, const float* stats,
                     int relu, void* dx, float* grad_gamma, float* grad_beta, void* workspace, size_t workspace_bytes, int summed, void* stream) {
    Geom g;
    int nblk;
    if ((is_bf16 != LISO_ELEM_F32 && is_bf16 != LISO_ELEM_BF16) || groups < 1 || m <= 0 || !geom(c, is_bf16 ? 8 : 4, m, &g, &nblk))
        return LISO_EINVAL;  // (InstanceNorm: SLIM's encoders, fp32 / bf16 only)
    if (!dy || !x || !gamma || !stats || !dx || !grad_gamma || !grad_beta || !workspace) return LISO_EINVAL;
    if (workspace_bytes < liso_in_workspace_bytes(groups, c)) return LISO_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    float* partial = (float*)workspace;
    float* coef = partial + (size_t)groups * kMaxBlocks * 2 * c;
    const dim3 gs((unsigned)nblk, (unsigned)groups), ga((unsigned)stream_grid(m, g), (unsigned)groups);
    const int cw = finalize_segment(c, nblk);
    const liso_chain::BnBwdFinalizeArgs fa{partial, nblk, m, c, cw, gamma, stats, 1, grad_gamma, grad_beta, coef};
    with_elem_relu(is_bf16, relu, [&](auto t, auto r) {  // (fp32 / bf16: checked above)
        using T = decltype(t);
        constexpr bool R = decltype(r)::value;
        bn_bwd_reduce_kernel<T, R><<<gs, kThreads, 0, st>>>((const T*)dy, (const T*)x, m, c, g, stats, partial);
        if (summed)
            in_bwd_finalize_sum_kernel<<<1, 1024, 0, st>>>(partial, groups, nblk, m, c, gamma, stats, grad_gamma, grad_beta, coef);
        else
            bn_bwd_finalize_kernel<<<dim3(groups, c / cw), 1024, 0, st>>>(fa);
        bn_bwd_dx_kernel<T, R><<<ga, kThreads, 0, st>>>((const T*)dy, (const T*)x, m, c, g, stats, coef, (T*)dx);
    });
    return check_launch();
}

int liso_in_relu_bwd(const void* dy, const void* x, int is_bf16, int groups, long m, int c, const float* gamma, const float* stats,
                     int relu, void* dx, float* grad_gamma, float* grad_beta, void* workspace, size_t workspace_bytes, void* stream) {
    return in_relu_bwd(dy, x, is_bf16, groups, m, c, gamma, stats, relu, dx, grad_gamma, grad_beta, workspace, workspace_bytes, 0, stream);
}

int liso_in_relu_bwd_sum(const void* dy, const void* x, int is_bf16, int groups, long m, int c, const float* gamma, const float* stats,
                         int relu, void* dx, float* grad_gamma, float* grad_beta, void* workspace, size_t workspace_bytes, void* stream) {
    return in_relu_bwd(dy, x, is_bf16, groups, m, c, gamma, stats, relu, dx, grad_gamma, grad_beta, workspace, workspace_bytes, 1, stream);
}

}  // extern "C"
