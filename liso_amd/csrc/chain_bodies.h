// Block bodies shared by two translation units: the weight-gradient slab reduction (conv_wgrad.hip) and the BatchNorm-backward
// finalize (bn.hip), each launched on its own AND as the two roles of one combined launch (bn.hip: bn_bwd_finalize_reduce_kernel,
// include/liso_bn.h: liso_bn_relu_bwd_chained).  One copy of each body: a block does the same loads, additions and stores whichever
// kernel it belongs to, so the results of the combined launch are the bits of the separate ones.
#ifndef LISO_CHAIN_BODIES_H
#define LISO_CHAIN_BODIES_H

#include <hip/hip_runtime.h>

#include "../../include/liso_conv.h"

namespace liso_chain {

// dw (torch layout) = sum over splits of the slabs, in a fixed order.  PARTS = 16: block = one (tap, k) row x 64 output channels;
// thread = 4 consecutive channels (one 16-B load per split) x one of 16 split groups (group g adds splits g, g + 16, ... in that
// order, four loads in flight), then the 16 group sums are added pairwise in a fixed tree.  PARTS = 1 (<= 16 splits): block = 16
// rows x 64 channels, every thread walks all splits of its 4 channels (all loads in flight), no tree.  The slabs were written a
// moment ago and sit in L2 / the Infinity Cache; what the reduction needs is bytes in flight (the former version: one 4-B load at a
// time per thread, 2 TB/s on 37 MB of slabs).
// `bid` / `tid`: the index of this 256-thread block of the reduction and the thread's index in it (a 1024-thread launch carries four
// such blocks per workgroup); `red`: the block's own 16 x 16 float4 of LDS; `live` = false: the block takes part in the barriers only.
template <int PARTS>
__device__ __forceinline__ void wgrad_reduce_block(const liso_wgrad_reduce_job& j, long bid, int tid, float4 (*red)[16], bool live) {
    constexpr int RPB = 16 / PARTS;  // rows per block
    const float* __restrict__ slab = j.slab;
    const float* __restrict__ bias_slab = j.bias_slab;
    float* __restrict__ dw = j.dw;
    float* __restrict__ dbias = j.dbias;
    const int taps = j.taps, ci = j.ci, co = j.co;
    const long cip = j.cip, cop = j.cop;
    const int c4 = tid & 15, part = PARTS == 16 ? tid >> 4 : 0, rib = PARTS == 16 ? 0 : tid >> 4;
    const int n_tiles = (co + 63) / 64;
    const long rows = (long)taps * ci;
    const long row_blocks = (rows + RPB - 1) / RPB;
    const bool is_bias = bid >= row_blocks * n_tiles;
    if (is_bias && !dbias) live = false;
    const int ntile = (int)(is_bias ? bid - row_blocks * n_tiles : bid % n_tiles);
    const long row = is_bias ? 0 : (bid / n_tiles) * RPB + rib;  // tap * ci + k
    const bool row_ok = live && (is_bias ? rib == 0 : row < rows);
    const int k = (int)(row % ci), tap = (int)(row / ci);
    const int n = ntile * 64 + c4 * 4;
    const int count = is_bias ? j.bias_rows : j.splits;
    const float* src = is_bias ? bias_slab + n : slab + ((long)tap * cip + k) * cop + n;
    const long stride = is_bias ? cop : (long)taps * cip * cop;
    float4 s = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (n < co && row_ok) {
        int sp = part;
        for (; sp + 3 * PARTS < count; sp += 4 * PARTS) {  // four loads in flight per thread
            const float4 v0 = *reinterpret_cast<const float4*>(src + (long)sp * stride);
            const float4 v1 = *reinterpret_cast<const float4*>(src + (long)(sp + PARTS) * stride);
            const float4 v2 = *reinterpret_cast<const float4*>(src + (long)(sp + 2 * PARTS) * stride);
            const float4 v3 = *reinterpret_cast<const float4*>(src + (long)(sp + 3 * PARTS) * stride);
            s.x = (((s.x + v0.x) + v1.x) + v2.x) + v3.x;
            s.y = (((s.y + v0.y) + v1.y) + v2.y) + v3.y;
            s.z = (((s.z + v0.z) + v1.z) + v2.z) + v3.z;
            s.w = (((s.w + v0.w) + v1.w) + v2.w) + v3.w;
        }
        for (; sp < count; sp += PARTS) {
            const float4 v = *reinterpret_cast<const float4*>(src + (long)sp * stride);
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
    }
    if constexpr (PARTS == 16) {
        red[part][c4] = s;
        __syncthreads();
#pragma unroll
        for (int w = 8; w >= 1; w >>= 1) {  // fixed pairing: (p, p + w)
            if (part < w) {
                const float4 o = red[part + w][c4];
                s.x += o.x; s.y += o.y; s.z += o.z; s.w += o.w;
                red[part][c4] = s;
            }
            __syncthreads();
        }
    }
    if (part == 0 && n < co && row_ok) {
        const float v[4] = {s.x, s.y, s.z, s.w};
#pragma unroll
        for (int e = 0; e < 4; e++) {
            if (n + e >= co) break;
            if (is_bias)
                dbias[n + e] = v[e];
            else
                dw[j.transposed ? (((long)k * co + n + e) * taps + tap) : (((long)(n + e) * ci + k) * taps + tap)] = v[e];
        }
    }
}

// 256-thread blocks of a job's reduction (the bias row's blocks behind the weight rows')
inline long wgrad_reduce_blocks(const liso_wgrad_reduce_job& j) {
    const long rows = (long)j.taps * j.ci;
    const int n_tiles = (j.co + 63) / 64;
    return j.splits > 16 ? (rows + (j.dbias ? 1 : 0)) * n_tiles : ((rows + 15) / 16 + (j.dbias ? 1 : 0)) * n_tiles;
}

inline bool wgrad_reduce_job_ok(const liso_wgrad_reduce_job* j) {
    if (!j || !j->slab || !j->dw || (j->dbias && !j->bias_slab)) return false;
    if (j->splits <= 0 || j->taps <= 0 || j->ci <= 0 || j->co <= 0 || (j->dbias && j->bias_rows <= 0)) return false;
    if (j->cip < j->ci || j->cop < j->co || j->cop % 4) return false;  // (a thread reads the 16 B of 4 channels n .. n + 3, n < co)
    const long blocks = wgrad_reduce_blocks(*j);
    return blocks > 0 && blocks < (1L << 30);
}

// sums -> grad_beta, grad_gamma and the three dx coefficients per channel: dx = A * (dz - B - xhat * Cc)
// One 1024-thread block per (group = InstanceNorm sample, channel segment `seg` of `cw` channels; cw = c: one block per group).  With
// 32-channel segments every thread merges nblk / 32 partial sums -- one round of loads instead of four to eight dependent ones at
// 128 / 256 channels (the launch sits between the reduction and the dx pass of EVERY layer: 6.1 us each before, 23 per detector step).
struct BnBwdFinalizeArgs {
    const float* partial;
    int nblk;
    long m;
    int c, cw;
    const float* gamma;
    const float* stats;
    int training;
    float *grad_gamma, *grad_beta, *coef;
};

__device__ __forceinline__ void bn_bwd_finalize_segment(const BnBwdFinalizeArgs& f, int group, int seg, double* sh_a, double* sh_b) {
    const int nblk = f.nblk, c = f.c, cw = f.cw;
    const float* __restrict__ partial = f.partial + (size_t)group * nblk * 2 * c;
    const float* __restrict__ stats = f.stats + (size_t)group * 4 * c;
    const float* __restrict__ gamma = f.gamma;
    float* __restrict__ coef = f.coef + (size_t)group * 3 * c;
    float* __restrict__ grad_gamma = f.grad_gamma + (size_t)group * c;
    float* __restrict__ grad_beta = f.grad_beta + (size_t)group * c;
    const int tid = threadIdx.x;
    const int chunks = 1024 / cw > 0 ? 1024 / cw : 1;
    const int lc = tid % cw, chunk = tid / cw;
    const int ch = seg * cw + lc;
    double a = 0.0, b = 0.0;
    if (chunk < chunks) {
        const int per = (nblk + chunks - 1) / chunks;
        const int lo = chunk * per, hi = lo + per < nblk ? lo + per : nblk;
        int q = lo;
        for (; q + 8 <= hi; q += 8) {  // 16 independent loads in flight, summed in block order
            float va[8], vb[8];
#pragma unroll
            for (int j = 0; j < 8; j++) { va[j] = partial[(size_t)(q + j) * 2 * c + ch]; vb[j] = partial[(size_t)(q + j) * 2 * c + c + ch]; }
#pragma unroll
            for (int j = 0; j < 8; j++) { a += (double)va[j]; b += (double)vb[j]; }
        }
        for (; q < hi; q++) { a += (double)partial[(size_t)q * 2 * c + ch]; b += (double)partial[(size_t)q * 2 * c + c + ch]; }
    }
    sh_a[tid] = a; sh_b[tid] = b;
    __syncthreads();
    // the chunk sums per channel in chunk order; 32 chunks (32-channel segments) as a fixed two-level tree: 4 runs of 8, then the 4 run sums
    if (chunks == 32) {
        double ra = 0.0, rb = 0.0;
        if (tid < 4 * cw) {
            const int run = tid / cw;
#pragma unroll
            for (int q = 0; q < 8; q++) { ra += sh_a[(run * 8 + q) * cw + lc]; rb += sh_b[(run * 8 + q) * cw + lc]; }
        }
        __syncthreads();
        if (tid < 4 * cw) { sh_a[tid] = ra; sh_b[tid] = rb; }
        __syncthreads();
    }
    if (tid < cw) {
        a = 0.0; b = 0.0;
        const int left = chunks == 32 ? 4 : chunks;
        for (int q = 0; q < left; q++) { a += sh_a[q * cw + tid]; b += sh_b[q * cw + tid]; }
        grad_beta[ch] = (float)a;
        grad_gamma[ch] = (float)b;
        coef[ch] = gamma[ch] * stats[3 * c + ch];
        coef[c + ch] = f.training ? (float)(a / (double)f.m) : 0.f;
        coef[2 * c + ch] = f.training ? (float)(b / (double)f.m) : 0.f;
    }
}

}  // namespace liso_chain

#endif  // LISO_CHAIN_BODIES_H
