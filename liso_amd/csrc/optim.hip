// AdamW over one flat fp32 parameter buffer on gfx950.  C ABI + reference lines: include/liso_optim.h.
//
// HBM-bound: 16 B read (p, g, m, v) + 12 B written (p, m, v) per element, nothing else.  Every thread moves one float4 of
// each stream per iteration (a wave reads 1 KiB contiguous per stream); the grid is sized to a few waves per SIMD and
// strides over the buffer.  The per-element operation order follows torch's multi-tensor AdamW (see the header), so the
// trajectories agree with torch.optim.AdamW to rounding.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/liso_conv.h"
#include "../../include/liso_iou3d.h"
#include "../../include/liso_optim.h"
#include "adamw_body.h"
#include "pack_chunk.h"

namespace {

using liso_adamw::adamw_one;  // (adamw_body.h: one copy for every update kernel)
using liso_adamw::AdamwScalars;

__global__ __launch_bounds__(256) void adamw_flat_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                         float* __restrict__ v, size_t n4, size_t n, AdamwScalars s) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        float4 pp = reinterpret_cast<float4*>(p)[i];
        const float4 gg = reinterpret_cast<const float4*>(g)[i];
        float4 mm = reinterpret_cast<float4*>(m)[i];
        float4 vv = reinterpret_cast<float4*>(v)[i];
        adamw_one(pp.x, gg.x, mm.x, vv.x, s);
        adamw_one(pp.y, gg.y, mm.y, vv.y, s);
        adamw_one(pp.z, gg.z, mm.z, vv.z, s);
        adamw_one(pp.w, gg.w, mm.w, vv.w, s);
        reinterpret_cast<float4*>(p)[i] = pp;
        reinterpret_cast<float4*>(m)[i] = mm;
        reinterpret_cast<float4*>(v)[i] = vv;
    }
    if (blockIdx.x == 0) {  // tail (n % 4 elements)
        const size_t i = 4 * n4 + threadIdx.x;
        if (i < n) adamw_one(p[i], g[i], m[i], v[i], s);
    }
}

// ---- AdamW that also writes the convolutions' packed filter panels (include/liso_optim.h: liso_adamw_step_packed_f32) ------------------
// The flat buffers are cut into work items, one 256-thread block each, in address order: tiles of the listed filter tensors and plain
// float4 ranges of everything else.  A tile is R rows (the tensor's leading dimension) x C columns (its second) x all taps: per row one
// contiguous run of C * taps floats in the four flat buffers.  The block updates the tile exactly as adamw_flat_kernel updates its
// elements (adamw_one), keeps the new parameters in LDS and writes from there the 16-byte chunks of up to two panels (pack_chunk.h: the
// chunk of the pack launches) and, optionally, the fp32 values a second time into a derived buffer ("mirror").  HBM traffic: the 28 B
// per element of the plain update + 2-8 B of panels.  LDS: <= 16.3 KiB per block, so residency is bounded by the 8 blocks of 256
// threads a CU holds, as for the plain update.
constexpr int kTileFloats = 2304;        // target tile: 8 rows x 32 columns x 9 taps
constexpr int kTileLds = 4096 + 64;      // capacity (floats): tiles that must span a whole tensor dimension may be larger than the target
constexpr int kPlainChunk4 = 1024;       // float4 per block of a plain range
constexpr unsigned kTableMagic = 0x4c50414du;

struct PackDestDev {
    unsigned short* dst;
    int fmt, planes, swap_ab, Kp, Np, k_off, n_off, pad;
};
struct PackItemDev {
    unsigned long long offset, numel;  // in the flat buffers (elements)
    int d0, d1, taps, vec, n_dest, pad;
    float* mirror;
    unsigned long long mirror_stride;
    PackDestDev dest[2];
};
struct PackWork {
    int item;  // >= 0: a tile of that item; -1: float4 range [start, start + R) in float4 units; -2: scalar range [start, start + R)
    int R, c0, C;
    unsigned long long start;  // tile: first row
};
struct PackTableHeader {
    unsigned magic;
    int n_items, n_work, pad;
    unsigned long long n, items_off, work_off, bytes;
};

__device__ __forceinline__ void emit_panel(const PackDestDev& D, const PackWork& w, int r0, int taps, int P, const float* __restrict__ tile,
                                           int tid) {
    const bool sw = D.swap_ab != 0;  // k runs along the rows (leading dimension) of the tensor, n along its columns
    const int kck = liso_pack::pack_chunk_k(D.fmt);
    const int klo = sw ? r0 : w.c0, kn = sw ? w.R : w.C;
    const int nlo = sw ? w.c0 : r0, nn = sw ? w.C : w.R;
    const int kc_lo = (klo + D.k_off) / kck, nkc = (klo + kn + D.k_off + kck - 1) / kck - kc_lo;
    const int total = D.planes * taps * nkc * nn;
    for (int idx = tid; idx < total; idx += 256) {
        const int nl = idx % nn;
        int t = idx / nn;
        const int kc = kc_lo + t % nkc;
        t /= nkc;
        const int tap = t % taps, plane = t / taps;
        liso_pack::pack_chunk_at(
            [&](int kp, int, int tp) {
                const int kl = kp - D.k_off - klo;
                if (kl < 0 || kl >= kn) return 0.0f;
                return sw ? tile[kl * P + nl * taps + tp] : tile[nl * P + kl * taps + tp];
            },
            D.fmt, plane, tap, kc, nlo + nl + D.n_off, taps, D.Kp, D.Np, D.dst);
    }
}

__global__ __launch_bounds__(256) void adamw_pack_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                         float* __restrict__ v, size_t n, AdamwScalars s,
                                                         const unsigned char* __restrict__ table) {
    __shared__ float tile[kTileLds];
    const PackTableHeader& h = *reinterpret_cast<const PackTableHeader*>(table);
    if (h.magic != kTableMagic || h.n != n || (int)blockIdx.x >= h.n_work) return;  // (not the table this launch was sized for)
    const PackWork w = reinterpret_cast<const PackWork*>(table + h.work_off)[blockIdx.x];
    const int tid = threadIdx.x;
    if (w.item == -1) {
        for (size_t i = w.start + tid; i < w.start + w.R; i += 256) {
            float4 pp = reinterpret_cast<float4*>(p)[i];
            const float4 gg = reinterpret_cast<const float4*>(g)[i];
            float4 mm = reinterpret_cast<float4*>(m)[i];
            float4 vv = reinterpret_cast<float4*>(v)[i];
            adamw_one(pp.x, gg.x, mm.x, vv.x, s);
            adamw_one(pp.y, gg.y, mm.y, vv.y, s);
            adamw_one(pp.z, gg.z, mm.z, vv.z, s);
            adamw_one(pp.w, gg.w, mm.w, vv.w, s);
            reinterpret_cast<float4*>(p)[i] = pp;
            reinterpret_cast<float4*>(m)[i] = mm;
            reinterpret_cast<float4*>(v)[i] = vv;
        }
        return;
    }
    if (w.item == -2) {
        const size_t i = w.start + tid;
        if (tid < w.R && i < n) adamw_one(p[i], g[i], m[i], v[i], s);
        return;
    }
    const PackItemDev& it = reinterpret_cast<const PackItemDev*>(table + h.items_off)[w.item];
    const int taps = it.taps, r0 = (int)w.start;
    const int run = w.C * taps, P = run | 1;  // odd row pitch in LDS: a chunk along the rows reads 8 different banks
    const size_t row_len = (size_t)it.d1 * taps;
    const size_t base = it.offset + (size_t)r0 * row_len + (size_t)w.c0 * taps;
    float* __restrict__ mir = it.mirror ? it.mirror + (size_t)r0 * it.mirror_stride + (size_t)w.c0 * taps : nullptr;
    if (it.vec) {  // rows, runs and the mirror's rows are multiples of 16 bytes
        const int run4 = run >> 2, total4 = w.R * run4;
        for (int i = tid; i < total4; i += 256) {
            const int r = i / run4, j = (i - r * run4) * 4;
            const size_t e = base + r * row_len + j;
            float4 pp = *reinterpret_cast<float4*>(p + e);
            const float4 gg = *reinterpret_cast<const float4*>(g + e);
            float4 mm = *reinterpret_cast<float4*>(m + e);
            float4 vv = *reinterpret_cast<float4*>(v + e);
            adamw_one(pp.x, gg.x, mm.x, vv.x, s);
            adamw_one(pp.y, gg.y, mm.y, vv.y, s);
            adamw_one(pp.z, gg.z, mm.z, vv.z, s);
            adamw_one(pp.w, gg.w, mm.w, vv.w, s);
            *reinterpret_cast<float4*>(p + e) = pp;
            *reinterpret_cast<float4*>(m + e) = mm;
            *reinterpret_cast<float4*>(v + e) = vv;
            float* t = tile + r * P + j;
            t[0] = pp.x, t[1] = pp.y, t[2] = pp.z, t[3] = pp.w;
            if (mir) *reinterpret_cast<float4*>(mir + (size_t)r * it.mirror_stride + j) = pp;
        }
    } else {
        const int total = w.R * run;
        for (int i = tid; i < total; i += 256) {
            const int r = i / run, j = i - r * run;
            const size_t e = base + r * row_len + j;
            float pp = p[e], mm = m[e], vv = v[e];
            adamw_one(pp, g[e], mm, vv, s);
            p[e] = pp, m[e] = mm, v[e] = vv;
            tile[r * P + j] = pp;
            if (mir) mir[(size_t)r * it.mirror_stride + j] = pp;
        }
    }
    if (r0 + w.R == it.d0 && w.c0 + w.C == it.d1) {  // the tensor's last tile: the 1-3 elements up to the next multiple of four
        const size_t e = it.offset + it.numel + tid;
        if (tid < (int)((4 - (it.numel & 3)) & 3) && e < n) adamw_one(p[e], g[e], m[e], v[e], s);
    }
    if (it.n_dest == 0) return;
    __syncthreads();
    for (int d = 0; d < it.n_dest; d++) emit_panel(it.dest[d], w, r0, taps, P, tile, tid);
}

// ---- loss scaling: the non-finite check, AdamW gated by it, the scale update (include/liso_optim.h) ----------------------------------
__device__ __forceinline__ bool nonfinite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }

__global__ __launch_bounds__(256) void grad_nonfinite_kernel(const float* __restrict__ g, size_t n4, size_t n,
                                                             liso_loss_scale_state* __restrict__ st) {
    bool bad = false;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        const float4 v = reinterpret_cast<const float4*>(g)[i];
        bad = bad || nonfinite(v.x) || nonfinite(v.y) || nonfinite(v.z) || nonfinite(v.w);
    }
    if (blockIdx.x == 0) {
        const size_t i = 4 * n4 + threadIdx.x;
        if (i < n) bad = bad || nonfinite(g[i]);
    }
    // one store per wave that saw a non-finite element (every writer stores the same 1: no atomic needed)
    if (__any(bad) && (threadIdx.x & 63) == 0) __hip_atomic_store(&st->found_inf, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(256) void adamw_amp_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                        float* __restrict__ v, size_t n4, size_t n, AdamwScalars s, double lr, double beta1,
                                                        double beta2, double grad_scale, const liso_loss_scale_state* __restrict__ st) {
    if (st->found_inf) return;  // skipped step: nothing is written
    __shared__ float sh[3];
    if (threadIdx.x == 0) {  // the step-dependent scalars, in double as the host computes them for liso_adamw_step_scaled_f32
        const double step = (double)(st->step + 1);
        sh[0] = (float)sqrt(1.0 - pow(beta2, step));
        sh[1] = (float)(lr / (1.0 - pow(beta1, step)));
        sh[2] = (float)(grad_scale / (double)st->scale);
    }
    __syncthreads();
    s.bc2_sqrt = sh[0];
    s.step_size = sh[1];
    s.gscale = sh[2];
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        float4 pp = reinterpret_cast<float4*>(p)[i];
        const float4 gg = reinterpret_cast<const float4*>(g)[i];
        float4 mm = reinterpret_cast<float4*>(m)[i];
        float4 vv = reinterpret_cast<float4*>(v)[i];
        adamw_one(pp.x, gg.x, mm.x, vv.x, s);
        adamw_one(pp.y, gg.y, mm.y, vv.y, s);
        adamw_one(pp.z, gg.z, mm.z, vv.z, s);
        adamw_one(pp.w, gg.w, mm.w, vv.w, s);
        reinterpret_cast<float4*>(p)[i] = pp;
        reinterpret_cast<float4*>(m)[i] = mm;
        reinterpret_cast<float4*>(v)[i] = vv;
    }
    if (blockIdx.x == 0) {
        const size_t i = 4 * n4 + threadIdx.x;
        if (i < n) adamw_one(p[i], g[i], m[i], v[i], s);
    }
}

__global__ void loss_scale_update_kernel(liso_loss_scale_state* st, float growth, float backoff, int interval) {
    liso_loss_scale_state s = *st;
    if (s.found_inf) {
        s.scale *= backoff;
        s.growth_tracker = 0;
        s.skipped += 1;
    } else {
        s.step += 1;
        const int successful = s.growth_tracker + 1;
        const float grown = s.scale * growth;
        if (successful >= interval && !nonfinite(grown)) {
            s.scale = grown;
            s.growth_tracker = 0;
        } else {
            s.growth_tracker = successful >= interval ? 0 : successful;
        }
    }
    s.found_inf = 0;
    *st = s;
}

// ---- RMSprop over one flat buffer (SLIM's optimizer: liso/slim/experiment.py:200-219, torch.optim.RMSprop defaults) ---------------------
// torch's multi-tensor form, per element: sq = sq * alpha + (1 - alpha) * g * g;  p = p - lr * g / (sqrt(sq) + eps)
// HBM-bound: 12 B read (p, g, sq) + 8 B written (p, sq) per element, one launch instead of five foreach launches per 1-3 chunks.
__global__ __launch_bounds__(256) void rmsprop_flat_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ sq,
                                                           size_t n4, size_t n, float lr, float alpha, float w, float eps, float gscale) {
    auto one = [&](float& pp, float gg, float& ss) {
        gg = gg * gscale;
        ss = fmaf(w, gg * gg, ss * alpha);
        pp = fmaf(-lr, gg / (sqrtf(ss) + eps), pp);
    };
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        float4 pp = reinterpret_cast<float4*>(p)[i];
        const float4 gg = reinterpret_cast<const float4*>(g)[i];
        float4 ss = reinterpret_cast<float4*>(sq)[i];
        one(pp.x, gg.x, ss.x);
        one(pp.y, gg.y, ss.y);
        one(pp.z, gg.z, ss.z);
        one(pp.w, gg.w, ss.w);
        reinterpret_cast<float4*>(p)[i] = pp;
        reinterpret_cast<float4*>(sq)[i] = ss;
    }
    if (blockIdx.x == 0) {
        const size_t i = 4 * n4 + threadIdx.x;
        if (i < n) one(p[i], g[i], sq[i]);
    }
}

// ---- gradients that autograd produced outside the flat buffer: one launch moves all of them into their slices ----------------------
struct GatherTable {
    const float* src[LISO_GATHER_MAX];
    float* dst[LISO_GATHER_MAX];
    unsigned n[LISO_GATHER_MAX];
};

__global__ __launch_bounds__(256) void gather_f32_kernel(GatherTable t) {
    const float* __restrict__ s = t.src[blockIdx.y];
    float* __restrict__ d = t.dst[blockIdx.y];
    const unsigned n = t.n[blockIdx.y];
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) d[i] = s[i];
}

}  // namespace

// ---- the table of liso_adamw_step_packed_f32: checked and laid out on the host ----------------------------------------------------------
namespace {

inline int round_up_i(int x, int m) { return (x + m - 1) / m * m; }

struct Span {
    uintptr_t lo, hi;  // bytes [lo, hi)
    bool meets(const Span& o) const { return lo < o.hi && o.lo < hi; }
};
struct DestPlan {
    const void* dst;
    int mode, taps, K, N, kc_lo, kc_hi, n_lo, n_hi;
    Span span;
};

// -> LISO_OK with the device image's items and work list, or LISO_EINVAL
int plan_table(const liso_adamw_pack_item* items, int n_items, size_t n, std::vector<PackItemDev>* out_items, std::vector<PackWork>* out_work) {
    if (n_items < 0 || (n_items > 0 && !items) || n == 0) return LISO_EINVAL;
    std::vector<int> order(n_items);
    for (int i = 0; i < n_items; i++) order[i] = i;
    std::sort(order.begin(), order.end(), [&](int a, int b) { return items[a].offset < items[b].offset; });
    std::vector<DestPlan> dests;
    std::vector<Span> mirrors;
    size_t cursor = 0;  // first element no work item covers yet (a multiple of four)
    auto plain = [&](size_t a, size_t b) {  // [a, b): a a multiple of four, b one or n
        size_t a4 = a / 4;
        const size_t b4 = b / 4;
        for (; a4 < b4; a4 += kPlainChunk4) out_work->push_back(PackWork{-1, (int)std::min<size_t>(kPlainChunk4, b4 - a4), 0, 0, a4});
        if (b & 3) out_work->push_back(PackWork{-2, (int)(b & 3), 0, 0, b4 * 4});
    };
    for (int oi = 0; oi < n_items; oi++) {
        const liso_adamw_pack_item& it = items[order[oi]];
        if (it.d0 <= 0 || it.d1 <= 0 || it.kh <= 0 || it.kw <= 0 || it.n_dest < 0 || it.n_dest > 2) return LISO_EINVAL;
        const long taps = (long)it.kh * it.kw;
        const unsigned long long numel = (unsigned long long)it.d0 * it.d1 * taps;
        if ((it.offset & 3) || it.offset < cursor || it.offset > n || numel > n - it.offset) return LISO_EINVAL;  // (sorted: < cursor = overlap)
        if (taps > 64 || (long)it.d1 * taps > (1 << 24)) return LISO_EINVAL;
        const long row_len = (long)it.d1 * taps;
        PackItemDev d = {};
        d.offset = it.offset, d.numel = numel;
        d.d0 = it.d0, d.d1 = it.d1, d.taps = (int)taps, d.n_dest = it.n_dest;
        d.vec = row_len % 4 == 0;
        if (it.mirror) {
            if (((uintptr_t)it.mirror & 3) || it.mirror_row_stride < (size_t)row_len) return LISO_EINVAL;
            if (((uintptr_t)it.mirror & 15) || (it.mirror_row_stride & 3)) d.vec = 0;
            d.mirror = it.mirror, d.mirror_stride = it.mirror_row_stride;
            const Span sp{(uintptr_t)it.mirror, (uintptr_t)(it.mirror + (size_t)(it.d0 - 1) * it.mirror_row_stride + row_len)};
            for (const Span& o : mirrors)
                if (sp.meets(o)) return LISO_EINVAL;
            mirrors.push_back(sp);
        }
        bool whole_rows = false, whole_cols = false;  // a tile must span all of d0 / all of d1
        for (int k = 0; k < it.n_dest; k++) {
            const liso_adamw_pack_dest& q = it.dest[k];
            if (!q.dst || ((uintptr_t)q.dst & 15)) return LISO_EINVAL;
            if (q.mode != LISO_CONV_BF16 && q.mode != LISO_CONV_F32X3 && q.mode != LISO_CONV_F32) return LISO_EINVAL;
            const bool same = (it.transposed != 0) == (q.for_dgrad != 0);
            const int K = same ? it.d1 : it.d0, N = same ? it.d0 : it.d1;
            if (q.K <= 0 || q.N <= 0 || q.k_offset < 0 || q.n_offset < 0) return LISO_EINVAL;
            if ((long)q.k_offset + K > q.K || (long)q.n_offset + N > q.N) return LISO_EINVAL;
            const int fmt = liso_pack::pack_format(q.mode), kck = liso_pack::pack_chunk_k(fmt);
            PackDestDev& o = d.dest[k];
            o.dst = (unsigned short*)q.dst;
            o.fmt = fmt, o.planes = liso_pack::pack_planes(q.mode), o.swap_ab = same ? 0 : 1;
            o.Kp = round_up_i(q.K, 16), o.Np = round_up_i(q.N, 64), o.k_off = q.k_offset, o.n_off = q.n_offset;
            if (q.k_offset % kck) (o.swap_ab ? whole_rows : whole_cols) = true;  // tiles along k would share chunks otherwise
            DestPlan pl{q.dst, q.mode, (int)taps, q.K, q.N, q.k_offset / kck, (q.k_offset + K + kck - 1) / kck, q.n_offset, q.n_offset + N,
                        Span{(uintptr_t)q.dst, (uintptr_t)q.dst + liso_conv_packed_bytes(q.K, q.N, (int)taps, q.mode)}};
            for (const DestPlan& e : dests) {
                if (!pl.span.meets(e.span)) continue;
                if (e.dst != pl.dst || e.mode != pl.mode || e.taps != pl.taps || e.K != pl.K || e.N != pl.N) return LISO_EINVAL;
                if (pl.kc_lo < e.kc_hi && e.kc_lo < pl.kc_hi && pl.n_lo < e.n_hi && e.n_lo < pl.n_hi) return LISO_EINVAL;  // shared chunks
            }
            dests.push_back(pl);
        }
        for (const DestPlan& e : dests)
            for (const Span& o : mirrors)
                if (e.span.meets(o)) return LISO_EINVAL;
        // tile: R rows x C columns; several row (column) tiles start at multiples of 8, so that they never share a chunk
        int R, C;
        if (whole_rows && whole_cols) {
            R = it.d0, C = it.d1;
        } else if (whole_rows) {
            R = it.d0;
            const long fit = (kTileLds - R) / ((long)R * taps);
            C = fit >= it.d1 ? it.d1 : (int)(fit / 8 * 8);
        } else if (whole_cols || row_len * 8 <= kTileFloats) {
            C = it.d1;
            const long fit = row_len * 8 <= kTileFloats ? kTileFloats / row_len : kTileLds / (row_len | 1);
            R = fit >= it.d0 ? it.d0 : (int)(fit / 8 * 8);
            if (R > 64) R = 64;
        } else {
            R = std::min(8, it.d0);
            C = (int)std::max<long>(8, kTileFloats / (8 * taps) / 8 * 8);
        }
        if (R < 1 || C < 1 || (R < it.d0 && R % 8) || (C < it.d1 && C % 8)) return LISO_EINVAL;
        if ((long)R * (((long)C * taps) | 1) > kTileLds) return LISO_EINVAL;
        if (it.offset > cursor) plain(cursor, it.offset);
        const int item = (int)out_items->size();
        out_items->push_back(d);
        for (int r0 = 0; r0 < it.d0; r0 += R)
            for (int c0 = 0; c0 < it.d1; c0 += C)
                out_work->push_back(PackWork{item, std::min(R, it.d0 - r0), c0, std::min(C, it.d1 - c0), (unsigned long long)r0});
        cursor = std::min<size_t>(n, (size_t)((it.offset + numel + 3) / 4 * 4));
    }
    if (cursor < n) plain(cursor, n);
    return out_work->size() < (size_t)1 << 30 ? LISO_OK : LISO_EINVAL;
}

AdamwScalars adamw_scalars(double lr, double beta1, double beta2, double eps, double weight_decay, double grad_scale, long step) {
    AdamwScalars s;
    s.decay = (float)(1.0 - lr * weight_decay);
    s.w1 = (float)(1.0 - beta1);
    s.beta2 = (float)beta2;
    s.w2 = (float)(1.0 - beta2);
    s.bc2_sqrt = (float)sqrt(1.0 - pow(beta2, (double)step));
    s.eps = (float)eps;
    s.step_size = (float)(lr / (1.0 - pow(beta1, (double)step)));
    s.gscale = (float)grad_scale;
    return s;
}

}  // namespace

extern "C" int liso_adamw_pack_table_plan(const liso_adamw_pack_item* items, int n_items, size_t n, size_t* bytes, int* blocks) {
    std::vector<PackItemDev> di;
    std::vector<PackWork> dw;
    const int rc = plan_table(items, n_items, n, &di, &dw);
    if (rc != LISO_OK) return rc;
    if (bytes) *bytes = sizeof(PackTableHeader) + di.size() * sizeof(PackItemDev) + dw.size() * sizeof(PackWork);
    if (blocks) *blocks = (int)dw.size();
    return LISO_OK;
}

extern "C" int liso_adamw_pack_table_fill(const liso_adamw_pack_item* items, int n_items, size_t n, void* image, size_t bytes) {
    std::vector<PackItemDev> di;
    std::vector<PackWork> dw;
    const int rc = plan_table(items, n_items, n, &di, &dw);
    if (rc != LISO_OK) return rc;
    PackTableHeader h = {};
    h.magic = kTableMagic, h.n_items = (int)di.size(), h.n_work = (int)dw.size(), h.n = n;
    h.items_off = sizeof(PackTableHeader), h.work_off = h.items_off + di.size() * sizeof(PackItemDev);
    h.bytes = h.work_off + dw.size() * sizeof(PackWork);
    if (!image || bytes != h.bytes) return LISO_EINVAL;
    unsigned char* o = (unsigned char*)image;
    memcpy(o, &h, sizeof(h));
    if (!di.empty()) memcpy(o + h.items_off, di.data(), di.size() * sizeof(PackItemDev));
    memcpy(o + h.work_off, dw.data(), dw.size() * sizeof(PackWork));
    return LISO_OK;
}

extern "C" int liso_adamw_step_packed_f32(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n, double lr,
                                          double beta1, double beta2, double eps, double weight_decay, double grad_scale, long step,
                                          const void* table, int blocks, void* stream) {
    if (!param || !grad || !exp_avg || !exp_avg_sq || !table || step < 1 || n == 0 || blocks < 1) return LISO_EINVAL;
    if ((((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq | (uintptr_t)table) & 15) != 0) return LISO_EINVAL;
    const AdamwScalars s = adamw_scalars(lr, beta1, beta2, eps, weight_decay, grad_scale, step);
    hipLaunchKernelGGL(adamw_pack_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, param, grad, exp_avg, exp_avg_sq, n,
                       s, (const unsigned char*)table);
    return hipGetLastError() == hipSuccess ? LISO_OK : LISO_ELAUNCH;
}

extern "C" int liso_gather_f32(int count, const void* const* src, void* const* dst, const size_t* numel, void* stream) {
    if (count < 0 || (count > 0 && (!src || !dst || !numel))) return LISO_EINVAL;
    for (int base = 0; base < count; base += LISO_GATHER_MAX) {
        GatherTable t;
        const int m = count - base < LISO_GATHER_MAX ? count - base : LISO_GATHER_MAX;
        size_t longest = 0;
        for (int k = 0; k < m; k++) {
            if (!src[base + k] || !dst[base + k] || numel[base + k] > 0xffffffffull) return LISO_EINVAL;
            t.src[k] = (const float*)src[base + k];
            t.dst[k] = (float*)dst[base + k];
            t.n[k] = (unsigned)numel[base + k];
            longest = numel[base + k] > longest ? numel[base + k] : longest;
        }
        size_t bx = (longest + 1023) / 1024;  // (4 elements per thread and pass)
        bx = bx < 1 ? 1 : (bx > 64 ? 64 : bx);
        hipLaunchKernelGGL(gather_f32_kernel, dim3((unsigned)bx, (unsigned)m), dim3(256), 0, (hipStream_t)stream, t);
    }
    return hipGetLastError() == hipSuccess ? LISO_OK : LISO_ELAUNCH;
}

extern "C" int liso_adamw_step_scaled_f32(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n, double lr,
                                          double beta1, double beta2, double eps, double weight_decay, double grad_scale, long step,
                                          void* stream);

extern "C" int liso_adamw_step_f32(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n, double lr,
                                   double beta1, double beta2, double eps, double weight_decay, long step, void* stream) {
    return liso_adamw_step_scaled_f32(param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, 1.0, step, stream);
}

extern "C" int liso_adamw_step_scaled_f32(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n, double lr,
                                          double beta1, double beta2, double eps, double weight_decay, double grad_scale, long step,
                                          void* stream) {
    if (n == 0) return LISO_OK;
    if (!param || !grad || !exp_avg || !exp_avg_sq || step < 1) return LISO_EINVAL;
    if ((((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15) != 0) return LISO_EINVAL;
    const AdamwScalars s = adamw_scalars(lr, beta1, beta2, eps, weight_decay, grad_scale, step);
    const size_t n4 = n / 4;
    size_t blocks = (n4 + 255) / 256;
    if (blocks > 2048) blocks = 2048;  // 256 CUs x 8 blocks: the rest is the grid-stride loop
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(adamw_flat_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, param, grad, exp_avg,
                       exp_avg_sq, n4, n, s);
    return hipGetLastError() == hipSuccess ? LISO_OK : LISO_ELAUNCH;
}

extern "C" int liso_grad_nonfinite_f32(const float* grad, size_t n, liso_loss_scale_state* state, void* stream) {
    if (!state || ((uintptr_t)state & 15)) return LISO_EINVAL;
    if (n == 0) return LISO_OK;
    if (!grad || (((uintptr_t)grad | (uintptr_t)state) & 15) != 0) return LISO_EINVAL;
    const size_t n4 = n / 4;
    size_t blocks = (n4 + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(grad_nonfinite_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, grad, n4, n, state);
    return hipGetLastError() == hipSuccess ? LISO_OK : LISO_ELAUNCH;
}

extern "C" int liso_adamw_step_amp_f32(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n, double lr,
                                       double beta1, double beta2, double eps, double weight_decay, double grad_scale,
                                       const liso_loss_scale_state* state, void* stream) {
    if (n == 0) return LISO_OK;
    if (!param || !grad || !exp_avg || !exp_avg_sq || !state) return LISO_EINVAL;
    if ((((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq | (uintptr_t)state) & 15) != 0) return LISO_EINVAL;
    AdamwScalars s;
    s.decay = (float)(1.0 - lr * weight_decay);
    s.w1 = (float)(1.0 - beta1);
    s.beta2 = (float)beta2;
    s.w2 = (float)(1.0 - beta2);
    s.eps = (float)eps;
    s.bc2_sqrt = s.step_size = s.gscale = 0.0f;  // (from the device state, inside the kernel)
    const size_t n4 = n / 4;
    size_t blocks = (n4 + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(adamw_amp_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, param, grad, exp_avg, exp_avg_sq, n4,
                       n, s, lr, beta1, beta2, grad_scale, state);
    return hipGetLastError() == hipSuccess ? LISO_OK : LISO_ELAUNCH;
}

extern "C" int liso_loss_scale_update(liso_loss_scale_state* state, double growth_factor, double backoff_factor, int growth_interval,
                                      void* stream) {
    if (!state || ((uintptr_t)state & 15) || growth_interval < 1 || !(growth_factor >= 1.0) || !(backoff_factor > 0.0 && backoff_factor <= 1.0))
        return LISO_EINVAL;
    hipLaunchKernelGGL(loss_scale_update_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, state, (float)growth_factor,
                       (float)backoff_factor, growth_interval);
    return hipGetLastError() == hipSuccess ? LISO_OK : LISO_ELAUNCH;
}

extern "C" int liso_rmsprop_step_f32(float* param, const float* grad, float* square_avg, size_t n, double lr, double alpha, double eps,
                                     double grad_scale, void* stream) {
    if (n == 0) return LISO_OK;
    if (!param || !grad || !square_avg) return LISO_EINVAL;
    if ((((uintptr_t)param | (uintptr_t)grad | (uintptr_t)square_avg) & 15) != 0) return LISO_EINVAL;
    const size_t n4 = n / 4;
    size_t blocks = (n4 + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(rmsprop_flat_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, param, grad, square_avg, n4, n,
                       (float)lr, (float)alpha, (float)(1.0 - alpha), (float)eps, (float)grad_scale);
    return hipGetLastError() == hipSuccess ? LISO_OK : LISO_ELAUNCH;
}
