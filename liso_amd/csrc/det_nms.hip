// Detector inference post-processing for gfx950 (MI355X): dense head maps -> post-NMS boxes, C ABI in
// include/liso_det_nms.h.  Reference semantics: run_val (liso/eval/eval_ours.py:361-386) and the tracker
// (liso/tracker/tracking.py:710-740) around rotate_nms_pcdet (liso/utils/nms_iou.py:257-282).
//
//   (a) order: a segmented LSD radix sort of order-preserving uint32 keys with the slot index as payload, 8-bit digits,
//       4 passes of (tile histogram, per-sample scan, stable tile scatter).  The scatter ranks equal digits in item order
//       (ballot match per wave + per-wave digit counts in LDS), so every pass is stable and ties keep slot order.
//       No sort library: the keys need 13 small launches per batch.
//   (b) select: one workgroup per sample walks the ordered candidates in chunks of 64.  Each candidate is tested against
//       the boxes kept so far (their geometry is parked in LDS, at most LISO_DET_NMS_MAX_POST), the survivors of a chunk
//       are resolved among themselves in rank order with a 64x64 ballot mask, as nms_greedy_kernel does on its diagonal,
//       and the walk ends once post_nms_max boxes are kept.  Greedy NMS decides a box from the boxes ranked above it
//       only, so the first P survivors are exact without the N x N mask of liso_iou3d_nms_f32.
//       The pair predicate is rbev_geom.h's box_overlap_dev / iou_from_overlap with "> thresh", higher-ranked box as A.
//   (c) gather: the kept rows of up to 8 per-slot fields, padding rows elsewhere, one launch.
//
// Built with -ffp-contract=off (the geometry must round exactly as in iou3d_nms.hip).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "dev_common.h"
#include "rbev_geom.h"
#include "../../include/liso_det_nms.h"

namespace {

using liso_dev::check_launch;

using namespace liso_rbev;

// ---------------------------------------------------------------- (a) order
constexpr int kSortThreads = 256;
constexpr int kSortItems = 16;                          // items per thread and tile
constexpr int kSortTile = kSortThreads * kSortItems;    // 4096 keys per workgroup
constexpr int kRadix = 256;
constexpr uint32_t kEndKey = LISO_DET_NMS_END_KEY;
constexpr int kMaxBatch = 65535;                        // grid.y / grid.x limit of the per-sample launches

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
inline int sort_tiles(int n) { return (n + kSortTile - 1) / kSortTile; }

// ascending key == descending score; NaN first (key 0), -0.0 == +0.0, -inf last of the participating keys (0xFF800000)
__device__ __forceinline__ uint32_t desc_key(float f) {
    if (f != f) return 0u;
    uint32_t u = __float_as_uint(f);
    if (u == 0x80000000u) u = 0u;
    const uint32_t ord = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ~ord;
}

__global__ __launch_bounds__(kSortThreads) void order_keys_kernel(int n, const float* __restrict__ scores,
                                                                  const float* __restrict__ gate,
                                                                  const uint8_t* __restrict__ valid, float thr,
                                                                  uint32_t* __restrict__ keys, int32_t* __restrict__ idx) {
    const int i = blockIdx.x * kSortThreads + threadIdx.x;
    if (i >= n) return;
    const size_t o = (size_t)blockIdx.y * n + i;
    const float s = scores[o];
    const float g = gate ? gate[o] : s;
    const bool part = (!valid || valid[o] != 0) && !(g < thr);
    keys[o] = part ? desc_key(s) : kEndKey;
    idx[o] = i;
}

// hist[b][digit][tile] = number of keys of tile `tile` of sample b whose digit at `shift` is `digit`
__global__ __launch_bounds__(kSortThreads) void radix_hist_kernel(int n, int tiles, int shift, const uint32_t* __restrict__ keys,
                                                                  uint32_t* __restrict__ hist) {
    __shared__ uint32_t h[kRadix];
    const int tid = threadIdx.x, tile = blockIdx.x, b = blockIdx.y;
    h[tid] = 0;
    __syncthreads();
    const uint32_t* k = keys + (size_t)b * n;
#pragma unroll 4
    for (int it = 0; it < kSortItems; it++) {
        const int i = tile * kSortTile + it * kSortThreads + tid;
        if (i < n) atomicAdd(&h[(k[i] >> shift) & 255u], 1u);
    }
    __syncthreads();
    hist[((size_t)b * kRadix + tid) * tiles + tile] = h[tid];
}

// in place: hist[b][d][t] <- position (within sample b) of the first key of tile t with digit d (digit-major exclusive scan)
__global__ __launch_bounds__(kSortThreads) void radix_scan_kernel(int tiles, uint32_t* __restrict__ hist) {
    __shared__ uint32_t tot[kRadix];
    const int d = threadIdx.x;
    uint32_t* row = hist + ((size_t)blockIdx.x * kRadix + d) * tiles;
    uint32_t s = 0;
    for (int t = 0; t < tiles; t++) s += row[t];
    tot[d] = s;
    __syncthreads();
    for (int off = 1; off < kRadix; off <<= 1) {  // Hillis-Steele inclusive scan of the 256 digit totals
        const uint32_t v = d >= off ? tot[d - off] : 0u;
        __syncthreads();
        tot[d] += v;
        __syncthreads();
    }
    uint32_t run = tot[d] - s;  // exclusive
    for (int t = 0; t < tiles; t++) {
        const uint32_t c = row[t];
        row[t] = run;
        run += c;
    }
}

// stable scatter of one tile: items in order (chunk, wave, lane); equal digits ranked by a ballot match inside a wave and
// by the per-wave digit counts across waves
__global__ __launch_bounds__(kSortThreads) void radix_scatter_kernel(int n, int tiles, int shift, const uint32_t* __restrict__ kin,
                                                                     const int32_t* __restrict__ iin, const uint32_t* __restrict__ hist,
                                                                     uint32_t* __restrict__ kout, int32_t* __restrict__ iout) {
    constexpr int kWaves = kSortThreads / 64;
    __shared__ uint32_t base[kRadix];
    __shared__ uint32_t wcnt[kWaves][kRadix];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, tile = blockIdx.x, b = blockIdx.y;
    const size_t so = (size_t)b * n;
    base[tid] = hist[((size_t)b * kRadix + tid) * tiles + tile];
#pragma unroll
    for (int q = 0; q < kWaves; q++) wcnt[q][tid] = 0;
    __syncthreads();
    const unsigned long long lt = (1ULL << lane) - 1ULL;
    for (int it = 0; it < kSortItems; it++) {
        const int i = tile * kSortTile + it * kSortThreads + tid;
        if (tile * kSortTile + it * kSortThreads >= n) break;  // block-uniform
        const bool in = i < n;
        const uint32_t key = in ? kin[so + i] : 0u;
        const int32_t val = in ? iin[so + i] : 0;
        const uint32_t d = (key >> shift) & 255u;
        unsigned long long m = __ballot(in);
#pragma unroll
        for (int bit = 0; bit < 8; bit++) {
            const bool set = (d >> bit) & 1u;
            const unsigned long long bb = __ballot(set);
            m &= set ? bb : ~bb;
        }
        const uint32_t rank = (uint32_t)__popcll(m & lt);
        if (in && rank == 0) wcnt[w][d] = (uint32_t)__popcll(m);
        __syncthreads();
        if (in) {
            uint32_t pos = base[d] + rank;
            for (int q = 0; q < w; q++) pos += wcnt[q][d];
            kout[so + pos] = key;
            iout[so + pos] = val;
        }
        __syncthreads();
        uint32_t add = 0;
#pragma unroll
        for (int q = 0; q < kWaves; q++) {
            add += wcnt[q][tid];
            wcnt[q][tid] = 0;
        }
        base[tid] += add;
        __syncthreads();
    }
}

// ---------------------------------------------------------------- (b) select
constexpr int kSelThreads = kPolyThreads;  // 4 waves; PolyLds has one column per thread
constexpr int kChunk = 64;                 // candidates per step == wavefront width == bits of a ballot word
constexpr int kMaxPost = LISO_DET_NMS_MAX_POST;

struct SelectLds {
    float kept[G_N][kMaxPost];   // geometry of the kept boxes, keep order
    float kept_rr[kMaxPost];     // their reject radius (NaN: never rejected early)
    float cand[G_N][kChunk];     // geometry of the current chunk
    PolyLds poly;
    unsigned long long sup[kChunk];  // sup[i] bit j: alive chunk candidate i suppresses alive candidate j > i
    int slot[kChunk];            // slot index of each chunk candidate, -1 past the end
    int dead[kChunk];
    int kept_n;
};

// Radius of the cheap reject: the conservative circumscribed radius Geo::rad (rbev_geom.h: half diagonal x 1.001 + the
// in-box margin + slack for far-away coordinates), NaN when the box's centre or radius is not finite so that NaN / Inf
// geometry always reaches the exact predicate.
__device__ __forceinline__ float reject_radius(const Geo& g) {
    return (isfinite(g.cx) && isfinite(g.cy) && isfinite(g.rad)) ? g.rad : __builtin_nanf("");
}

// True only where box_overlap_dev(A, B) takes its own disjoint-circle early-out (the same float expression on the same
// values) and returns 0: IoU is then 0 and "0 > thresh" is false for every thresh >= 0.  Callers disable it for thresh < 0.
__device__ __forceinline__ bool circles_disjoint(float acx, float acy, float arr, float bcx, float bcy, float brr) {
    const float ddx = acx - bcx, ddy = acy - bcy;
    const float rr = arr + brr;
    return ddx * ddx + ddy * ddy > rr * rr;
}

__device__ __forceinline__ bool suppresses(const Geo& A, const Geo& B, float thresh, PolyLds* P, int tid) {
    const float ov = box_overlap_dev(A, B, P, tid);
    return iou_from_overlap(A, B, ov) > thresh;
}

__global__ __launch_bounds__(kSelThreads) void det_nms_select_kernel(int n, const float* __restrict__ boxes,
                                                                     const uint32_t* __restrict__ keys,
                                                                     const int32_t* __restrict__ order, float thresh, int m_cap,
                                                                     int post, long long* __restrict__ keep,
                                                                     int32_t* __restrict__ counts) {
    __shared__ SelectLds L;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const size_t so = (size_t)b * n;
    long long* kb = keep + (size_t)b * post;
    const bool reject = !(thresh < 0.f);  // thresh < 0: a pair with IoU 0 is suppressed too
    int K = 0;
    for (int base = 0; base < m_cap; base += kChunk) {
        if (tid < kChunk) {
            const int r = base + tid;
            int s = -1;
            if (r < m_cap && keys[so + r] != kEndKey) s = order[so + r];
            L.slot[tid] = s;
            L.dead[tid] = s < 0;
            if (s >= 0) store_geo(L.cand, tid, make_geo(boxes + (so + (size_t)s) * 7));
        }
        __syncthreads();
        if (L.slot[0] < 0) break;  // the participating slots are a prefix of the order

        // 1. every candidate against the kept boxes: candidate = lane, kept boxes strided over the 4 waves
        if (K > 0 && L.slot[lane] >= 0) {
            const Geo B = load_geo(L.cand, lane);
            const float brr = reject_radius(B);
            for (int k = w; k < K; k += kSelThreads / 64) {
                if (*(volatile int*)&L.dead[lane]) break;  // another wave already suppressed it
                if (reject && circles_disjoint(L.kept[G_CX][k], L.kept[G_CY][k], L.kept_rr[k], B.cx, B.cy, brr)) continue;
                const Geo A = load_geo(L.kept, k);
                if (suppresses(A, B, thresh, &L.poly, tid)) {
                    L.dead[lane] = 1;
                    break;
                }
            }
        }
        __syncthreads();

        // 2. the survivors among themselves: row i (higher rank, A) against column j > i (B), one ballot word per row
        const unsigned long long alive = __ballot(L.slot[lane] >= 0 && !L.dead[lane]);
        const bool pairs = __popcll(alive) > 1;
        if (pairs) {
            const bool me = (alive >> lane) & 1ULL;
            Geo B;
            float brr = 0.f;
            if (me) {
                B = load_geo(L.cand, lane);
                brr = reject_radius(B);
            }
            const int last = 63 - __clzll(alive);
            for (int i = w; i < last; i += kSelThreads / 64) {
                if (!((alive >> i) & 1ULL)) continue;  // wave-uniform
                bool hit = false;
                if (me && lane > i) {
                    const float arr = reject_radius(load_geo(L.cand, i));
                    if (!(reject && circles_disjoint(L.cand[G_CX][i], L.cand[G_CY][i], arr, B.cx, B.cy, brr))) {
                        const Geo A = load_geo(L.cand, i);
                        hit = suppresses(A, B, thresh, &L.poly, tid);
                    }
                }
                const unsigned long long word = __ballot(hit);
                if (lane == 0) L.sup[i] = word;
            }
        }
        __syncthreads();

        // 3. wave 0: the greedy pass over the chunk in rank order on scalar registers, stopping at `post` kept boxes
        if (w == 0) {
            const bool row = pairs && ((alive >> lane) & 1ULL) && lane < 63 - __clzll(alive);  // rows step 2 wrote
            const unsigned long long diag = row ? L.sup[lane] : 0ULL;
            unsigned long long cur = ~alive, kept = 0ULL;
            int k = K;
#pragma unroll
            for (int t = 0; t < 64; t++) {
                const unsigned int lo = (unsigned int)__builtin_amdgcn_readlane((unsigned int)diag, t);
                const unsigned int hi = (unsigned int)__builtin_amdgcn_readlane((unsigned int)(diag >> 32), t);
                const unsigned long long d = ((unsigned long long)hi << 32) | lo;
                if (k < post && !((cur >> t) & 1ULL)) {
                    kept |= 1ULL << t;
                    cur |= d;
                    k++;
                }
            }
            if ((kept >> lane) & 1ULL) {
                const int p = K + __popcll(kept & ((1ULL << lane) - 1ULL));
                kb[p] = L.slot[lane];
                const Geo g = load_geo(L.cand, lane);
                store_geo(L.kept, p, g);
                L.kept_rr[p] = reject_radius(g);
            }
            if (lane == 0) L.kept_n = k;
        }
        __syncthreads();
        K = L.kept_n;
        if (K >= post) break;
        // (the next chunk's staging overwrites cand / slot / dead only after this barrier)
    }
    for (int p = K + tid; p < post; p += kSelThreads) kb[p] = -1;
    if (tid == 0) counts[b] = K;
}

// ---------------------------------------------------------------- (c) gather
struct GatherArgs {
    liso_det_gather_field f[LISO_DET_GATHER_MAX_FIELDS];
};

template <typename T>
__device__ __forceinline__ void gather_rows(const liso_det_gather_field& f, int b, int n, int post, int count,
                                            const long long* __restrict__ kb) {
    const T* src = (const T*)f.src;
    T* dst = (T*)f.dst;
    const T pad = (T)f.pad_bits;  // the low sizeof(T) bytes
    const int re = f.row_elems;
    const int total = post * re;
    for (int e = threadIdx.x; e < total; e += blockDim.x) {
        const int p = e / re, j = e - p * re;
        const long long s = p < count ? kb[p] : -1;
        dst[((size_t)b * post + p) * re + j] = (s >= 0 && s < n) ? src[((size_t)b * n + (size_t)s) * re + j] : pad;
    }
}

__global__ __launch_bounds__(256) void det_nms_gather_kernel(int n, int post, const long long* __restrict__ keep,
                                                             const int32_t* __restrict__ counts, GatherArgs a) {
    const int b = blockIdx.x;
    const liso_det_gather_field& f = a.f[blockIdx.y];
    const long long* kb = keep + (size_t)b * post;
    const int count = counts[b];
    switch (f.elem_bytes) {
        case 1: gather_rows<uint8_t>(f, b, n, post, count, kb); break;
        case 2: gather_rows<uint16_t>(f, b, n, post, count, kb); break;
        case 4: gather_rows<uint32_t>(f, b, n, post, count, kb); break;
        default: gather_rows<uint64_t>(f, b, n, post, count, kb); break;
    }
}

struct SortWs {
    uint32_t* keys;
    int32_t* idx;
    uint32_t* hist;
};

inline size_t ws_bytes(int batch, int n, SortWs* out, void* base) {
    const size_t bn = (size_t)batch * (size_t)n;
    const size_t o_keys = 0, o_idx = align256(bn * 4), o_hist = o_idx + align256(bn * 4);
    const size_t total = o_hist + align256((size_t)batch * kRadix * (size_t)sort_tiles(n) * 4);
    if (out) {
        char* p = (char*)base;
        out->keys = (uint32_t*)(p + o_keys);
        out->idx = (int32_t*)(p + o_idx);
        out->hist = (uint32_t*)(p + o_hist);
    }
    return total;
}

}  // namespace

extern "C" {

size_t liso_det_nms_workspace_bytes(int batch, int n) {
    if (batch <= 0 || batch > kMaxBatch || n <= 0 || n > LISO_DET_NMS_MAX_N) return 0;
    return ws_bytes(batch, n, nullptr, nullptr);
}

int liso_det_nms_order(int batch, int n, const float* scores, const float* gate, const uint8_t* valid, float logit_threshold,
                       uint32_t* sorted_keys, int32_t* sorted_idx, void* workspace, size_t workspace_bytes, void* stream) {
    if (batch <= 0 || batch > kMaxBatch || n < 0 || n > LISO_DET_NMS_MAX_N) return LISO_EINVAL;
    if (n == 0) return (scores || gate || valid || sorted_keys || sorted_idx) ? LISO_EINVAL : LISO_OK;
    if (!scores || !sorted_keys || !sorted_idx || !workspace) return LISO_EINVAL;
    if (workspace_bytes < liso_det_nms_workspace_bytes(batch, n)) return LISO_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    SortWs ws;
    ws_bytes(batch, n, &ws, workspace);
    const int tiles = sort_tiles(n);
    hipLaunchKernelGGL(order_keys_kernel, dim3((n + kSortThreads - 1) / kSortThreads, batch), dim3(kSortThreads), 0, st, n, scores,
                       gate, valid, logit_threshold, sorted_keys, sorted_idx);
    if (check_launch() != LISO_OK) return LISO_ELAUNCH;
    uint32_t* ka[2] = {sorted_keys, ws.keys};
    int32_t* ia[2] = {sorted_idx, ws.idx};
    for (int pass = 0; pass < 4; pass++) {  // even number of passes: the result lands in sorted_keys / sorted_idx
        const int src = pass & 1, dst = src ^ 1, shift = 8 * pass;
        hipLaunchKernelGGL(radix_hist_kernel, dim3(tiles, batch), dim3(kSortThreads), 0, st, n, tiles, shift, ka[src], ws.hist);
        hipLaunchKernelGGL(radix_scan_kernel, dim3(batch), dim3(kSortThreads), 0, st, tiles, ws.hist);
        hipLaunchKernelGGL(radix_scatter_kernel, dim3(tiles, batch), dim3(kSortThreads), 0, st, n, tiles, shift, ka[src], ia[src],
                           ws.hist, ka[dst], ia[dst]);
        if (check_launch() != LISO_OK) return LISO_ELAUNCH;
    }
    return LISO_OK;
}

int liso_det_nms_select(int batch, int n, const float* boxes, const uint32_t* sorted_keys, const int32_t* sorted_idx, float thresh,
                        int pre_nms_max, int post_nms_max, int64_t* keep, int32_t* counts, void* stream) {
    if (batch <= 0 || batch > kMaxBatch || n < 0 || n > LISO_DET_NMS_MAX_N) return LISO_EINVAL;
    if (post_nms_max < 1 || post_nms_max > LISO_DET_NMS_MAX_POST) return LISO_EINVAL;
    if (!keep || !counts) return LISO_EINVAL;
    if (n == 0 ? (boxes || sorted_keys || sorted_idx) : (!boxes || !sorted_keys || !sorted_idx)) return LISO_EINVAL;
    const int m_cap = pre_nms_max > 0 && pre_nms_max < n ? pre_nms_max : n;
    hipLaunchKernelGGL(det_nms_select_kernel, dim3(batch), dim3(kSelThreads), 0, (hipStream_t)stream, n, boxes, sorted_keys,
                       sorted_idx, thresh, m_cap, post_nms_max, (long long*)keep, counts);
    return check_launch();
}

int liso_det_nms_gather(int batch, int n, int post_nms_max, const int64_t* keep, const int32_t* counts,
                        const liso_det_gather_field* fields, int n_fields, void* stream) {
    if (batch <= 0 || batch > kMaxBatch || n < 0 || n > LISO_DET_NMS_MAX_N) return LISO_EINVAL;
    if (post_nms_max < 1 || post_nms_max > LISO_DET_NMS_MAX_POST) return LISO_EINVAL;
    if (!keep || !counts || !fields || n_fields < 1 || n_fields > LISO_DET_GATHER_MAX_FIELDS) return LISO_EINVAL;
    GatherArgs a;
    memset(&a, 0, sizeof(a));
    for (int i = 0; i < n_fields; i++) {
        const liso_det_gather_field& f = fields[i];
        const int eb = f.elem_bytes;
        if (!(eb == 1 || eb == 2 || eb == 4 || eb == 8) || f.row_elems < 1 || !f.dst) return LISO_EINVAL;
        if (n == 0 ? f.src != nullptr : f.src == nullptr) return LISO_EINVAL;
        if ((size_t)post_nms_max * (size_t)f.row_elems > (size_t)INT32_MAX) return LISO_EINVAL;
        a.f[i] = f;
    }
    hipLaunchKernelGGL(det_nms_gather_kernel, dim3(batch, n_fields), dim3(256), 0, (hipStream_t)stream, n, post_nms_max,
                       (const long long*)keep, counts, a);
    return check_launch();
}

}  // extern "C"
