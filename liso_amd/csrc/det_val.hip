// Detector validation matching for gfx950 (MI355X), C ABI in include/liso_det_val.h: the pair matrices of every frame of a padded
// batch in one launch, run_val's class transfer in one launch, every (job, frame) greedy matching in one launch, and every (job, frame)
// optimal assignment of the Waymo-style collections in one launch (assign_kernel, further down); and the per-frame part of the
// nuScenes detection metrics, every (frame, distance threshold) walk in one launch (nusc_kernel, include/liso_nusc_metrics.h).
//
// The work per matching is tiny (tens of boxes) and there are thousands of them per validation batch, so the shape is: one
// wavefront per (job, frame) cell, the serial walk over the predictions kept short --
//   * a lane owns the ground-truth slots lane, lane+64, ...: "in the filter set and not yet taken" is one bit per owned slot in
//     a register, so the walk touches no memory but the prediction's row of the pair matrix;
//   * the prediction order and the predictions' membership are staged in LDS once per cell;
//   * a prediction with no value past the threshold (most of them) costs one ballot; otherwise the best candidate is a 64-bit
//     key maximum over the wave: (order-preserving bits of the value, ~slot) -- largest value, lowest slot on ties, as
//     liso_match_greedy_f32;
//   * the matched pairs stay in LDS during the walk; the true-positive error terms are evaluated afterwards, one lane per
//     match, and added in match order in fp64.
// The pair geometry is rbev_geom.h's (shared with iou3d_nms.hip and det_nms.hip), so the BEV numbers equal
// liso_iou3d_*_f32 bit for bit.  Built with -ffp-contract=off: every expression the header states is evaluated operation by
// operation.
#include <hip/hip_runtime.h>
#include "dev_common.h"
#include "rbev_geom.h"
#include "rbev_geom_host.h"
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "../../include/liso_det_val.h"
#include "../../include/liso_nusc_metrics.h"

namespace {

using liso_dev::check_launch;
using namespace liso_rbev;

constexpr int kCols = 64;      // ground-truth slots per tile == wavefront width
constexpr int kRows = 16;      // prediction slots per tile
constexpr int kThreads = 256;  // 4 waves, each owns kRows/4 rows
constexpr int kMaxBoxes = LISO_DET_VAL_MAX_BOXES;
constexpr int kOwned = kMaxBoxes / 64;  // ground-truth slots a lane owns in the walk
static_assert(kThreads == kPolyThreads, "PolyLds holds one column per thread");
static_assert(kOwned <= 32, "one bit per owned slot in a 32-bit register");

// torch.min / torch.max, np.minimum: NaN if either operand is NaN
__host__ __device__ inline float nan_min(float a, float b) { return (a != a || b != b) ? NAN : (a < b ? a : b); }
__host__ __device__ inline float nan_max(float a, float b) { return (a != a || b != b) ? NAN : (a > b ? a : b); }

// the header's 3-D IoU from the BEV overlap; area = dx*dy of each box
__host__ __device__ inline float iou3d_from_overlap(float ov, float gz, float gdz, float garea, float pz, float pdz, float parea) {
    const float lo_g = gz - 0.5f * gdz, hi_g = gz + 0.5f * gdz;
    const float lo_p = pz - 0.5f * pdz, hi_p = pz + 0.5f * pdz;
    const float h = nan_min(hi_g, hi_p) - nan_max(lo_g, lo_p);
    const float inter = h > 0.f ? ov * h : 0.f;
    const float uni = garea * gdz + parea * pdz - inter;
    const float den = uni < FLT_EPSILON ? FLT_EPSILON : uni;  // NaN stays NaN
    return inter / den;
}

__host__ __device__ inline float centre_dist(const float* g, const float* p) {
    const float dx = g[0] - p[0], dy = g[1] - p[1];
    return sqrtf(dx * dx + dy * dy);
}

__host__ __device__ inline bool in_set(const float* b, uint8_t valid, int cls, const liso_det_val_filter& f) {
    if (!valid) return false;
    const float x = b[0], y = b[1];
    if (f.use_area && !(f.area_min_x <= x && x <= f.area_max_x && f.area_min_y <= y && y <= f.area_max_y)) return false;
    if (f.use_range) {
        const float r = sqrtf(x * x + y * y);
        if (!(f.range_min <= r && r < f.range_max)) return false;
    }
    if (f.class_id >= 0 && cls != f.class_id) return false;
    return true;
}

struct PairLds {
    float col[G_N][kCols];  // ground truth
    float row[G_N][kCols];  // predictions; only kRows used, same shape keeps one load_geo
    PolyLds poly;
};

__global__ __launch_bounds__(kThreads) void pairs_kernel(int G, int P, const float* __restrict__ gt,
                                                          const uint8_t* __restrict__ gv, const float* __restrict__ pred,
                                                          const uint8_t* __restrict__ pv, float* __restrict__ o_bev,
                                                          float* __restrict__ o_3d, float* __restrict__ o_dist) {
    __shared__ PairLds L;
    const int f = blockIdx.z, c0 = blockIdx.x * kCols, r0 = blockIdx.y * kRows;
    gt += (size_t)f * G * 7;
    gv += (size_t)f * G;
    pred += (size_t)f * P * 7;
    pv += (size_t)f * P;
    const int t = threadIdx.x;
    const bool want_overlap = o_bev != nullptr || o_3d != nullptr;
    if (want_overlap) {
        if (t < kCols) {
            const int g = c0 + t;
            if (g < G && gv[g]) store_geo(L.col, t, make_geo(gt + (size_t)g * 7));
        } else if (t < kCols + kRows) {
            const int p = r0 + (t - kCols);
            if (p < P && pv[p]) store_geo(L.row, t - kCols, make_geo(pred + (size_t)p * 7));
        }
    }
    __syncthreads();
    const int lane = t & 63, wave = t >> 6;
    const int g = c0 + lane;
    if (g >= G) return;
    const bool g_ok = gv[g] != 0;
    const float* gb = gt + (size_t)g * 7;
    Geo A;
    if (g_ok && want_overlap) A = load_geo(L.col, lane);
#pragma unroll 1
    for (int rr = wave; rr < kRows; rr += kThreads / 64) {
        const int p = r0 + rr;
        if (p >= P) break;
        float bev = 0.f, i3d = 0.f, d = 0.f;
        if (g_ok && pv[p]) {
            const float* pb = pred + (size_t)p * 7;
            if (want_overlap) {
                const Geo B = load_geo(L.row, rr);
                const float ov = box_overlap_dev(A, B, &L.poly, t);
                bev = iou_from_overlap(A, B, ov);
                i3d = iou3d_from_overlap(ov, gb[2], gb[5], A.area, pb[2], pb[5], B.area);
            }
            d = centre_dist(gb, pb);
        }
        const size_t o = ((size_t)f * P + p) * G + g;
        if (o_bev) o_bev[o] = bev;
        if (o_3d) o_3d[o] = i3d;
        if (o_dist) o_dist[o] = d;
    }
}

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const unsigned int lo = (unsigned int)__shfl_xor((int)(unsigned int)v, m);
        const unsigned int hi = (unsigned int)__shfl_xor((int)(unsigned int)(v >> 32), m);
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;
        v = o > v ? o : v;
    }
    return v;
}

// The greedy walk of one wavefront.  val: the frame's [P,G] matrix; s_order / s_pin: the prediction order and the predictions'
// membership, in LDS; avail: bit r = ground-truth slot lane + 64 r is in the set and free.  on_match(m, g, p) runs on every lane
// with the same arguments.  Returns the number of matches.
template <class OnMatch>
__device__ __forceinline__ int greedy_walk(const float* __restrict__ val, bool smaller_wins, float thr, int G, int P,
                                           const int* s_order, const uint8_t* s_pin, uint32_t avail, OnMatch on_match) {
    const int lane = threadIdx.x & 63;
    const float sgn = smaller_wins ? -1.f : 1.f;  // "smallest distance below thr" == "largest -distance above -thr", exactly
    const float t = sgn * thr;
    int m = 0;
    for (int k = 0; k < P; ++k) {
        const int p = s_order[k];
        if (p < 0 || p >= P || !s_pin[p]) continue;
        const float* row = val + (size_t)p * G;
        unsigned long long key = 0;
        uint32_t a = avail;
        for (int r = 0; a != 0u; ++r, a >>= 1) {
            if (!(a & 1u)) continue;
            const int g = lane + 64 * r;
            const float v = sgn * row[g];
            if (v > t) {  // NaN never passes
                const uint32_t u = __float_as_uint(v);
                const unsigned long long kk =
                    ((unsigned long long)(u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u)) << 32) | (0xFFFFFFFFu - (uint32_t)g);
                key = kk > key ? kk : key;
            }
        }
        if (__ballot(key != 0ull) == 0ull) continue;
        const unsigned long long top = wave_max_u64(key);
        const int bi = (int)(0xFFFFFFFFu - (uint32_t)top);
        if ((bi & 63) == lane) avail &= ~(1u << (bi >> 6));
        on_match(m, bi, p);
        ++m;
    }
    return m;
}

// the AOE term of one match (header), fp32
__host__ __device__ inline float orient_term(float yaw_gt, float yaw_pred) {
    const float pi = 3.14159265358979323846f, two_pi = (float)(2.0 * 3.14159265358979323846);
    float r = fmodf(yaw_gt - yaw_pred + pi, two_pi);
    if (r != 0.f) {
        if (r < 0.f) r = r + two_pi;
    } else {
        r = 0.f;
    }
    float d = r - pi;
    if (d > pi) d = d - two_pi;
    return fabsf(d);
}

// the three true-positive error terms of one match (header), fp32
__host__ __device__ inline void tp_terms(const float* g, const float* p, float& ate, float& ase, float& aoe) {
    ate = centre_dist(g, p);
    const float inter = nan_min(g[3], p[3]) * nan_min(g[4], p[4]) * nan_min(g[5], p[5]);
    const float uni = g[3] * g[4] * g[5] + p[3] * p[4] * p[5] - inter;
    const float den = uni < 1e-6f ? 1e-6f : uni;
    ase = 1.0f - inter / den;
    aoe = orient_term(g[6], p[6]);
}

struct MatchArgs {
    int G, P, S, J, M;
    const float* gt;
    const uint8_t* gv;
    const int32_t* gc;
    const float* pred;
    const uint8_t* pv;
    const int32_t* pc;
    const int32_t* order;
    const float* mat[3];
    const liso_det_val_filter* filters;
    const liso_det_val_job* jobs;
    int32_t* count;
    int16_t* pairs;
    double* sums;
    uint8_t* gt_in;
    uint8_t* pred_in;
};

__global__ __launch_bounds__(64) void match_kernel(MatchArgs a) {
    __shared__ int s_order[kMaxBoxes];
    __shared__ int s_pair[kMaxBoxes];  // (gt slot << 16) | pred slot
    __shared__ uint8_t s_pin[kMaxBoxes];
    const int lane = threadIdx.x;
    const size_t cell = blockIdx.x;
    const int f = (int)(cell / (size_t)a.J), j = (int)(cell - (size_t)f * a.J);
    const int G = a.G, P = a.P, M = a.M;
    const liso_det_val_job job = a.jobs[j];
    int16_t* pairs = a.pairs + cell * (size_t)M * 2;
    int m = 0;
    double ate = 0.0, ase = 0.0, aoe = 0.0;
    const bool ok = job.filter >= 0 && job.filter < a.S && job.criterion >= 0 && job.criterion <= 2;
    if (ok) {
        const liso_det_val_filter fl = a.filters[job.filter];
        const float* gt = a.gt + (size_t)f * G * 7;
        const float* pred = a.pred + (size_t)f * P * 7;
        uint32_t avail = 0u;
        for (int r = 0; r < kOwned; ++r) {
            const int g = lane + 64 * r;
            if (g >= G) break;
            const size_t s = (size_t)f * G + g;
            const bool in = in_set(gt + (size_t)g * 7, a.gv[s], a.gc[s], fl);
            a.gt_in[((size_t)f * a.S + job.filter) * G + g] = in ? 1 : 0;
            if (in) avail |= 1u << r;
        }
        for (int p = lane; p < P; p += 64) {
            const size_t s = (size_t)f * P + p;
            const bool in = in_set(pred + (size_t)p * 7, a.pv[s], a.pc[s], fl);
            a.pred_in[((size_t)f * a.S + job.filter) * P + p] = in ? 1 : 0;
            s_pin[p] = in ? 1 : 0;
            s_order[p] = a.order[s];
        }
        __syncthreads();
        if (G > 0 && P > 0) {
            const float* val = a.mat[job.criterion] + (size_t)f * P * G;
            m = greedy_walk(val, job.criterion == LISO_DET_VAL_DIST, job.threshold, G, P, s_order, s_pin, avail,
                            [&](int i, int g, int p) {
                                if (lane == 0 && i < M) s_pair[i] = (g << 16) | p;
                            });
            if (m > M) m = M;  // (only an `order` that names a slot twice gets here)
        }
        __syncthreads();
        for (int base = 0; base < m; base += 64) {
            const int i = base + lane;
            float ta = 0.f, ts = 0.f, to = 0.f;
            if (i < m) {
                const int g = s_pair[i] >> 16, p = s_pair[i] & 0xFFFF;
                pairs[2 * i] = (int16_t)g;
                pairs[2 * i + 1] = (int16_t)p;
                tp_terms(gt + (size_t)g * 7, pred + (size_t)p * 7, ta, ts, to);
            }
            const int n = m - base < 64 ? m - base : 64;
            for (int q = 0; q < n; ++q) {  // match order, every lane the same sum
                ate += (double)__shfl(ta, q);
                ase += (double)__shfl(ts, q);
                aoe += (double)__shfl(to, q);
            }
        }
    }
    for (int i = m + lane; i < M; i += 64) {
        pairs[2 * i] = -1;
        pairs[2 * i + 1] = -1;
    }
    if (lane == 0) {
        a.count[cell] = m;
        a.sums[cell * 3] = ate;
        a.sums[cell * 3 + 1] = ase;
        a.sums[cell * 3 + 2] = aoe;
    }
}

__global__ __launch_bounds__(64) void transfer_kernel(int G, int P, const uint8_t* __restrict__ gv,
                                                       const int32_t* __restrict__ gc, const uint8_t* __restrict__ pv,
                                                       const int32_t* __restrict__ order, const float* __restrict__ dist,
                                                       float thr, const int32_t* __restrict__ draws,
                                                       int32_t* __restrict__ out) {
    __shared__ int s_order[kMaxBoxes];
    __shared__ int s_cls[kMaxBoxes];
    __shared__ int s_gc[kMaxBoxes];
    __shared__ uint8_t s_pin[kMaxBoxes];
    const int lane = threadIdx.x, f = blockIdx.x;
    uint32_t avail = 0u;
    for (int r = 0; r < kOwned; ++r) {
        const int g = lane + 64 * r;
        if (g >= G) break;
        const size_t s = (size_t)f * G + g;
        s_gc[g] = gc[s];
        if (gv[s]) avail |= 1u << r;
    }
    for (int p = lane; p < P; p += 64) {
        const size_t s = (size_t)f * P + p;
        const bool in = pv[s] != 0;
        s_pin[p] = in ? 1 : 0;
        s_cls[p] = in ? draws[s] : -1;
        s_order[p] = order[s];
    }
    __syncthreads();
    if (G > 0 && P > 0)
        greedy_walk(dist + (size_t)f * P * G, true, thr, G, P, s_order, s_pin, avail, [&](int, int g, int p) {
            if (lane == 0) s_cls[p] = s_gc[g];
        });
    __syncthreads();
    for (int p = lane; p < P; p += 64) out[(size_t)f * P + p] = s_cls[p];
}

// ---- optimal assignment of a cell (header: "(4) Assign") ---------------------------------------------------------------------------
// Shortest augmenting paths with potentials, one wavefront per cell.  Rows: the smaller set, inserted one by one; columns: the larger
// set; a lane owns the column positions lane, lane + 64, ...  Potentials and running minima are fp64 in LDS, the "visited" flags one
// bit per owned column in a register.  A step of a row's search is one pass over the lane's unvisited columns (one value of the
// pair matrix each), a wave minimum of (reduced distance, assigned?, column position) and one pass that shifts potentials and minima
// by it.
// Only additions, subtractions and comparisons of fp64 values: liso_amd/eval/det_validation.py::assign_host performs the same
// operations in the same order and so finds the same pairs bit for bit.
struct AssignLds {
    double u[kMaxBoxes];          // row potentials
    double v[kMaxBoxes];          // column potentials
    double minv[kMaxBoxes];       // running minima of the current row's search
    int16_t way[kMaxBoxes];       // column visited before this one on its shortest path (-1: the search's start)
    int16_t owner[kMaxBoxes];     // row assigned to a column (-1: free)
    int16_t g_slot[kMaxBoxes];    // the members' slots in ascending order: one list is the rows, the other the columns
    int16_t p_slot[kMaxBoxes];
    int16_t col_of_row[kMaxBoxes];  // the result read by rows: a row's column position (-1: none)
    uint8_t gin[kMaxBoxes], pin[kMaxBoxes];
};
static_assert(sizeof(AssignLds) <= 48 * 1024, "static LDS of a cell");

// members of `in[0..n)` in ascending slot order -> list; every lane returns their number
__device__ __forceinline__ int compact_members(const uint8_t* in, int n, int16_t* list) {
    const int lane = threadIdx.x & 63;
    int k = 0;
    for (int base = 0; base < n; base += 64) {
        const int s = base + lane;
        const bool m = s < n && in[s] != 0;
        const unsigned long long b = __ballot(m);
        if (m) {
            list[k + __popcll(b & ((1ull << lane) - 1ull))] = (int16_t)s;
        }
        k += __popcll(b);
    }
    return k;
}

// the value of a pair as the assignment sees it: non-finite entries count as -1 (assignable, never kept)
__device__ __forceinline__ float assign_value(float x) { return (x - x == 0.f) ? x : -1.0f; }

// One cell.  val: [P,G] pred-major; L.gin / L.pin hold the membership of every slot (written by the caller, visible after its
// barrier).  Writes the kept pairs (ascending ground-truth slot) to pairs[0..M) and pads with (-1,-1); returns their number.
__device__ int assign_cell(AssignLds& L, const float* __restrict__ val, int G, int P, int M, float thr, int16_t* __restrict__ pairs) {
    const int lane = threadIdx.x & 63;
    const int n_g = compact_members(L.gin, G, L.g_slot), n_p = compact_members(L.pin, P, L.p_slot);
    __syncthreads();
    int kept = 0;
    if (n_g > 0 && n_p > 0) {
        const bool gt_rows = n_g <= n_p;  // the ground truth takes the rows when both sets are equally large
        const int n = gt_rows ? n_g : n_p, m = gt_rows ? n_p : n_g;
        const int16_t* row_slot = gt_rows ? L.g_slot : L.p_slot;
        const int16_t* col_slot = gt_rows ? L.p_slot : L.g_slot;
        // element strides of a step along the columns / of a row, in the pred-major matrix
        const size_t col_stride = gt_rows ? (size_t)G : 1, row_stride = gt_rows ? 1 : (size_t)G;
        const int owned = (m + 63) >> 6;
        for (int r = 0; r < owned; ++r) {
            const int j = lane + 64 * r;
            if (j < m) L.v[j] = 0.0, L.owner[j] = -1;
        }
        for (int i = lane; i < n; i += 64) L.u[i] = 0.0, L.col_of_row[i] = -1;
        __syncthreads();
        const double inf = __longlong_as_double(0x7FF0000000000000LL);
        for (int i = 0; i < n; ++i) {
            for (int r = 0; r < owned; ++r) {
                const int j = lane + 64 * r;
                if (j < m) L.minv[j] = inf;
            }
            uint32_t used = 0u;
            int j0 = -1;
            bool found = false;
            for (int step = 0; step <= n; ++step) {  // (a search visits at most the i assigned columns and one free one)
                const int i0 = j0 < 0 ? i : (int)L.owner[j0];
                const double ui = L.u[i0];
                const float* row = val + (size_t)row_slot[i0] * row_stride;
                double best = inf;
                int bj = 0x7FFFFFFF;
                for (int r = 0; r < owned; ++r) {
                    const int j = lane + 64 * r;
                    if (j >= m || ((used >> r) & 1u)) continue;
                    const float c = assign_value(row[(size_t)col_slot[j] * col_stride]);
                    const double cur = ((double)(-c) - ui) - L.v[j];
                    double mv = L.minv[j];
                    if (cur < mv) {
                        mv = cur;
                        L.minv[j] = cur;
                        L.way[j] = (int16_t)j0;
                    }
                    const int key = j | (L.owner[j] >= 0 ? kMaxBoxes : 0);  // on equal distances: a free column first, then the lowest position
                    if (mv < best || (mv == best && key < bj)) best = mv, bj = key;
                }
#pragma unroll
                for (int x = 32; x >= 1; x >>= 1) {  // wave minimum of (distance, key)
                    const long long bits = __double_as_longlong(best);
                    const int lo = __shfl_xor((int)(unsigned int)bits, x), hi = __shfl_xor((int)(bits >> 32), x);
                    const double ob = __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
                    const int oj = __shfl_xor(bj, x);
                    if (ob < best || (ob == best && oj < bj)) best = ob, bj = oj;
                }
                if (bj == 0x7FFFFFFF) break;  // (cannot happen: a free column exists and every value is finite)
                bj &= kMaxBoxes - 1;
                const double delta = best;
                for (int r = 0; r < owned; ++r) {
                    const int j = lane + 64 * r;
                    if (j >= m) continue;
                    if ((used >> r) & 1u) {
                        L.u[L.owner[j]] = L.u[L.owner[j]] + delta;
                        L.v[j] = L.v[j] - delta;
                    } else {
                        L.minv[j] = L.minv[j] - delta;
                    }
                }
                if (lane == 0) L.u[i] = L.u[i] + delta;
                j0 = bj;
                if ((j0 & 63) == lane) used |= 1u << (j0 >> 6);
                __syncthreads();
                if (L.owner[j0] < 0) {
                    found = true;
                    break;
                }
            }
            if (lane == 0 && found) {  // flip the path back to the start
                int j = j0;
                for (int guard = 0; guard <= n && j >= 0; ++guard) {
                    const int j1 = L.way[j];
                    L.owner[j] = j1 < 0 ? (int16_t)i : L.owner[j1];
                    j = j1;
                }
            }
            __syncthreads();
        }
        // the kept pairs in ascending ground-truth slot: position k of the ground truth's side (rows or columns) in ascending k
        if (gt_rows) {
            for (int r = 0; r < owned; ++r) {
                const int j = lane + 64 * r;
                if (j < m && L.owner[j] >= 0) L.col_of_row[L.owner[j]] = (int16_t)j;
            }
            __syncthreads();
        }
        for (int base = 0; base < n_g; base += 64) {
            const int k = base + lane;
            int g = -1, p = -1;
            bool keep = false;
            if (k < n_g) {
                const int q = gt_rows ? L.col_of_row[k] : L.owner[k];  // the prediction's position; -1: a column left free
                if (q >= 0) {
                    g = L.g_slot[k], p = L.p_slot[q];
                    keep = assign_value(val[(size_t)p * G + g]) >= thr;
                }
            }
            const unsigned long long b = __ballot(keep);
            if (keep) {
                const int at = kept + __popcll(b & ((1ull << lane) - 1ull));
                if (at < M) pairs[2 * at] = (int16_t)g, pairs[2 * at + 1] = (int16_t)p;
            }
            kept += __popcll(b);
        }
        if (kept > M) kept = M;
    }
    for (int i = kept + lane; i < M; i += 64) pairs[2 * i] = -1, pairs[2 * i + 1] = -1;
    return kept;
}

struct AssignArgs {
    int G, P, S, J, M;
    const float* gt;
    const uint8_t* gv;
    const int32_t* gc;
    const float* pred;
    const uint8_t* pv;
    const int32_t* pc;
    const float* mat[2];
    const liso_det_val_filter* filters;
    const liso_det_val_job* jobs;
    int32_t* count;
    int16_t* pairs;
    uint8_t* gt_in;
    uint8_t* pred_in;
};

__global__ __launch_bounds__(64) void assign_kernel(AssignArgs a) {
    __shared__ AssignLds L;
    const int lane = threadIdx.x;
    const size_t cell = blockIdx.x;
    const int f = (int)(cell / (size_t)a.J), j = (int)(cell - (size_t)f * a.J);
    const int G = a.G, P = a.P, M = a.M;
    const liso_det_val_job job = a.jobs[j];
    int16_t* pairs = a.pairs + cell * (size_t)M * 2;
    const bool set_ok = job.filter >= 0 && job.filter < a.S;
    const bool ok = set_ok && (job.criterion == LISO_DET_VAL_IOU_BEV || job.criterion == LISO_DET_VAL_IOU_3D);
    liso_det_val_filter fl = {};
    if (set_ok) fl = a.filters[job.filter];
    const float* gt = a.gt + (size_t)f * G * 7;
    const float* pred = a.pred + (size_t)f * P * 7;
    for (int g = lane; g < G; g += 64) {
        const size_t s = (size_t)f * G + g;
        const bool in = set_ok && in_set(gt + (size_t)g * 7, a.gv[s], a.gc[s], fl);
        if (set_ok) a.gt_in[((size_t)f * a.S + job.filter) * G + g] = in ? 1 : 0;
        L.gin[g] = (in && ok) ? 1 : 0;
    }
    for (int p = lane; p < P; p += 64) {
        const size_t s = (size_t)f * P + p;
        const bool in = set_ok && in_set(pred + (size_t)p * 7, a.pv[s], a.pc[s], fl);
        if (set_ok) a.pred_in[((size_t)f * a.S + job.filter) * P + p] = in ? 1 : 0;
        L.pin[p] = (in && ok) ? 1 : 0;
    }
    __syncthreads();
    const float* val = a.mat[ok ? job.criterion : 0];
    if (val) val += (size_t)f * P * G;
    const int kept = assign_cell(L, val, G, P, M, job.threshold, pairs);
    if (lane == 0) a.count[cell] = kept;
}

__global__ __launch_bounds__(64) void assign_plain_kernel(int G, int P, int M, const float* __restrict__ val, float thr,
                                                           int32_t* __restrict__ count, int16_t* __restrict__ pairs) {
    __shared__ AssignLds L;
    const int lane = threadIdx.x;
    const size_t cell = blockIdx.x;
    for (int g = lane; g < G; g += 64) L.gin[g] = 1;
    for (int p = lane; p < P; p += 64) L.pin[p] = 1;
    __syncthreads();
    const int kept = assign_cell(L, val + cell * (size_t)P * G, G, P, M, thr, pairs + cell * (size_t)M * 2);
    if (lane == 0) count[cell] = kept;
}

// ---- nuScenes detection metrics, the per-frame part (include/liso_nusc_metrics.h) -----------------------------------------------------
// One wavefront per (frame, threshold) cell.  Unlike match_kernel the walk reads no pair matrix: a lane keeps x, y and class of its
// ground-truth slots in registers next to the "member and free" bits and computes the centre distance of a step on the fly; the
// member predictions are compacted into visiting order in LDS first, so the serial loop has no skipped iterations.  The best
// candidate of a step is a 64-bit key maximum (~bits of the distance, ~slot): distances are >= +0 and never NaN here, so their bit
// patterns order like their values -- smallest distance, lowest slot on ties.
struct NuscArgs {
    int G, P, T, M, n_classes, as_one;
    const float* gt;
    const uint8_t* gv;
    const int32_t* gc;
    const float* pred;
    const uint8_t* pv;
    const int32_t* pc;
    const int32_t* order;
    const float* radius;
    float thr[LISO_NUSC_MAX_THRESHOLDS];
    int32_t* count;
    int16_t* pairs;
    float* err;
    uint8_t* gt_in;
    uint8_t* pred_in;
};

// the header's membership; `cls` is already 0 when every box counts as one class
__device__ __forceinline__ bool nusc_member(float x, float y, uint8_t valid, int cls, int n_classes, const float* __restrict__ radius) {
    if (!valid || cls < 0 || cls >= n_classes) return false;
    return sqrtf(x * x + y * y) <= radius[cls];  // NaN fails
}

// the header's scale term: the prediction's sizes raised to 1e-4f, no clamp on the union
__host__ __device__ inline float nusc_scale_term(const float* g, const float* p) {
    const float sx = p[3] < 1e-4f ? 1e-4f : p[3], sy = p[4] < 1e-4f ? 1e-4f : p[4], sz = p[5] < 1e-4f ? 1e-4f : p[5];
    const float inter = (nan_min(g[3], sx) * nan_min(g[4], sy)) * nan_min(g[5], sz);
    const float uni = (g[3] * g[4]) * g[5] + (sx * sy) * sz - inter;
    return 1.0f - inter / uni;
}

__global__ __launch_bounds__(64) void nusc_kernel(NuscArgs a) {
    __shared__ float s_px[kMaxBoxes], s_py[kMaxBoxes];
    __shared__ int s_pc[kMaxBoxes];
    __shared__ int s_pair[kMaxBoxes];     // (gt slot << 16) | pred slot
    __shared__ int16_t s_vis[kMaxBoxes];  // the member predictions in visiting order
    __shared__ uint8_t s_pin[kMaxBoxes];
    const int lane = threadIdx.x;
    const size_t cell = blockIdx.x;
    const int f = (int)(cell / (size_t)a.T), t = (int)(cell - (size_t)f * a.T);
    const int G = a.G, P = a.P, M = a.M;
    const float thr = a.thr[t];
    const float* gt = a.gt + (size_t)f * G * 7;
    const float* pred = a.pred + (size_t)f * P * 7;
    const int owned = (G + 63) >> 6;
    float gx[kOwned], gy[kOwned];
    int gc[kOwned];
    uint32_t avail = 0u;
#pragma unroll
    for (int r = 0; r < kOwned; ++r) {
        const int g = lane + 64 * r;
        float x = 0.f, y = 0.f;
        int c = -1;
        bool in = false;
        if (g < G) {
            const size_t s = (size_t)f * G + g;
            c = a.as_one ? 0 : a.gc[s];
            x = gt[(size_t)g * 7], y = gt[(size_t)g * 7 + 1];
            in = nusc_member(x, y, a.gv[s], c, a.n_classes, a.radius);
            if (t == 0) a.gt_in[s] = in ? 1 : 0;  // the same for every threshold: the frame's first cell writes it
        }
        gx[r] = x, gy[r] = y, gc[r] = c;  // (assigned outside the branch: the arrays stay plain registers)
        avail |= (in ? 1u : 0u) << r;
    }
    for (int p = lane; p < P; p += 64) {
        const size_t s = (size_t)f * P + p;
        const int c = a.as_one ? 0 : a.pc[s];
        const float x = pred[(size_t)p * 7], y = pred[(size_t)p * 7 + 1];
        const bool in = nusc_member(x, y, a.pv[s], c, a.n_classes, a.radius);
        if (t == 0) a.pred_in[s] = in ? 1 : 0;
        s_pin[p] = in ? 1 : 0;
        s_px[p] = x, s_py[p] = y, s_pc[p] = c;
    }
    __syncthreads();
    int n_vis = 0;
    for (int base = 0; base < P; base += 64) {
        const int k = base + lane;
        int p = -1;
        if (k < P) {
            p = a.order[(size_t)f * P + k];
            if (p < 0 || p >= P || !s_pin[p]) p = -1;
        }
        const unsigned long long b = __ballot(p >= 0);
        if (p >= 0) s_vis[n_vis + __popcll(b & ((1ull << lane) - 1ull))] = (int16_t)p;
        n_vis += __popcll(b);
    }
    __syncthreads();
    int m = 0;
#pragma unroll 1
    for (int k = 0; k < n_vis; ++k) {
        const int p = s_vis[k];
        const float px = s_px[p], py = s_py[p];
        const int pc = s_pc[p];
        unsigned long long key = 0;
#pragma unroll
        for (int r = 0; r < kOwned; ++r) {
            if (r >= owned) break;
            if (!((avail >> r) & 1u) || gc[r] != pc) continue;
            const float dx = gx[r] - px, dy = gy[r] - py;
            const float d = sqrtf(dx * dx + dy * dy);
            if (d < thr) {  // NaN never passes
                const unsigned long long kk =
                    ((unsigned long long)(0xFFFFFFFFu - __float_as_uint(d)) << 32) | (0xFFFFFFFFu - (uint32_t)(lane + 64 * r));
                key = kk > key ? kk : key;
            }
        }
        if (__ballot(key != 0ull) == 0ull) continue;
        const unsigned long long top = wave_max_u64(key);
        const int bi = (int)(0xFFFFFFFFu - (uint32_t)top);
        if ((bi & 63) == lane) avail &= ~(1u << (bi >> 6));
        if (lane == 0 && m < M) s_pair[m] = (bi << 16) | p;
        ++m;
    }
    if (m > M) m = M;  // (only an `order` that names a slot twice gets here)
    __syncthreads();
    int16_t* pairs = a.pairs + cell * (size_t)M * 2;
    float* err = a.err + cell * (size_t)M * 3;
#pragma unroll 1
    for (int i = lane; i < M; i += 64) {
        int g = -1, p = -1;
        float e_t = 0.f, e_s = 0.f, e_o = 0.f;
        if (i < m) {
            g = s_pair[i] >> 16, p = s_pair[i] & 0xFFFF;
            const float* gb = gt + (size_t)g * 7;
            const float* pb = pred + (size_t)p * 7;
            e_t = centre_dist(gb, pb);
            e_s = nusc_scale_term(gb, pb);
            e_o = orient_term(gb[6], pb[6]);
            const float qnan = __uint_as_float(0x7FC00000u);  // one NaN pattern, whatever operation made it
            if (e_s != e_s) e_s = qnan;
            if (e_o != e_o) e_o = qnan;
        }
        pairs[2 * i] = (int16_t)g, pairs[2 * i + 1] = (int16_t)p;
        err[3 * i] = e_t, err[3 * i + 1] = e_s, err[3 * i + 2] = e_o;
    }
    if (lane == 0) a.count[cell] = m;
}

bool bad_shape(int frames, int G, int P) { return frames < 0 || G < 0 || P < 0 || G > kMaxBoxes || P > kMaxBoxes; }

}  // namespace

extern "C" {

int liso_det_val_pairs_f32(int frames, int n_gt, int n_pred, const float* gt, const uint8_t* gt_valid, const float* pred,
                           const uint8_t* pred_valid, float* iou_bev, float* iou_3d, float* dist, void* stream) {
    if (bad_shape(frames, n_gt, n_pred)) return LISO_EINVAL;
    if (frames == 0 || n_gt == 0 || n_pred == 0) return LISO_OK;
    if (!gt || !gt_valid || !pred || !pred_valid) return LISO_EINVAL;
    if (!iou_bev && !iou_3d && !dist) return LISO_OK;
    if (frames > 65535) return LISO_EINVAL;
    const dim3 grid((n_gt + kCols - 1) / kCols, (n_pred + kRows - 1) / kRows, frames);
    hipLaunchKernelGGL(pairs_kernel, grid, dim3(kThreads), 0, (hipStream_t)stream, n_gt, n_pred, gt, gt_valid, pred, pred_valid,
                       iou_bev, iou_3d, dist);
    return check_launch();
}

int liso_det_val_pairs_cpu_f32(int frames, int n_gt, int n_pred, const float* gt, const uint8_t* gt_valid, const float* pred,
                               const uint8_t* pred_valid, float* iou_bev, float* iou_3d, float* dist) {
    using namespace liso_rbev_host;
    if (bad_shape(frames, n_gt, n_pred)) return LISO_EINVAL;
    if (frames == 0 || n_gt == 0 || n_pred == 0) return LISO_OK;
    if (!gt || !gt_valid || !pred || !pred_valid) return LISO_EINVAL;
    for (int f = 0; f < frames; ++f)
        for (int p = 0; p < n_pred; ++p)
            for (int g = 0; g < n_gt; ++g) {
                const float* gb = gt + ((size_t)f * n_gt + g) * 7;
                const float* pb = pred + ((size_t)f * n_pred + p) * 7;
                float bev = 0.f, i3d = 0.f, d = 0.f;
                if (gt_valid[(size_t)f * n_gt + g] && pred_valid[(size_t)f * n_pred + p]) {
                    if (iou_bev || iou_3d) {
                        const float ov = h_overlap_bev(gb, pb);
                        bev = h_iou_from_overlap(gb, pb, ov);
                        i3d = iou3d_from_overlap(ov, gb[2], gb[5], gb[3] * gb[4], pb[2], pb[5], pb[3] * pb[4]);
                    }
                    d = centre_dist(gb, pb);
                }
                const size_t o = ((size_t)f * n_pred + p) * n_gt + g;
                if (iou_bev) iou_bev[o] = bev;
                if (iou_3d) iou_3d[o] = i3d;
                if (dist) dist[o] = d;
            }
    return LISO_OK;
}

int liso_det_val_transfer_classes(int frames, int n_gt, int n_pred, const uint8_t* gt_valid, const int32_t* gt_class,
                                  const uint8_t* pred_valid, const int32_t* order, const float* dist, float threshold,
                                  const int32_t* draws, int32_t* pred_class_out, void* stream) {
    if (bad_shape(frames, n_gt, n_pred)) return LISO_EINVAL;
    if (frames == 0 || n_pred == 0) return LISO_OK;
    if (!pred_valid || !order || !draws || !pred_class_out) return LISO_EINVAL;
    if (n_gt > 0 && (!gt_valid || !gt_class || !dist)) return LISO_EINVAL;
    hipLaunchKernelGGL(transfer_kernel, dim3(frames), dim3(64), 0, (hipStream_t)stream, n_gt, n_pred, gt_valid, gt_class,
                       pred_valid, order, dist, threshold, draws, pred_class_out);
    return check_launch();
}

int liso_det_val_match_f32(int frames, int n_gt, int n_pred, const float* gt, const uint8_t* gt_valid, const int32_t* gt_class,
                           const float* pred, const uint8_t* pred_valid, const int32_t* pred_class, const int32_t* order,
                           const float* iou_bev, const float* iou_3d, const float* dist, int criteria_mask,
                           const liso_det_val_filter* filters, int n_filters, const liso_det_val_job* jobs, int n_jobs,
                           int32_t* count, int16_t* pairs, double* sums, uint8_t* gt_in, uint8_t* pred_in, void* stream) {
    if (bad_shape(frames, n_gt, n_pred) || n_filters < 0 || n_jobs < 0 || criteria_mask < 0 || criteria_mask > 7) return LISO_EINVAL;
    if (frames == 0 || n_jobs == 0) return LISO_OK;
    if (n_filters == 0 || !filters || !jobs || !count || !sums) return LISO_EINVAL;
    if (n_gt > 0 && (!gt || !gt_valid || !gt_class || !gt_in)) return LISO_EINVAL;
    if (n_pred > 0 && (!pred || !pred_valid || !pred_class || !order || !pred_in)) return LISO_EINVAL;
    const int M = n_gt < n_pred ? n_gt : n_pred;
    if (M > 0) {
        if (!pairs) return LISO_EINVAL;
        const float* mats[3] = {iou_bev, iou_3d, dist};
        for (int c = 0; c < 3; ++c)
            if (((criteria_mask >> c) & 1) && !mats[c]) return LISO_EINVAL;
    }
    if ((long long)frames * n_jobs > 0x7FFFFFFFLL) return LISO_EINVAL;
    MatchArgs a;
    a.G = n_gt, a.P = n_pred, a.S = n_filters, a.J = n_jobs, a.M = M;
    a.gt = gt, a.gv = gt_valid, a.gc = gt_class, a.pred = pred, a.pv = pred_valid, a.pc = pred_class, a.order = order;
    // a criterion whose bit is not set never reaches its matrix: point it at one that is there so a job that names it reads valid memory
    const float* any = iou_bev ? iou_bev : (iou_3d ? iou_3d : dist);
    if (M > 0 && !any) return LISO_EINVAL;
    a.mat[0] = iou_bev ? iou_bev : any, a.mat[1] = iou_3d ? iou_3d : any, a.mat[2] = dist ? dist : any;
    a.filters = filters, a.jobs = jobs, a.count = count, a.pairs = pairs, a.sums = sums, a.gt_in = gt_in, a.pred_in = pred_in;
    hipLaunchKernelGGL(match_kernel, dim3((unsigned)(frames * n_jobs)), dim3(64), 0, (hipStream_t)stream, a);
    return check_launch();
}

int liso_det_val_assign_f32(int frames, int n_gt, int n_pred, const float* gt, const uint8_t* gt_valid, const int32_t* gt_class,
                            const float* pred, const uint8_t* pred_valid, const int32_t* pred_class, const float* iou_bev,
                            const float* iou_3d, int criteria_mask, const liso_det_val_filter* filters, int n_filters,
                            const liso_det_val_job* jobs, int n_jobs, int32_t* count, int16_t* pairs, uint8_t* gt_in, uint8_t* pred_in,
                            void* stream) {
    if (bad_shape(frames, n_gt, n_pred) || n_filters < 0 || n_jobs < 0 || criteria_mask < 0 || criteria_mask > 3) return LISO_EINVAL;
    if (frames == 0 || n_jobs == 0) return LISO_OK;
    if (n_filters == 0 || !filters || !jobs || !count) return LISO_EINVAL;
    if (n_gt > 0 && (!gt || !gt_valid || !gt_class || !gt_in)) return LISO_EINVAL;
    if (n_pred > 0 && (!pred || !pred_valid || !pred_class || !pred_in)) return LISO_EINVAL;
    const int M = n_gt < n_pred ? n_gt : n_pred;
    const float* any = iou_bev ? iou_bev : iou_3d;
    if (M > 0) {
        if (!pairs || !any) return LISO_EINVAL;
        if (((criteria_mask & 1) && !iou_bev) || ((criteria_mask & 2) && !iou_3d)) return LISO_EINVAL;
    }
    if ((long long)frames * n_jobs > 0x7FFFFFFFLL) return LISO_EINVAL;
    AssignArgs a;
    a.G = n_gt, a.P = n_pred, a.S = n_filters, a.J = n_jobs, a.M = M;
    a.gt = gt, a.gv = gt_valid, a.gc = gt_class, a.pred = pred, a.pv = pred_valid, a.pc = pred_class;
    a.mat[0] = iou_bev ? iou_bev : any, a.mat[1] = iou_3d ? iou_3d : any;  // (as liso_det_val_match_f32: never a NULL read)
    a.filters = filters, a.jobs = jobs, a.count = count, a.pairs = pairs, a.gt_in = gt_in, a.pred_in = pred_in;
    hipLaunchKernelGGL(assign_kernel, dim3((unsigned)(frames * n_jobs)), dim3(64), 0, (hipStream_t)stream, a);
    return check_launch();
}

int liso_match_assign_f32(const float* value_pred_major, long batch, int n_gt, int n_pred, float threshold, int32_t* count,
                          int16_t* pairs, void* stream) {
    if (batch < 0 || batch > 0x7FFFFFFFL || bad_shape(0, n_gt, n_pred)) return LISO_EINVAL;
    if (batch == 0) return LISO_OK;
    if (!count) return LISO_EINVAL;
    const int M = n_gt < n_pred ? n_gt : n_pred;
    if (M > 0 && (!value_pred_major || !pairs)) return LISO_EINVAL;
    hipLaunchKernelGGL(assign_plain_kernel, dim3((unsigned)batch), dim3(64), 0, (hipStream_t)stream, n_gt, n_pred, M, value_pred_major,
                       threshold, count, pairs);
    return check_launch();
}

int liso_det_val_nusc_f32(int frames, int n_gt, int n_pred, const float* gt, const uint8_t* gt_valid, const int32_t* gt_class,
                          const float* pred, const uint8_t* pred_valid, const int32_t* pred_class, const int32_t* order,
                          const float* radius, int n_classes, int as_one, const float* thresholds, int n_thresholds, int32_t* count,
                          int16_t* pairs, float* err, uint8_t* gt_in, uint8_t* pred_in, void* stream) {
    if (bad_shape(frames, n_gt, n_pred) || n_classes < 1 || n_thresholds < 1 || n_thresholds > LISO_NUSC_MAX_THRESHOLDS) return LISO_EINVAL;
    if (frames == 0) return LISO_OK;
    if (!radius || !thresholds || !count) return LISO_EINVAL;
    if (n_gt > 0 && (!gt || !gt_valid || !gt_in || (!as_one && !gt_class))) return LISO_EINVAL;
    if (n_pred > 0 && (!pred || !pred_valid || !order || !pred_in || (!as_one && !pred_class))) return LISO_EINVAL;
    const int M = n_gt < n_pred ? n_gt : n_pred;
    if (M > 0 && (!pairs || !err)) return LISO_EINVAL;
    if ((long long)frames * n_thresholds > 0x7FFFFFFFLL) return LISO_EINVAL;
    NuscArgs a;
    a.G = n_gt, a.P = n_pred, a.T = n_thresholds, a.M = M, a.n_classes = n_classes, a.as_one = as_one ? 1 : 0;
    a.gt = gt, a.gv = gt_valid, a.gc = gt_class, a.pred = pred, a.pv = pred_valid, a.pc = pred_class, a.order = order, a.radius = radius;
    for (int i = 0; i < LISO_NUSC_MAX_THRESHOLDS; ++i) a.thr[i] = i < n_thresholds ? thresholds[i] : 0.f;
    a.count = count, a.pairs = pairs, a.err = err, a.gt_in = gt_in, a.pred_in = pred_in;
    hipLaunchKernelGGL(nusc_kernel, dim3((unsigned)(frames * n_thresholds)), dim3(64), 0, (hipStream_t)stream, a);
    return check_launch();
}

}  // extern "C"
