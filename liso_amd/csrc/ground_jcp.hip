// JCP range-image ground removal, the cone test and ground-point removal on gfx950.  C ABI, stages and semantics:
// include/liso_ground.h.  Compiled without FMA contraction: every threshold is the reference's fp64 expression, operation by operation.
//
// Images: `widx` (the reference's cloud_index_) is laid out col * H + row as in the reference, because the candidate filter
// reads it with a transposed index; the label images are row-major (row * W + col), the order JCP visits candidates in.
// Labels: kEmpty = no point in the pixel (never scored), kGround, kObstacle, kCandidate = not resolved yet (never scored).
//
// Resolve (stage 5).  A candidate reads the labels of its 5x5 window.  The ones before it in raster order -- rows r-2, r-1 at
// columns c-2..c+2 and row r at c-2, c-1 -- must be final, the others must still be as the candidate stage left them.  With row
// r running three columns behind row r-1 (lane r resolves column t - 3r at step t, one barrier per step) both hold: at step t
// row r-1 has finished column c+2 in step t-1 and writes c+3, row r+1 has finished c-4 and writes c-3.  The 24 weights do not
// depend on labels; stage 4 leaves them per row in column order, and every lane loads the weights of its next candidate right
// after it has resolved one, so that the load is not part of the step that needs them.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "../../include/liso_box_mining.h"
#include "../../include/liso_ground.h"
#include "dev_common.h"
#include "per_device.h"

namespace {

using liso_dev::Carver;
using liso_dev::check_launch;
using liso_dev::cloud_rows;
using liso_dev::to_i32;
using liso_dev::up256;

constexpr int kThreads = 256;
constexpr int kNb = 24;
constexpr double kMinRange = 3.0, kMaxRange = 70.0, kThG = 0.3, kSigmaDeg = 7.0;
enum : uint8_t { kEmpty = 0, kGround = 1, kObstacle = 2, kCandidate = 3 };

struct Tables {
    unsigned long long* ele_key;  // [B][2] ordered keys of min / max finite elevation
    double* ele;                  // [B][N]
    int32_t* pix;                 // [B][N] col * H + row of the pixel the point's label is read from, -1 for invalid rows
    int32_t* widx;                // [B][W*H] winner point per pixel, -1 = none
    uint32_t* minz_key;           // [B][W*L] ordered fp32 key of the smallest z per (column, region)
    double* minz;                 // [B][W*L] the same as fp64, then RECM's thresholds
    uint8_t* lab0;                // [B][lab_stride] labels after RECM
    uint8_t* lab1;                // [B][lab_stride] labels after the candidate filter, then final
    int32_t* row_cnt;             // [B][H] candidates per row
    int32_t* cols;                // [B][H*W] their columns, ascending, row r at r * W
    double* wts;                  // [B][H*W][24] their weights, same slots
    size_t bytes;
};

struct Dims {
    int B, N, stride, W, H, L;
    size_t lab_stride;  // H*W rounded up to 16
};

// 0 = fine, else the error code
int read_cfg(const liso_ground_cfg* c, Dims* d) {
    if (!c) return LISO_EINVAL;
    if (c->batch < 1 || c->n_max < 0 || c->n_max > LISO_GROUND_MAX_N || c->point_stride < 3) return LISO_EINVAL;
    if (c->width < 1 || c->height < 1 || c->height > LISO_GROUND_MAX_HEIGHT) return LISO_EINVAL;
    if ((long)c->width * c->height > LISO_GROUND_MAX_PIXELS) return LISO_EINVAL;
    // the candidate filter reads widx[row * H + col]
    if ((long)(c->height - 1) * c->height + c->width - 1 >= (long)c->width * c->height) return LISO_EINVAL;
    if (!(c->delta_r > 0.0) || !isfinite(c->delta_r) || !isfinite(c->sensor_height)) return LISO_EINVAL;
    const double len = (kMaxRange - kMinRange) / c->delta_r;
    if (len >= 256.0) return LISO_GROUND_ELENGTH;
    if ((int)len < 1) return LISO_EINVAL;
    d->B = c->batch, d->N = c->n_max, d->stride = c->point_stride, d->W = c->width, d->H = c->height, d->L = (int)len;
    d->lab_stride = ((size_t)d->W * d->H + 15) / 16 * 16;
    if ((size_t)d->B * d->lab_stride * kNb * sizeof(double) > ((size_t)1 << 40)) return LISO_EINVAL;
    return LISO_OK;
}

Tables carve(const Dims& d, void* base) {
    Tables t;
    Carver ws{base};
    const size_t B = d.B, N = d.N, WH = (size_t)d.W * d.H, WL = (size_t)d.W * d.L;
    t.ele_key = ws.take<unsigned long long>(B * 2);
    t.ele = ws.take<double>(B * N);
    t.pix = ws.take<int32_t>(B * N);
    t.widx = ws.take<int32_t>(B * WH);
    t.minz_key = ws.take<uint32_t>(B * WL);
    t.minz = ws.take<double>(B * WL);
    t.lab0 = ws.take<uint8_t>(B * d.lab_stride);
    t.lab1 = ws.take<uint8_t>(B * d.lab_stride);
    t.row_cnt = ws.take<int32_t>(B * d.H);
    t.cols = ws.take<int32_t>(B * WH);
    t.wts = ws.take<double>(B * WH * kNb);
    t.bytes = ws.bytes;
    return t;
}

// ---- order-preserving integer keys ------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t key_f32(float v) {
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float unkey_f32(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }
__device__ __forceinline__ unsigned long long key_f64(double v) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double unkey_f64(unsigned long long k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k));
}

// Python's min(a, b)
__device__ __forceinline__ double pymin(double a, double b) { return b < a ? b : a; }


__device__ __forceinline__ bool load_point(const float* pcl, const int32_t* counts, int b, int i, int N, int stride, double* x, double* y,
                                           double* z, float* zf) {
    if (i >= cloud_rows(counts, b, N)) return false;
    const float* p = pcl + ((size_t)b * N + i) * stride;
    const float fx = p[0], fy = p[1], fz = p[2];
    *x = (double)fx, *y = (double)fy, *z = (double)fz, *zf = fz;
    return !(isnan(fx) || isnan(fy) || isnan(fz));
}

// ---- stage 0 -----------------------------------------------------------------------------------------------------------------------
__global__ void init_kernel(Tables t, size_t n_widx, size_t n_minz, int B) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const size_t i0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (size_t i = i0; i < n_widx; i += stride) t.widx[i] = -1;
    const uint32_t k100 = key_f32(100.0f);
    for (size_t i = i0; i < n_minz; i += stride) t.minz_key[i] = k100;
    for (size_t i = i0; i < (size_t)B; i += stride) {
        t.ele_key[2 * i] = ~0ull;    // min
        t.ele_key[2 * i + 1] = 0ull;  // max
    }
}

// ---- stage 1 -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void elevation_kernel(Tables t, Dims d, const float* pcl, const int32_t* counts) {
    const int b = blockIdx.y, i = blockIdx.x * kThreads + threadIdx.x;
    double mn = INFINITY, mx = -INFINITY;
    if (i < d.N) {
        double x, y, z;
        float zf;
        if (load_point(pcl, counts, b, i, d.N, d.stride, &x, &y, &z, &zf)) {
            const double r = sqrt(x * x + y * y);
            double a = z / fmax(r, 1e-6);
            if (a > 1.0) a = 1.0;
            else if (a < -1.0) a = -1.0;
            const double e = asin(a);
            t.ele[(size_t)b * d.N + i] = e;
            if (isfinite(e)) mn = e, mx = e;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mn = fmin(mn, __shfl_xor(mn, o, 64));
        mx = fmax(mx, __shfl_xor(mx, o, 64));
    }
    __shared__ double s_mn[kThreads / 64], s_mx[kThreads / 64];
    if ((threadIdx.x & 63) == 0) s_mn[threadIdx.x >> 6] = mn, s_mx[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kThreads / 64; ++w) mn = fmin(mn, s_mn[w]), mx = fmax(mx, s_mx[w]);
        if (mn <= mx) {
            atomicMin(&t.ele_key[2 * b], key_f64(mn));
            atomicMax(&t.ele_key[2 * b + 1], key_f64(mx));
        }
    }
}

// ---- stage 2 -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void project_kernel(Tables t, Dims d, const float* pcl, const int32_t* counts, double delta_r) {
    const int b = blockIdx.y, i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= d.N) return;
    double x, y, z;
    float zf;
    int32_t* pix = t.pix + (size_t)b * d.N + i;
    if (!load_point(pcl, counts, b, i, d.N, d.stride, &x, &y, &z, &zf)) {
        *pix = -1;
        return;
    }
    const double min_ele = unkey_f64(t.ele_key[2 * b]), max_ele = unkey_f64(t.ele_key[2 * b + 1]);
    const double e = t.ele[(size_t)b * d.N + i];
    int row = to_i32(((double)d.H * (e - min_ele)) / (max_ele - min_ele));
    row = row < 0 ? 0 : (row > d.H - 1 ? d.H - 1 : row);
    double ang = atan2(y, x);
    if (y < 0.0) ang = ang + 2.0 * M_PI;
    const int col = to_i32(((double)(d.W - 1) * (ang * 180.0 / M_PI)) / 360.0);
    // y == -0.0 with x < 0: atan2 gives -pi, `y < 0` is false, the column is trunc(-(W-1)/2).  The reference keeps such a point
    // out of the projection (col < 0) and reads its label with numpy's negative index, at column W + col.
    const int read_col = col < 0 ? col + d.W : col;
    if (read_col < 0 || read_col >= d.W) {  // not reachable: the angle lies in [-pi, 2 pi]
        *pix = -1;
        return;
    }
    *pix = read_col * d.H + row;
    if (col < 0) return;
    const double r = sqrt(x * x + y * y);
    // the reference's bounds tests on col / row (> W, > H) and its z clause never hold
    if (r < kMinRange || r > kMaxRange || ((x < 3.0 && x > -2.0) && (y < 1.5 && y > -1.5))) return;
    const int region = (int)((r - kMinRange) / delta_r);
    const size_t ri = (size_t)col * d.L + region;  // region == L for r == 70: the reference's flat index, next column's region 0
    if (ri < (size_t)d.W * d.L) atomicMin(&t.minz_key[(size_t)b * d.W * d.L + ri], key_f32(zf));
    atomicMax(&t.widx[(size_t)b * d.W * d.H + col * d.H + row], i);
}

// ---- stage 3 -----------------------------------------------------------------------------------------------------------------------
__global__ void recm_kernel(Tables t, Dims d, double ground_level, double sensor_height, double step) {
    const int b = blockIdx.y, col = blockIdx.x * blockDim.x + threadIdx.x;
    if (col >= d.W) return;
    const size_t base = ((size_t)b * d.W + col) * d.L;
    const uint32_t* key = t.minz_key + base;
    double* m = t.minz + base;
    const int L = d.L;
    for (int j = 0; j < L; ++j) m[j] = (double)unkey_f32(key[j]);
    // first scan (jcp.py:75-94): holes, in-place three-point smoothing reading the updated [j-1] and the original [j+1]
    bool flag = false;
    double prev = pymin(m[0], ground_level);
    m[0] = prev;
    for (int j = 1; j + 1 < L; ++j) {
        double v = m[j];
        if (v == 100.0 && !flag) {
            m[j] = prev = ground_level;
            continue;
        }
        if (v == 100.0) v = prev;
        flag = true;
        const double next = m[j + 1];
        if (fabs(v - prev) > 0.5 && fabs(v - next) > 0.5) v = (prev + next) / 2;
        m[j] = prev = v;
    }
    // second scan (:96-105)
    double pre_th = pymin(m[0], sensor_height);
    for (int j = 1; j < L; ++j) {
        pre_th = pymin(m[j], pre_th + step);
        m[j] = pre_th;
    }
}

__global__ __launch_bounds__(kThreads) void classify_kernel(Tables t, Dims d, const float* pcl, double delta_r) {
    const int b = blockIdx.y;
    const long p = (long)blockIdx.x * kThreads + threadIdx.x;
    if (p >= (long)d.W * d.H) return;
    const int row = (int)(p / d.W), col = (int)(p % d.W);
    const int pt = t.widx[(size_t)b * d.W * d.H + (size_t)col * d.H + row];
    uint8_t lab = kEmpty;
    if (pt >= 0) {
        const float* q = pcl + ((size_t)b * d.N + pt) * d.stride;
        const double x = q[0], y = q[1], z = q[2];
        const int region = (int)((sqrt(x * x + y * y) - kMinRange) / delta_r);
        size_t ri = (size_t)col * d.L + region;
        if (ri >= (size_t)d.W * d.L) ri = (size_t)d.W * d.L - 1;
        const double th = t.minz[(size_t)b * d.W * d.L + ri];
        lab = z >= th + kThG ? kObstacle : kGround;
    }
    t.lab0[b * d.lab_stride + p] = lab;
}

// ---- stage 4 -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void candidates_kernel(Tables t, Dims d) {
    const int b = blockIdx.y;
    const long p = (long)blockIdx.x * kThreads + threadIdx.x;
    if (p >= (long)d.W * d.H) return;
    const int row = (int)(p / d.W), col = (int)(p % d.W);
    const uint8_t* in = t.lab0 + b * d.lab_stride;
    uint8_t lab = in[p];
    if (lab == kGround) {
        bool hit = false;  // 5x5 cross (cv2 MORPH_CROSS, centre anchor); outside the image counts as nothing
#pragma unroll
        for (int o = -2; o <= 2; ++o) {
            if (o == 0) continue;
            if (col + o >= 0 && col + o < d.W) hit |= in[p + o] == kObstacle;
            if (row + o >= 0 && row + o < d.H) hit |= in[p + (long)o * d.W] == kObstacle;
        }
        // the reference's transposed read: cloud_index_[row * H + col] of a table laid out col * H + row
        if (hit) lab = t.widx[(size_t)b * d.W * d.H + (size_t)row * d.H + col] != -1 ? kCandidate : kObstacle;
    }
    t.lab1[b * d.lab_stride + p] = lab;
}

// one wave per (row, cloud): the columns of the row's candidates, ascending
__global__ __launch_bounds__(64) void row_lists_kernel(Tables t, Dims d) {
    const int b = blockIdx.y, row = blockIdx.x, lane = threadIdx.x;
    const uint8_t* lab = t.lab1 + b * d.lab_stride + (size_t)row * d.W;
    int32_t* cols = t.cols + ((size_t)b * d.H + row) * d.W;
    int base = 0;
    for (int c0 = 0; c0 < d.W; c0 += 64) {
        const int c = c0 + lane;
        const bool cand = c < d.W && lab[c] == kCandidate;
        const unsigned long long mask = __ballot(cand);
        if (cand) cols[base + __popcll(mask & ((1ull << lane) - 1ull))] = c;
        base += __popcll(mask);
    }
    if (lane == 0) t.row_cnt[b * d.H + row] = base;
}

// one thread per candidate slot: D = exp(-5 |p - p_n|) for neighbours with a point within 3 m, W = D / max(sum D, 1e-6)
__global__ __launch_bounds__(kThreads) void weights_kernel(Tables t, Dims d, const float* pcl) {
    const int b = blockIdx.y;
    const long s = (long)blockIdx.x * kThreads + threadIdx.x;
    if (s >= (long)d.W * d.H) return;
    const int row = (int)(s / d.W), k = (int)(s % d.W);
    if (k >= t.row_cnt[b * d.H + row]) return;
    const int col = t.cols[(size_t)b * d.H * d.W + s];
    const int32_t* widx = t.widx + (size_t)b * d.W * d.H;
    const float* pts = pcl + (size_t)b * d.N * d.stride;
    const float* q = pts + (size_t)widx[(size_t)col * d.H + row] * d.stride;
    const double x = q[0], y = q[1], z = q[2];
    double D[kNb];
    double sum = 0.0;
#pragma unroll
    for (int i = 0; i < kNb; ++i) {
        const int w = i < 12 ? i : i + 1;
        const int ny = row + w / 5 - 2, nx = col + w % 5 - 2;
        double v = 0.0;
        if (nx >= 0 && nx < d.W && ny >= 0 && ny < d.H) {
            const int pn = widx[(size_t)nx * d.H + ny];
            if (pn != -1) {
                const float* qn = pts + (size_t)pn * d.stride;
                const double dx = x - (double)qn[0], dy = y - (double)qn[1], dz = z - (double)qn[2];
                const double dist = sqrt(dx * dx + dy * dy + dz * dz);
                if (!(dist > 3.0)) v = exp(-5.0 * dist);
            }
        }
        D[i] = v;
        sum += v;
    }
    const double den = fmax(sum, 1e-6);
    double* out = t.wts + ((size_t)b * d.H * d.W + s) * kNb;
#pragma unroll
    for (int i = 0; i < kNb; ++i) out[i] = D[i] / den;
}

// ---- stage 5 -----------------------------------------------------------------------------------------------------------------------
struct Weights {
    double w[kNb];
};

__device__ __forceinline__ void load_weights(Weights& o, const double* src) {
    const double2* s2 = (const double2*)src;  // slots are 192 B apart in a 256-B aligned table
#pragma unroll
    for (int i = 0; i < kNb / 2; ++i) {
        const double2 v = s2[i];
        o.w[2 * i] = v.x, o.w[2 * i + 1] = v.y;
    }
}

template <bool kLds>
__global__ void resolve_kernel(Tables t, Dims d) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int b = blockIdx.x, r = threadIdx.x, W = d.W, H = d.H;
    uint8_t* glab = t.lab1 + b * d.lab_stride;
    uint8_t* lab = kLds ? smem : glab;
    if (kLds) {
        const uint4* src = (const uint4*)glab;
        uint4* dst = (uint4*)smem;
        for (size_t i = threadIdx.x; i < d.lab_stride / 16; i += blockDim.x) dst[i] = src[i];
        __syncthreads();
    }
    const bool active = r < H;
    const int32_t* cols = t.cols + ((size_t)b * H + (active ? r : 0)) * W;
    const double* wts = t.wts + ((size_t)b * H + (active ? r : 0)) * W * kNb;
    const int cnt = active ? t.row_cnt[b * H + r] : 0;
    int k = 0, next_col = INT_MAX;
    Weights wt;
#pragma unroll
    for (int i = 0; i < kNb; ++i) wt.w[i] = 0.0;
    if (cnt > 0) {
        next_col = cols[0];
        load_weights(wt, wts);
    }
    const int steps = W + 3 * (H - 1);
    for (int step = 0; step < steps; ++step) {
        const int c = step - 3 * r;
        if (c == next_col) {  // implies an active lane and 0 <= c < W
            double score_r = 0.0, score_g = 0.0;
#pragma unroll
            for (int i = 0; i < kNb; ++i) {  // the reference's neighbour order: the window in raster order without its centre
                const int w = i < 12 ? i : i + 1;
                const int ny = r + w / 5 - 2, nx = c + w % 5 - 2;
                if (nx >= 0 && nx < W && ny >= 0 && ny < H) {
                    const uint8_t l = lab[ny * W + nx];
                    if (l == kObstacle) score_r += wt.w[i];
                    else if (l == kGround) score_g += wt.w[i];
                }
            }
            lab[r * W + c] = score_r > score_g ? kObstacle : kGround;
            ++k;
            if (k < cnt) {
                next_col = cols[k];
                load_weights(wt, wts + (size_t)k * kNb);
            } else {
                next_col = INT_MAX;
            }
        }
        __syncthreads();
    }
    if (kLds) {
        const uint4* src = (const uint4*)smem;
        uint4* dst = (uint4*)glab;
        for (size_t i = threadIdx.x; i < d.lab_stride / 16; i += blockDim.x) dst[i] = src[i];
    }
}

// ---- stage 6 -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void gather_kernel(Tables t, Dims d, uint8_t* is_ground) {
    const int b = blockIdx.y, i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= d.N) return;
    const int pix = t.pix[(size_t)b * d.N + i];
    uint8_t g = 0;
    if (pix >= 0) g = t.lab1[b * d.lab_stride + (size_t)(pix % d.H) * d.W + pix / d.H] == kGround;
    is_ground[(size_t)b * d.N + i] = g;
}

// ---- cone test, removal ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void cone_kernel(int N, int stride, const float* pcl, const int32_t* counts, double z_threshold,
                                                        double slope, const uint8_t* or_with, uint8_t* out) {
    const int b = blockIdx.y, i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= N) return;
    double x, y, z;
    float zf;
    uint8_t g = 0;
    if (load_point(pcl, counts, b, i, N, stride, &x, &y, &z, &zf)) {
        g = z < z_threshold + slope * sqrt(x * x + y * y);
        if (or_with) g |= or_with[(size_t)b * N + i] != 0;
    }
    out[(size_t)b * N + i] = g;
}

__global__ __launch_bounds__(kThreads) void keep_flags_kernel(int N, int stride, const float* pcl, const int32_t* counts,
                                                              const uint8_t* drop, int32_t* flags) {
    const int b = blockIdx.y, i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= N) return;
    double x, y, z;
    float zf;
    const bool valid = load_point(pcl, counts, b, i, N, stride, &x, &y, &z, &zf);
    flags[(size_t)b * N + i] = valid && drop[(size_t)b * N + i] == 0;
}

__global__ __launch_bounds__(kThreads) void compact_kernel(int N, int stride, const float* pcl, const int32_t* flags, const int32_t* pos,
                                                           float* out, int32_t* out_counts) {
    const int b = blockIdx.y, i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= N) return;
    const int32_t* ps = pos + (size_t)b * N;
    const int total = ps[N - 1];
    if (i == 0) out_counts[b] = total;
    if (flags[(size_t)b * N + i]) {
        const float* src = pcl + ((size_t)b * N + i) * stride;
        float* dst = out + ((size_t)b * N + ps[i] - 1) * stride;
        for (int c = 0; c < stride; ++c) dst[c] = src[c];
    }
    if (i >= total) {
        float* dst = out + ((size_t)b * N + i) * stride;
        for (int c = 0; c < stride; ++c) dst[c] = NAN;
    }
}

liso_dev::PerDeviceFlag g_resolve_lds;

}  // namespace

extern "C" {

size_t liso_ground_jcp_workspace_bytes(const liso_ground_cfg* cfg) {
    Dims d;
    if (read_cfg(cfg, &d) != LISO_OK) return 0;
    return carve(d, nullptr).bytes;
}

int liso_ground_jcp_workspace_layout(const liso_ground_cfg* cfg, size_t* offsets) {
    Dims d;
    if (read_cfg(cfg, &d) != LISO_OK || !offsets) return LISO_EINVAL;
    const Tables t = carve(d, nullptr);
    const void* at[LISO_GROUND_N_LAYOUT] = {t.ele_key, t.ele, t.pix, t.widx, t.minz_key, t.minz, t.lab0, t.lab1, t.row_cnt, t.cols, t.wts};
    for (int i = 0; i < LISO_GROUND_N_LAYOUT; ++i) offsets[i] = (size_t)(uintptr_t)at[i];
    return LISO_OK;
}

int liso_ground_jcp_stages_f32(const liso_ground_cfg* cfg, const float* pcl, const int32_t* counts, uint8_t* is_ground,
                               void* workspace, size_t workspace_bytes, int stage_begin, int stage_end, void* stream) {
    Dims d;
    const int rc = read_cfg(cfg, &d);
    if (rc != LISO_OK) return rc;
    if (stage_begin < 0 || stage_end > LISO_GROUND_N_STAGES || stage_begin > stage_end) return LISO_EINVAL;
    if (d.N == 0) return (pcl || is_ground) ? LISO_EINVAL : LISO_OK;
    if (!pcl || !is_ground || !workspace) return LISO_EINVAL;
    if (((uintptr_t)workspace & 255) != 0) return LISO_EINVAL;
    const Tables t = carve(d, workspace);
    if (workspace_bytes < t.bytes) return LISO_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const dim3 pts((unsigned)((d.N + kThreads - 1) / kThreads), d.B);
    const size_t WH = (size_t)d.W * d.H, WL = (size_t)d.W * d.L;
    const dim3 pixels((unsigned)((WH + kThreads - 1) / kThreads), d.B);
    const bool lds = d.lab_stride <= (size_t)LISO_GROUND_LDS_BYTES;
    if (lds && d.lab_stride > 64 * 1024 &&
        !liso_dev::lds_opt_in(g_resolve_lds, (const void*)resolve_kernel<true>, LISO_GROUND_LDS_BYTES))
        return LISO_ELAUNCH;
    for (int s = stage_begin; s < stage_end; ++s) {
        switch (s) {
        case 0: {
            const size_t most = d.B * (WH > WL ? WH : WL);
            init_kernel<<<(unsigned)((most + kThreads * 4 - 1) / (kThreads * 4)), kThreads, 0, st>>>(t, d.B * WH, d.B * WL, d.B);
            break;
        }
        case 1:
            elevation_kernel<<<pts, kThreads, 0, st>>>(t, d, pcl, counts);
            break;
        case 2:
            project_kernel<<<pts, kThreads, 0, st>>>(t, d, pcl, counts, cfg->delta_r);
            break;
        case 3:
            // sensor_height + th_g and delta_R * tan(sigma) are formed on the host as the reference forms them
            recm_kernel<<<dim3((unsigned)((d.W + 63) / 64), d.B), 64, 0, st>>>(t, d, cfg->sensor_height + kThG, cfg->sensor_height,
                                                                              cfg->delta_r * tan(kSigmaDeg * M_PI / 180));
            classify_kernel<<<pixels, kThreads, 0, st>>>(t, d, pcl, cfg->delta_r);
            break;
        case 4:
            candidates_kernel<<<pixels, kThreads, 0, st>>>(t, d);
            row_lists_kernel<<<dim3(d.H, d.B), 64, 0, st>>>(t, d);
            weights_kernel<<<pixels, kThreads, 0, st>>>(t, d, pcl);
            break;
        case 5: {
            const unsigned threads = (unsigned)((d.H + 63) / 64 * 64);
            if (lds) resolve_kernel<true><<<d.B, threads, d.lab_stride, st>>>(t, d);
            else resolve_kernel<false><<<d.B, threads, 0, st>>>(t, d);
            break;
        }
        default:
            gather_kernel<<<pts, kThreads, 0, st>>>(t, d, is_ground);
            break;
        }
    }
    return check_launch();
}

int liso_ground_jcp_f32(const liso_ground_cfg* cfg, const float* pcl, const int32_t* counts, uint8_t* is_ground, void* workspace,
                        size_t workspace_bytes, void* stream) {
    return liso_ground_jcp_stages_f32(cfg, pcl, counts, is_ground, workspace, workspace_bytes, 0, LISO_GROUND_N_STAGES, stream);
}

int liso_ground_cone_f32(int batch, int n_max, int point_stride, const float* pcl, const int32_t* counts, double z_threshold,
                         double slope, const uint8_t* or_with, uint8_t* out, void* stream) {
    if (batch < 1 || n_max < 0 || n_max > LISO_GROUND_MAX_N || point_stride < 3) return LISO_EINVAL;
    if (!isfinite(z_threshold) || !isfinite(slope)) return LISO_EINVAL;
    if (n_max == 0) return (pcl || out || or_with) ? LISO_EINVAL : LISO_OK;
    if (!pcl || !out) return LISO_EINVAL;
    cone_kernel<<<dim3((unsigned)((n_max + kThreads - 1) / kThreads), batch), kThreads, 0, (hipStream_t)stream>>>(
        n_max, point_stride, pcl, counts, z_threshold, slope, or_with, out);
    return check_launch();
}

size_t liso_ground_compact_workspace_bytes(int batch, int n_max) {
    if (batch < 1 || n_max < 1 || n_max > LISO_GROUND_MAX_N) return 0;
    return 2 * up256((size_t)batch * n_max * sizeof(int32_t)) + up256(liso_scan_workspace_bytes(batch, n_max));
}

int liso_ground_compact_f32(int batch, int n_max, int point_stride, const float* pcl, const int32_t* counts, const uint8_t* drop,
                            float* out, int32_t* out_counts, void* workspace, size_t workspace_bytes, void* stream) {
    if (batch < 1 || n_max < 0 || n_max > LISO_GROUND_MAX_N || point_stride < 3 || !out_counts) return LISO_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (n_max == 0) {
        if (pcl || drop || out) return LISO_EINVAL;
        return hipMemsetAsync(out_counts, 0, sizeof(int32_t) * batch, st) == hipSuccess ? LISO_OK : LISO_ELAUNCH;
    }
    if (!pcl || !drop || !out || !workspace || pcl == out) return LISO_EINVAL;
    if (workspace_bytes < liso_ground_compact_workspace_bytes(batch, n_max)) return LISO_EWORKSPACE;
    const size_t table = up256((size_t)batch * n_max * sizeof(int32_t));
    int32_t* flags = (int32_t*)workspace;
    int32_t* pos = (int32_t*)((char*)workspace + table);
    void* scan_ws = (char*)workspace + 2 * table;
    const dim3 pts((unsigned)((n_max + kThreads - 1) / kThreads), batch);
    keep_flags_kernel<<<pts, kThreads, 0, st>>>(n_max, point_stride, pcl, counts, drop, flags);
    const int rc = liso_scan_inclusive_i32(flags, batch, n_max, pos, scan_ws, liso_scan_workspace_bytes(batch, n_max), st);
    if (rc != LISO_OK) return rc;
    compact_kernel<<<pts, kThreads, 0, st>>>(n_max, point_stride, pcl, flags, pos, out, out_counts);
    return check_launch();
}

}  // extern "C"
