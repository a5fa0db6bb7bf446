// Per-point ground truth from annotated, tracked boxes on gfx950: scene flow, track id, box slot and the boxes' point counts for
// many directed sweep pairs in one call, and KITTI's lidar rows and columns.  C ABI and semantics: include/liso_flow_labels.h.
// Compiled without FMA contraction: every expression is the header's expression, operation by operation.
//
// Flow labels: a small launch (one thread per box, one per job) builds A = rinv(pose_a), D = pose_b A - I, the half extents and
// the fp32 sphere of every box and S of every job into the workspace, and zeroes the counts.  The point launch has one block per
// (job, tile of 256 points); the job's boxes pass through LDS in chunks (A, half extents, sphere, label and class: 152 B a
// box), every thread runs the sphere reject and, behind it, the fp64 test.  Only the slot of the flow winner is kept while the
// boxes pass; its D is read from the workspace once the loop is over, so D never occupies LDS.  Counts go through an LDS
// counter per resident box (touched on a hit only) and one global atomic per box and block that saw a hit.
// Rows and columns: one block of 1024 threads per cloud walks its rows in tiles, a ballot and a prefix over the sixteen waves
// give every row its jump count, the running sum rides along.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "../../include/liso_flow_labels.h"
#include "dev_common.h"

namespace {

using liso_dev::Carver;
using liso_dev::check_launch;
using liso_dev::cloud_rows;

constexpr int kThreads = 256;
constexpr int kChunk = LISO_FLOW_LABELS_CHUNK;
constexpr int kGeo = 15;  // doubles of a box in LDS: A (3 x 4), half extents
constexpr int kDyn = 12;  // doubles of D, and of S
constexpr int kScanThreads = 1024;
constexpr int kScanWaves = kScanThreads / 64;

struct __align__(16) BoxPre {  // 32 B, moved as two 16-byte words: the sphere first, so the reject reads one of them
    float cx, cy, cz, r2;
    int label, cls, has_b, pad;
};

struct Workspace {
    double* geo;  // [J*K, 15]
    BoxPre* pre;  // [J*K]
    double* dyn;  // [J*K, 12]
    double* odo;  // [J, 12]
    size_t bytes;
};

Workspace carve(void* base, int J, int K) {
    Carver c{base};
    Workspace w;
    const size_t boxes = (size_t)J * K;
    w.geo = c.take<double>(boxes * kGeo);
    w.pre = c.take<BoxPre>(boxes);
    w.dyn = c.take<double>(boxes * kDyn);
    w.odo = c.take<double>((size_t)J * kDyn);
    w.bytes = c.bytes;
    return w;
}

bool sizes_ok(int J, int K) {
    return J >= 1 && J <= LISO_FLOW_LABELS_MAX_JOBS && K >= 0 && K <= LISO_FLOW_LABELS_MAX_BOXES && (size_t)J * K <= ((size_t)1 << 24);
}

// rows 0..2 of rinv(M) = [R^T | -R^T t] of a rigid 4x4 row-major pose
__device__ __forceinline__ void rigid_inv(const double* M, double* R) {
    for (int r = 0; r < 3; ++r) {
        R[4 * r] = M[r], R[4 * r + 1] = M[4 + r], R[4 * r + 2] = M[8 + r];
        R[4 * r + 3] = -((M[r] * M[3] + M[4 + r] * M[7]) + M[8 + r] * M[11]);
    }
}

// ---- launch 1: the per-box and per-job matrices ------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void flow_boxes_kernel(int J, int K, const double* __restrict__ odom, const double* __restrict__ pose_a,
                                                        const double* __restrict__ pose_b, const double* __restrict__ size,
                                                        const uint8_t* __restrict__ valid, const uint8_t* __restrict__ has_b,
                                                        const int32_t* __restrict__ label, const int32_t* __restrict__ box_class,
                                                        double* __restrict__ geo, BoxPre* __restrict__ pre, double* __restrict__ dyn,
                                                        double* __restrict__ odo, int32_t* __restrict__ count) {
    const size_t t = (size_t)blockIdx.x * 64 + threadIdx.x, boxes = (size_t)J * K;
    if (t >= boxes + (size_t)J) return;
    if (t >= boxes) {  // S of job t - boxes
        const size_t j = t - boxes;
        double S[12];
        rigid_inv(odom + j * 16, S);
        S[0] = S[0] - 1.0, S[5] = S[5] - 1.0, S[10] = S[10] - 1.0;
        for (int q = 0; q < 12; ++q) odo[j * kDyn + q] = S[q];
        return;
    }
    const double* Pa = pose_a + t * 16;
    const double* Pb = pose_b + t * 16;
    double A[12], D[12];
    rigid_inv(Pa, A);
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c)
            D[4 * r + c] = ((Pb[4 * r] * A[c] + Pb[4 * r + 1] * A[4 + c]) + Pb[4 * r + 2] * A[8 + c]) - (r == c ? 1.0 : 0.0);
        D[4 * r + 3] = ((Pb[4 * r] * A[3] + Pb[4 * r + 1] * A[7]) + Pb[4 * r + 2] * A[11]) + Pb[4 * r + 3];
    }
    const double hx = size[t * 3] / 2.0, hy = size[t * 3 + 1] / 2.0, hz = size[t * 3 + 2] / 2.0;
    for (int q = 0; q < 12; ++q) geo[t * kGeo + q] = A[q], dyn[t * kDyn + q] = D[q];
    geo[t * kGeo + 12] = hx, geo[t * kGeo + 13] = hy, geo[t * kGeo + 14] = hz;
    BoxPre p;
    p.cx = (float)Pa[3], p.cy = (float)Pa[7], p.cz = (float)Pa[11];
    // inside => |p - t|^2 < hx^2 + hy^2 + hz^2 for a rigid pose; the margin covers the fp32 rounding of the centre and of the squared
    // distance at |t|, |p| <= 1e4 m.  An empty slot gets a negative radius, a NaN box a NaN one: no distance is below either.
    p.r2 = valid[t] ? (float)(((hx * hx + hy * hy) + hz * hz) * 1.001 + 0.05) : -1.0f;
    p.label = label[t];
    p.cls = box_class ? box_class[t] : -1;
    p.has_b = has_b[t] ? 1 : 0;
    p.pad = 0;
    pre[t] = p;
    if (count) count[t] = 0;
}

// ---- launch 2: the points -----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float apply_row(const double* M, double x, double y, double z) {
    return (float)(((M[0] * x + M[1] * y) + M[2] * z) + M[3]);
}

__global__ __launch_bounds__(kThreads) void flow_points_kernel(liso_flow_labels_cfg c, const float* __restrict__ pcl,
                                                               const int32_t* __restrict__ counts, const int32_t* __restrict__ cloud_of,
                                                               const double* __restrict__ geo, const BoxPre* __restrict__ pre,
                                                               const double* __restrict__ dyn, const double* __restrict__ odo,
                                                               const int32_t* __restrict__ point_class, float* flow,
                                                               int32_t* __restrict__ point_label, int32_t* __restrict__ point_box,
                                                               int32_t* __restrict__ count) {
    __shared__ double s_geo[kChunk * kGeo];
    __shared__ BoxPre s_pre[kChunk];
    __shared__ int s_cnt[kChunk];
    const int j = blockIdx.y, N = c.n_max, K = c.n_boxes, tile = blockIdx.x * kThreads, i = tile + threadIdx.x;
    const int cloud = cloud_of[j];
    const int rows = (cloud >= 0 && cloud < c.n_clouds) ? cloud_rows(counts, cloud, N) : 0;
    const bool in_row = i < N;
    const size_t out = (size_t)j * N + (in_row ? i : 0);
    float px = NAN, py = NAN, pz = NAN;  // a NaN point is in no sphere
    int pc = 0;
    bool live = false;
    if (i < rows) {
        const size_t at = (size_t)cloud * N + i;
        const float* p = pcl + at * c.point_stride;
        const float x = p[0], y = p[1], z = p[2];
        live = isfinite(x) && isfinite(y) && isfinite(z);
        if (live) {
            px = x, py = y, pz = z;
            if (point_class) pc = point_class[at];
        }
    }
    const bool last = c.overlap == LISO_OVERLAP_LAST;
    int label_box = -1, label_val = c.no_label, flow_box = -1;
    if (tile < rows) {  // (uniform per block: a tile behind the count has nothing to test)
        const double x = px, y = py, z = pz;
        for (int k0 = 0; k0 < K; k0 += kChunk) {
            const int n = min(kChunk, K - k0);
            const size_t base = (size_t)j * K + k0;
            __syncthreads();  // the previous chunk has been read and its counts flushed
            for (int q = threadIdx.x; q < n * kGeo; q += kThreads) s_geo[q] = geo[base * kGeo + q];
            for (int q = threadIdx.x; q < n * 2; q += kThreads) ((uint4*)s_pre)[q] = ((const uint4*)(pre + base))[q];
            for (int q = threadIdx.x; q < n; q += kThreads) s_cnt[q] = 0;
            __syncthreads();
            for (int q = 0; q < n; ++q) {
                const BoxPre& b = s_pre[q];
                const float dx = px - b.cx, dy = py - b.cy, dz = pz - b.cz;
                if (!((dx * dx + dy * dy) + dz * dz < b.r2)) continue;
                const double* A = s_geo + q * kGeo;
                const double u = ((A[0] * x + A[1] * y) + A[2] * z) + A[3];
                const double v = ((A[4] * x + A[5] * y) + A[6] * z) + A[7];
                const double w = ((A[8] * x + A[9] * y) + A[10] * z) + A[11];
                if (!(fabs(u) < A[12] && fabs(v) < A[13] && fabs(w) < A[14])) continue;
                if (count) atomicAdd(&s_cnt[q], 1);
                if (b.cls >= 0 && pc != b.cls) continue;
                if (last || label_box < 0) label_box = k0 + q, label_val = b.label;
                if (b.has_b && (last || flow_box < 0)) flow_box = k0 + q;
            }
            if (count) {
                __syncthreads();
                for (int q = threadIdx.x; q < n; q += kThreads)
                    if (s_cnt[q] != 0) atomicAdd(&count[base + q], s_cnt[q]);
            }
        }
    }
    if (!in_row) return;
    if (point_label) point_label[out] = label_val;
    if (point_box) point_box[out] = label_box;
    float* f = flow + out * 3;
    if (!live) {
        f[0] = NAN, f[1] = NAN, f[2] = NAN;
        return;
    }
    const double* M = flow_box >= 0 ? dyn + ((size_t)j * K + flow_box) * kDyn : odo + (size_t)j * kDyn;
    if (flow_box < 0 && c.keep_flow) return;
    const double x = px, y = py, z = pz;
    f[0] = apply_row(M, x, y, z), f[1] = apply_row(M + 4, x, y, z), f[2] = apply_row(M + 8, x, y, z);
}

// ---- rows and columns ---------------------------------------------------------------------------------------------------------------
// numpy's astype(int32) of a float32: truncation, INT_MIN for NaN and for values outside int32
__device__ __forceinline__ int f32_to_i32(float v) { return (v > -2147483904.0f && v < 2147483648.0f) ? (int)v : INT_MIN; }

__global__ __launch_bounds__(kScanThreads) void rows_cols_kernel(int N, int stride, const float* __restrict__ pcl,
                                                                 const int32_t* __restrict__ counts, float threshold, int auto_correct,
                                                                 float columns_minus_1, int32_t* __restrict__ rows,
                                                                 int32_t* __restrict__ cols) {
    __shared__ float s_az[kScanThreads];
    __shared__ int s_wave[kScanWaves];
    const int b = blockIdx.x, n = cloud_rows(counts, b, N), lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t row0 = (size_t)b * N;
    const float pi = (float)3.141592653589793, two_pi = (float)(2.0 * 3.141592653589793);
    int running = 0;       // jumps of the tiles before this one (the same in every thread)
    float carried = 0.0f;  // the azimuth of the last row of the tile before this one
    for (int t0 = 0; t0 < n; t0 += kScanThreads) {
        const int i = t0 + threadIdx.x;
        const bool live = i < n;
        float az = 0.0f;
        if (live) {
            const float* p = pcl + (row0 + i) * stride;
            const double x = p[0], y = p[1];
            az = -(float)atan2(y, -x);
            if (cols) cols[row0 + i] = f32_to_i32((columns_minus_1 * (pi - (float)atan2(y, x))) / two_pi);
        }
        s_az[threadIdx.x] = az;
        __syncthreads();
        const float before = threadIdx.x > 0 ? s_az[threadIdx.x - 1] : carried;
        const bool jump = live && i >= 1 && (az - before) < threshold;
        const unsigned long long jumps = __ballot(jump);
        if (lane == 0) s_wave[wave] = __popcll(jumps);
        __syncthreads();
        int mine = running, total = running;
        for (int w = 0; w < kScanWaves; ++w) {
            if (w < wave) mine += s_wave[w];
            total += s_wave[w];
        }
        mine += __popcll(jumps & (~0ull >> (63 - lane)));  // inclusive within the wave
        if (live && rows) rows[row0 + i] = mine;
        carried = s_az[kScanThreads - 1];
        running = total;
        __syncthreads();  // s_az and s_wave have been read before the next tile writes them
    }
    if (rows && auto_correct && n > 0 && running < 63) {
        const int add = 63 - running;  // every thread revisits the rows it wrote itself
        for (int i = threadIdx.x; i < n; i += kScanThreads) rows[row0 + i] += add;
    }
    for (int i = n + threadIdx.x; i < N; i += kScanThreads) {
        if (rows) rows[row0 + i] = -1;
        if (cols) cols[row0 + i] = -1;
    }
}

}  // namespace

extern "C" size_t liso_flow_labels_workspace_bytes(int n_jobs, int n_boxes) {
    return sizes_ok(n_jobs, n_boxes) ? carve(nullptr, n_jobs, n_boxes).bytes : 0;
}

extern "C" int liso_flow_labels_f32(const liso_flow_labels_cfg* cfg, const float* pcl, const int32_t* counts, const int32_t* cloud_of,
                                    const double* odom, const double* pose_a, const double* pose_b, const double* size,
                                    const uint8_t* valid, const uint8_t* has_b, const int32_t* label, const int32_t* box_class,
                                    const int32_t* point_class, float* flow, int32_t* point_label, int32_t* point_box, int32_t* count,
                                    void* workspace, size_t workspace_bytes, void* stream) {
    if (!cfg || !sizes_ok(cfg->n_jobs, cfg->n_boxes)) return LISO_EINVAL;
    const int J = cfg->n_jobs, K = cfg->n_boxes, N = cfg->n_max;
    if (cfg->n_clouds < 1 || cfg->n_clouds > LISO_FLOW_LABELS_MAX_JOBS || N < 0 || N > LISO_FLOW_LABELS_MAX_N || cfg->point_stride < 3)
        return LISO_EINVAL;
    if (cfg->overlap != LISO_OVERLAP_LAST && cfg->overlap != LISO_OVERLAP_FIRST) return LISO_EINVAL;
    if (!cloud_of || !odom || (N > 0 && (!pcl || !flow))) return LISO_EINVAL;
    if (K > 0 && (!pose_a || !pose_b || !size || !valid || !has_b || !label)) return LISO_EINVAL;
    if ((box_class == nullptr) != (point_class == nullptr)) return LISO_EINVAL;
    const Workspace w = carve(workspace, J, K);
    if (!workspace || ((uintptr_t)workspace & 255) != 0 || workspace_bytes < w.bytes) return LISO_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const size_t prep = (size_t)J * K + (size_t)J;
    hipLaunchKernelGGL(flow_boxes_kernel, dim3((unsigned)((prep + 63) / 64)), dim3(64), 0, st, J, K, odom, pose_a, pose_b, size, valid, has_b,
                       label, box_class, w.geo, w.pre, w.dyn, w.odo, count);
    if (check_launch() != LISO_OK) return LISO_ELAUNCH;
    if (N == 0) return LISO_OK;
    hipLaunchKernelGGL(flow_points_kernel, dim3((unsigned)((N + kThreads - 1) / kThreads), (unsigned)J), dim3(kThreads), 0, st, *cfg, pcl,
                       counts, cloud_of, (const double*)w.geo, (const BoxPre*)w.pre, (const double*)w.dyn, (const double*)w.odo, point_class,
                       flow, point_label, point_box, count);
    return check_launch();
}

extern "C" int liso_kitti_rows_cols_f32(int batch, int n_max, int point_stride, const float* pcl, const int32_t* counts, double threshold,
                                        int auto_correct, int num_columns, int32_t* rows, int32_t* cols, void* stream) {
    if (batch < 1 || batch > LISO_FLOW_LABELS_MAX_JOBS || n_max < 0 || n_max > LISO_FLOW_LABELS_MAX_N || point_stride < 3) return LISO_EINVAL;
    if (!(threshold == threshold) || num_columns < 1 || (!rows && !cols)) return LISO_EINVAL;
    if (n_max == 0) return LISO_OK;
    if (!pcl) return LISO_EINVAL;
    hipLaunchKernelGGL(rows_cols_kernel, dim3((unsigned)batch), dim3(kScanThreads), 0, (hipStream_t)stream, n_max, point_stride, pcl, counts,
                       (float)threshold, auto_correct, (float)(num_columns - 1), rows, cols);
    return check_launch();
}
