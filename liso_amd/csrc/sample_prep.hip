// Geometric sample augmentation, the BEV crop with its compaction, and the BEV point maps on gfx950.  C ABI and semantics:
// include/liso_sample_prep.h.  Compiled without FMA contraction: every expression is the header's fp64 expression, operation by
// operation.
//
// Crop: flags (reads x, y, z and drop) -> liso_scan_inclusive_i32 -> move.  The move kernel reads every input row once, computes
// the pillar coordinates from the row it holds and writes every output array, paddings included; no pass per attribute.
//
// Flow mean: integer atomics only, so the result does not depend on the order in which they retire.  Pass A finds per cell and
// component the largest |v| (the bits of a non-negative float order like an unsigned integer) and counts the points; pass B
// rounds every value to a multiple of 2^(E-38), E the exponent of that maximum, and adds it to an int64 (|q| <= 2^39, at most
// 2^24 points per cloud: no overflow); the finalize pass divides in fp64 and rounds once.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "../../include/liso_box_mining.h"
#include "../../include/liso_sample_prep.h"
#include "dev_common.h"
#include "zero_fill.h"

namespace {

using liso_dev::Carver;
using liso_dev::affine_inv;
using liso_dev::check_launch;
using liso_dev::cloud_rows;
using liso_dev::mat4_mul;
using liso_dev::to_i32;
using liso_dev::up256;

constexpr int kThreads = 256;
constexpr int kFixedBits = 38;


// ---- 1. transform -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void transform_kernel(int N, int stride, const double* T, const float* pcl, const int32_t* counts,
                                                             const float* flow, float* out_pcl, float* out_flow) {
    const int b = blockIdx.y, i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= N) return;
    const size_t row = (size_t)b * N + i;
    const float* src = pcl + row * stride;
    float* dst = out_pcl + row * stride;
    if (i >= cloud_rows(counts, b, N)) {
        for (int c = 0; c < stride; ++c) dst[c] = NAN;
        if (flow) out_flow[row * 3 + 0] = NAN, out_flow[row * 3 + 1] = NAN, out_flow[row * 3 + 2] = NAN;
        return;
    }
    const double* t = T + (size_t)b * 16;
    const float xf = src[0], yf = src[1], zf = src[2];
    const bool valid = !(isnan(xf) || isnan(yf) || isnan(zf));
    const double x = xf, y = yf, z = zf;
    float o[3];
    for (int r = 0; r < 3; ++r) o[r] = valid ? (float)(((t[4 * r] * x + t[4 * r + 1] * y) + t[4 * r + 2] * z) + t[4 * r + 3]) : NAN;
    if (dst != src)
        for (int c = 3; c < stride; ++c) dst[c] = src[c];
    dst[0] = o[0], dst[1] = o[1], dst[2] = o[2];
    if (flow) {
        const double fx = flow[row * 3], fy = flow[row * 3 + 1], fz = flow[row * 3 + 2];
        for (int r = 0; r < 3; ++r) o[r] = valid ? (float)((t[4 * r] * fx + t[4 * r + 1] * fy) + t[4 * r + 2] * fz) : NAN;
        out_flow[row * 3] = o[0], out_flow[row * 3 + 1] = o[1], out_flow[row * 3 + 2] = o[2];
    }
}

// ---- 2. poses -----------------------------------------------------------------------------------------------------------------
struct PoseJobs {
    liso_sample_box_job box[LISO_SAMPLE_MAX_JOBS];
    liso_sample_odom_job odom[LISO_SAMPLE_MAX_JOBS];
    int n_boxes, n_odoms;
};

// blockIdx.y = job (boxes first, then odometries), blockIdx.z = b
__global__ __launch_bounds__(kThreads) void poses_kernel(PoseJobs jobs, const double* T) {
    const int j = blockIdx.y, b = blockIdx.z;
    const double* t = T + (size_t)b * 16;
    if (j < jobs.n_boxes) {
        const liso_sample_box_job& q = jobs.box[j];
        const int i = blockIdx.x * kThreads + threadIdx.x;
        if (i >= q.k) return;
        const size_t at = (size_t)b * q.k + i;
        if (q.valid && !q.valid[at]) return;
        double p[3] = {0.0, 0.0, 0.0}, yaw;
        if (q.is_f64) {
            for (int c = 0; c < q.pos_dim; ++c) p[c] = ((const double*)q.pos)[at * q.pos_dim + c];
            yaw = ((const double*)q.rot)[at];
        } else {
            for (int c = 0; c < q.pos_dim; ++c) p[c] = ((const float*)q.pos)[at * q.pos_dim + c];
            yaw = ((const float*)q.rot)[at];
        }
        const double cs = cos(yaw), sn = sin(yaw);
        double o[3];
        // T * pose as the reference's fp64 matrix product rounds it: a fused multiply-add chain along the row, left to right
        // (bit-identical to it on the fixture's boxes; the unfused order is up to 2 ulp away where the terms cancel)
        for (int r = 0; r < 3; ++r) o[r] = fma(t[4 * r + 3], 1.0, fma(t[4 * r + 2], p[2], fma(t[4 * r + 1], p[1], t[4 * r] * p[0])));
        // first column of T * pose: the pose's first column is (cos, sin, 0, 0)
        const double yaw_new = atan2(fma(t[5], sn, t[4] * cs), fma(t[1], sn, t[0] * cs));
        if (q.is_f64) {
            for (int c = 0; c < q.pos_dim; ++c) ((double*)q.pos)[at * q.pos_dim + c] = o[c];
            ((double*)q.rot)[at] = yaw_new;
        } else {
            for (int c = 0; c < q.pos_dim; ++c) ((float*)q.pos)[at * q.pos_dim + c] = (float)o[c];
            ((float*)q.rot)[at] = (float)yaw_new;
        }
        return;
    }
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const liso_sample_odom_job& q = jobs.odom[j - jobs.n_boxes];
    double Tm[16], O[16], Ti[16], A[16], R[16];
    for (int c = 0; c < 16; ++c) Tm[c] = t[c], O[c] = q.in[(size_t)b * 16 + c];
    affine_inv(Tm, Ti);
    mat4_mul(Tm, O, A);
    mat4_mul(A, Ti, R);
    for (int c = 0; c < 16; ++c) q.out[(size_t)b * 16 + c] = R[c];
    if (q.out_inv) {
        affine_inv(R, A);
        for (int c = 0; c < 16; ++c) q.out_inv[(size_t)b * 16 + c] = A[c];
    }
}

// ---- 3. crop ------------------------------------------------------------------------------------------------------------------
struct Crop {
    int N, stride, gx, gy;
    double rx, ry, zlo, zhi;
};

// pillar coordinates of a row and whether it is inside
__device__ __forceinline__ bool pillar_of(const Crop& c, float xf, float yf, float zf, int* cx, int* cy) {
    if (isnan(xf) || isnan(yf) || isnan(zf)) return false;
    const double x = xf, y = yf, z = zf;
    const int ix = to_i32(((x + 0.5 * c.rx) / c.rx) * (double)c.gx);
    const int iy = to_i32(((y + 0.5 * c.ry) / c.ry) * (double)c.gy);
    const int iz = to_i32(((z + 0.5 * 1000.0) / 1000.0) * 1.0);
    *cx = ix, *cy = iy;
    return 0 <= ix && 0 <= iy && 0 <= iz && ix < c.gx && iy < c.gy && iz < 1 && c.zlo < z && z < c.zhi;
}

__global__ __launch_bounds__(kThreads) void crop_flags_kernel(Crop c, const float* pcl, const int32_t* counts, const uint8_t* drop,
                                                              int32_t* flags) {
    const int b = blockIdx.y, i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= c.N) return;
    const size_t row = (size_t)b * c.N + i;
    int keep = 0;
    if (i < cloud_rows(counts, b, c.N) && !(drop && drop[row])) {
        const float* p = pcl + row * c.stride;
        int cx, cy;
        keep = pillar_of(c, p[0], p[1], p[2], &cx, &cy) ? 1 : 0;
    }
    flags[row] = keep;
}

__global__ __launch_bounds__(kThreads) void crop_move_kernel(Crop c, const float* pcl, const float* flow, const int32_t* lidar_rows,
                                                             const uint8_t* attr, const int32_t* flags, const int32_t* pos, float* out_pcl,
                                                             float* out_flow, int32_t* out_lidar_rows, uint8_t* out_attr, int32_t* coors,
                                                             int32_t* out_counts) {
    const int b = blockIdx.y, i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= c.N) return;
    const size_t base = (size_t)b * c.N, row = base + i;
    const int total = pos[base + c.N - 1];
    if (i == 0) out_counts[b] = total;
    if (flags[row]) {
        const size_t to = base + pos[row] - 1;
        const float* src = pcl + row * c.stride;
        float* dst = out_pcl + to * c.stride;
        int cx = 0, cy = 0;
        pillar_of(c, src[0], src[1], src[2], &cx, &cy);
        for (int k = 0; k < c.stride; ++k) dst[k] = src[k];
        coors[to * 2] = cx, coors[to * 2 + 1] = cy;
        if (flow) out_flow[to * 3] = flow[row * 3], out_flow[to * 3 + 1] = flow[row * 3 + 1], out_flow[to * 3 + 2] = flow[row * 3 + 2];
        if (lidar_rows) out_lidar_rows[to] = lidar_rows[row];
        if (attr) out_attr[to] = attr[row];
    }
    if (i >= total) {
        float* dst = out_pcl + row * c.stride;
        for (int k = 0; k < c.stride; ++k) dst[k] = NAN;
        coors[row * 2] = -1, coors[row * 2 + 1] = -1;
        if (flow) out_flow[row * 3] = NAN, out_flow[row * 3 + 1] = NAN, out_flow[row * 3 + 2] = NAN;
        if (lidar_rows) out_lidar_rows[row] = 0;
        if (attr) out_attr[row] = 0;
    }
}

// ---- 4. maps ------------------------------------------------------------------------------------------------------------------
struct MapTables {
    int32_t* count;            // [B*cells]
    uint32_t* maxbits[2];      // [B*cells][3] bits of the largest |v|
    unsigned long long* sum[2];  // [B*cells][3] int64 fixed-point sums (two's complement)
    size_t bytes;
};

MapTables carve_maps(size_t cells_total, int n_flows, void* base) {
    MapTables t;
    Carver ws{base};
    t.count = ws.take<int32_t>(cells_total);
    for (int s = 0; s < 2; ++s) {
        t.maxbits[s] = s < n_flows ? ws.take<uint32_t>(cells_total * 3) : nullptr;
        t.sum[s] = s < n_flows ? ws.take<unsigned long long>(cells_total * 3) : nullptr;
    }
    t.bytes = ws.bytes;
    return t;
}

struct Maps {
    int N, stride, gx, gy;
};

// the cell of a compacted row, or -1
__device__ __forceinline__ long cell_of(const Maps& m, const int32_t* counts, const int32_t* coors, int b, int i) {
    if (i >= cloud_rows(counts, b, m.N)) return -1;
    const size_t row = (size_t)b * m.N + i;
    const int cx = coors[row * 2], cy = coors[row * 2 + 1];
    if (cx < 0 || cy < 0 || cx >= m.gx || cy >= m.gy) return -1;
    return ((long)b * m.gx + cx) * m.gy + cy;
}

// exponent E with |v| < 2^(E+1) for the finite float whose magnitude bits are `bits`
__device__ __forceinline__ int exponent_of(uint32_t bits) {
    const int e = (int)(bits >> 23);
    return (e == 0 ? 1 : e) - 127;
}

__global__ __launch_bounds__(kThreads) void maps_scan_kernel(Maps m, MapTables t, const float* pcl, const int32_t* counts,
                                                             const int32_t* coors, const float* flow0, const float* flow1,
                                                             const double* odom, double threshold_dt, uint8_t* moving_mask) {
    const int b = blockIdx.y, i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= m.N) return;
    const size_t row = (size_t)b * m.N + i;
    const long cell = cell_of(m, counts, coors, b, i);
    if (cell >= 0) {
        atomicAdd(&t.count[cell], 1);
        const float* fl[2] = {flow0, flow1};
        for (int s = 0; s < 2; ++s)
            if (fl[s] && t.maxbits[s])
                for (int c = 0; c < 3; ++c) atomicMax(&t.maxbits[s][cell * 3 + c], __float_as_uint(fl[s][row * 3 + c]) & 0x7FFFFFFFu);
    }
    if (moving_mask) {
        uint8_t moving = 0;
        if (i < cloud_rows(counts, b, m.N)) {
            const float* p = pcl + row * m.stride;
            const double x = p[0], y = p[1], z = p[2];
            const double* o = odom + (size_t)b * 16;
            double d[3];
            for (int r = 0; r < 3; ++r) {
                const double m0 = o[4 * r] - (r == 0 ? 1.0 : 0.0), m1 = o[4 * r + 1] - (r == 1 ? 1.0 : 0.0);
                const double m2 = o[4 * r + 2] - (r == 2 ? 1.0 : 0.0), m3 = o[4 * r + 3];
                d[r] = (((m0 * x + m1 * y) + m2 * z) + m3) - (double)flow0[row * 3 + r];
            }
            moving = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) > threshold_dt ? 1 : 0;
        }
        moving_mask[row] = moving;
    }
}

__global__ __launch_bounds__(kThreads) void maps_add_kernel(Maps m, MapTables t, const int32_t* counts, const int32_t* coors,
                                                            const float* flow0, const float* flow1) {
    const int b = blockIdx.y, i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= m.N) return;
    const long cell = cell_of(m, counts, coors, b, i);
    if (cell < 0) return;
    const size_t row = (size_t)b * m.N + i;
    const float* fl[2] = {flow0, flow1};
    for (int s = 0; s < 2; ++s) {
        if (!fl[s] || !t.sum[s]) continue;
        for (int c = 0; c < 3; ++c) {
            const uint32_t top = t.maxbits[s][cell * 3 + c];
            if (top == 0u || top >= 0x7F800000u) continue;  // all zero, or the cell holds a non-finite value
            const double q = rint(ldexp((double)fl[s][row * 3 + c], kFixedBits - exponent_of(top)));
            atomicAdd(&t.sum[s][cell * 3 + c], (unsigned long long)(long long)q);
        }
    }
}

__global__ __launch_bounds__(kThreads) void maps_finalize_kernel(size_t cells_total, MapTables t, float* occupancy, float* bev0, float* bev1) {
    const size_t cell = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (cell >= cells_total) return;
    const int n = t.count[cell];
    if (occupancy) occupancy[cell] = n > 0 ? 1.0f : 0.0f;
    float* bev[2] = {bev0, bev1};
    for (int s = 0; s < 2; ++s) {
        if (!bev[s] || !t.sum[s]) continue;
        for (int c = 0; c < 3; ++c) {
            const uint32_t top = t.maxbits[s][cell * 3 + c];
            float v = 0.0f;
            if (n > 0 && top >= 0x7F800000u) v = NAN;
            else if (n > 0 && top != 0u)
                v = (float)ldexp((double)(long long)t.sum[s][cell * 3 + c] / (double)n, exponent_of(top) - kFixedBits);
            bev[s][cell * 3 + c] = v;
        }
    }
}

bool overlap(const void* a, size_t na, const void* b, size_t nb) {
    return (const char*)a < (const char*)b + nb && (const char*)b < (const char*)a + na;
}

}  // namespace

extern "C" {

int liso_sample_transform_f32(int batch, int n_max, int point_stride, const double* T, const float* pcl, const int32_t* counts,
                              const float* flow, float* out_pcl, float* out_flow, void* stream) {
    if (batch < 1 || batch > 65535 || n_max < 0 || n_max > LISO_SAMPLE_MAX_N || point_stride < 3 || !T) return LISO_EINVAL;
    if ((flow == nullptr) != (out_flow == nullptr)) return LISO_EINVAL;
    if (n_max == 0) return (pcl || out_pcl || flow) ? LISO_EINVAL : LISO_OK;
    if (!pcl || !out_pcl) return LISO_EINVAL;
    const size_t pb = (size_t)batch * n_max * point_stride * sizeof(float), fb = (size_t)batch * n_max * 3 * sizeof(float);
    if (out_pcl != pcl && overlap(pcl, pb, out_pcl, pb)) return LISO_EINVAL;
    if (flow && out_flow != flow && overlap(flow, fb, out_flow, fb)) return LISO_EINVAL;
    transform_kernel<<<dim3((unsigned)((n_max + kThreads - 1) / kThreads), batch), kThreads, 0, (hipStream_t)stream>>>(
        n_max, point_stride, T, pcl, counts, flow, out_pcl, out_flow);
    return check_launch();
}

int liso_sample_transform_poses_f64(int batch, const double* T, const liso_sample_box_job* boxes, int n_boxes,
                                    const liso_sample_odom_job* odoms, int n_odoms, void* stream) {
    if (batch < 1 || batch > 65535 || !T || n_boxes < 0 || n_odoms < 0 || n_boxes > LISO_SAMPLE_MAX_JOBS || n_odoms > LISO_SAMPLE_MAX_JOBS)
        return LISO_EINVAL;
    if ((n_boxes && !boxes) || (n_odoms && !odoms)) return LISO_EINVAL;
    PoseJobs jobs = {};
    int k_max = 1;
    for (int j = 0; j < n_boxes; ++j) {
        const liso_sample_box_job& q = boxes[j];
        if (q.k < 0 || (q.pos_dim != 2 && q.pos_dim != 3) || (q.is_f64 != 0 && q.is_f64 != 1)) return LISO_EINVAL;
        if (q.k > 0 && (!q.pos || !q.rot)) return LISO_EINVAL;
        jobs.box[j] = q;
        if (q.k > k_max) k_max = q.k;
    }
    for (int j = 0; j < n_odoms; ++j) {
        if (!odoms[j].in || !odoms[j].out || odoms[j].out == odoms[j].out_inv || odoms[j].in == odoms[j].out_inv) return LISO_EINVAL;
        jobs.odom[j] = odoms[j];
    }
    jobs.n_boxes = n_boxes, jobs.n_odoms = n_odoms;
    if (n_boxes + n_odoms == 0) return LISO_OK;
    poses_kernel<<<dim3((unsigned)((k_max + kThreads - 1) / kThreads), n_boxes + n_odoms, batch), kThreads, 0, (hipStream_t)stream>>>(jobs, T);
    return check_launch();
}

size_t liso_bev_crop_workspace_bytes(int batch, int n_max) {
    if (batch < 1 || n_max < 1 || n_max > LISO_SAMPLE_MAX_N) return 0;
    return 2 * up256((size_t)batch * n_max * sizeof(int32_t)) + up256(liso_scan_workspace_bytes(batch, n_max));
}

int liso_bev_crop_f32(const liso_bev_crop_cfg* cfg, const float* pcl, const int32_t* counts, const uint8_t* drop, const float* flow,
                      const int32_t* lidar_rows, const uint8_t* attr, float* out_pcl, float* out_flow, int32_t* out_lidar_rows,
                      uint8_t* out_attr, int32_t* pillar_coors, int32_t* out_counts, void* workspace, size_t workspace_bytes,
                      void* stream) {
    if (!cfg || !out_counts) return LISO_EINVAL;
    const int B = cfg->batch, N = cfg->n_max;
    if (B < 1 || B > 65535 || N < 0 || N > LISO_SAMPLE_MAX_N || cfg->point_stride < 3) return LISO_EINVAL;
    if (cfg->grid_x < 1 || cfg->grid_y < 1 || (long)cfg->grid_x * cfg->grid_y > LISO_SAMPLE_MAX_CELLS) return LISO_EINVAL;
    if (!(cfg->range_x > 0.0) || !(cfg->range_y > 0.0) || !isfinite(cfg->range_x) || !isfinite(cfg->range_y)) return LISO_EINVAL;
    if (isnan(cfg->z_min) || isnan(cfg->z_max)) return LISO_EINVAL;
    if ((flow == nullptr) != (out_flow == nullptr) || (lidar_rows == nullptr) != (out_lidar_rows == nullptr) ||
        (attr == nullptr) != (out_attr == nullptr))
        return LISO_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (N == 0) {
        if (pcl || drop || flow || lidar_rows || attr || out_pcl || pillar_coors) return LISO_EINVAL;
        return liso_zero::zero_async(out_counts, (size_t)B * sizeof(int32_t), st) == hipSuccess ? LISO_OK : LISO_ELAUNCH;
    }
    if (!pcl || !out_pcl || !pillar_coors || !workspace || pcl == out_pcl || (flow && flow == out_flow)) return LISO_EINVAL;
    if (workspace_bytes < liso_bev_crop_workspace_bytes(B, N)) return LISO_EWORKSPACE;
    const size_t table = up256((size_t)B * N * sizeof(int32_t));
    int32_t* flags = (int32_t*)workspace;
    int32_t* pos = (int32_t*)((char*)workspace + table);
    void* scan_ws = (char*)workspace + 2 * table;
    const Crop c = {N, cfg->point_stride, cfg->grid_x, cfg->grid_y, cfg->range_x, cfg->range_y, cfg->z_min, cfg->z_max};
    const dim3 pts((unsigned)((N + kThreads - 1) / kThreads), B);
    crop_flags_kernel<<<pts, kThreads, 0, st>>>(c, pcl, counts, drop, flags);
    const int rc = liso_scan_inclusive_i32(flags, B, N, pos, scan_ws, liso_scan_workspace_bytes(B, N), st);
    if (rc != LISO_OK) return rc;
    crop_move_kernel<<<pts, kThreads, 0, st>>>(c, pcl, flow, lidar_rows, attr, flags, pos, out_pcl, out_flow, out_lidar_rows, out_attr,
                                               pillar_coors, out_counts);
    return check_launch();
}

size_t liso_bev_point_maps_workspace_bytes(int batch, int grid_x, int grid_y, int n_flows) {
    if (batch < 1 || grid_x < 1 || grid_y < 1 || (long)grid_x * grid_y > LISO_SAMPLE_MAX_CELLS || n_flows < 0 || n_flows > 2) return 0;
    return carve_maps((size_t)batch * grid_x * grid_y, n_flows, nullptr).bytes;
}

int liso_bev_point_maps_f32(int batch, int n_max, int point_stride, int grid_x, int grid_y, const float* pcl, const int32_t* counts,
                            const int32_t* pillar_coors, const float* flow0, const float* flow1, const double* odom_tb_ta,
                            double threshold_dt, float* occupancy, float* flow_bev0, float* flow_bev1, uint8_t* moving_mask,
                            void* workspace, size_t workspace_bytes, void* stream) {
    if (batch < 1 || batch > 65535 || n_max < 0 || n_max > LISO_SAMPLE_MAX_N || point_stride < 3) return LISO_EINVAL;
    if (grid_x < 1 || grid_y < 1 || (long)grid_x * grid_y > LISO_SAMPLE_MAX_CELLS) return LISO_EINVAL;
    if (flow_bev1 && !flow_bev0) return LISO_EINVAL;
    if (n_max > 0 && ((flow_bev0 && !flow0) || (flow_bev1 && !flow1))) return LISO_EINVAL;
    if (n_max > 0 && moving_mask && (!pcl || !flow0 || !odom_tb_ta)) return LISO_EINVAL;
    if (isnan(threshold_dt)) return LISO_EINVAL;
    if (n_max > 0 && !pillar_coors) return LISO_EINVAL;
    if (!workspace || ((uintptr_t)workspace & 7) != 0) return LISO_EINVAL;
    const int n_flows = flow_bev1 ? 2 : (flow_bev0 ? 1 : 0);
    const size_t cells_total = (size_t)batch * grid_x * grid_y;
    const MapTables t = carve_maps(cells_total, n_flows, workspace);
    if (workspace_bytes < t.bytes) return LISO_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    if (liso_zero::zero_async(workspace, t.bytes, st) != hipSuccess) return LISO_ELAUNCH;
    const Maps m = {n_max, point_stride, grid_x, grid_y};
    if (n_max > 0) {
        const dim3 pts((unsigned)((n_max + kThreads - 1) / kThreads), batch);
        maps_scan_kernel<<<pts, kThreads, 0, st>>>(m, t, pcl, counts, pillar_coors, flow0, flow1, odom_tb_ta, threshold_dt, moving_mask);
        if (n_flows) maps_add_kernel<<<pts, kThreads, 0, st>>>(m, t, counts, pillar_coors, flow0, flow1);
    }
    if (occupancy || flow_bev0)
        maps_finalize_kernel<<<(unsigned)((cells_total + kThreads - 1) / kThreads), kThreads, 0, st>>>(cells_total, t, occupancy, flow_bev0,
                                                                                                      flow_bev1);
    return check_launch();
}

}  // extern "C"
