// Lidar odometry on the device (include/liso_odometry.h): range filter and first-come voxel downsampling, point-to-point ICP with
// an adaptive threshold against a voxel-hash map, and the map's update, for every frame of many padded sequences.
//
// One workgroup of kThreads lanes per sequence in every kernel, so __syncthreads is the only synchronisation, no block ever waits
// for another, and every loop is bounded by a size of the configuration (rows, table capacity, iterations).  Compiled with
// -ffp-contract=off: keys, kept points and stored values are fp64 expressions evaluated operation by operation, as
// liso_amd/odometry/host.py states them.
//
// Determinism.  A voxel's slot is claimed with a 64-bit compare-and-swap, so the slot depends on the race; nothing else does:
//   * first-come downsampling: atomicMax of ~index per claimed slot picks the smallest index, an ordered block scan compacts;
//   * the map: the voxels new in a frame are admitted in the order of their first point (ordered scan against the capacity), and
//     the points of a voxel are ranked by index through a cascade of atomicMin over a 20-entry list (entry j ends as the j-th
//     smallest index offered, whatever the interleaving), then appended behind the voxel's old points by one lane.
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/liso_odometry.h"
#include "dev_common.h"
#include "zero_fill.h"

using liso_dev::affine_inv;
using liso_dev::Carver;
using liso_dev::check_launch;
using liso_dev::cloud_rows;
using liso_dev::mat4_mul;
using liso_dev::shfl_xor_f64;

namespace {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;
constexpr int kVP = LISO_ODOM_VOXEL_POINTS;
constexpr int kHalf = LISO_ODOM_KEY_HALF_SPAN;
constexpr int kSums = 28;  // 21 of A's upper triangle, 6 of b, the number of kept pairs
typedef unsigned long long u64;

struct Ws {
    int32_t *n_ds, *n_src, *n_map, *n_err;
    double* sse;
    float *ds, *src, *qbuf;
    double* pcur;
    u64* kbuf;
    int32_t *aux, *lslot, *lists;
    u64* hkeys;
    uint32_t* hval;
    int32_t* hid;
    u64* mkeys;
    int32_t* mcnt;
    float* mpts;
    size_t H;  // slots of a sequence's scratch table
    size_t bytes;
};

size_t pow2_at_least(size_t v) {
    size_t p = 64;
    while (p < v) p <<= 1;
    return p;
}

bool cfg_ok(const liso_odometry_cfg* c) {
    if (!c) return false;
    if (c->n_seq < 0 || c->max_frames < 1 || c->n_max < 1 || c->n_max > LISO_ODOM_MAX_N) return false;
    if ((long long)c->n_seq * c->max_frames > (1 << 24)) return false;
    if (c->point_stride != 3 && c->point_stride != 4) return false;
    if (c->map_voxels < 64 || c->map_voxels > LISO_ODOM_MAX_MAP_VOXELS || (c->map_voxels & (c->map_voxels - 1))) return false;
    if (c->max_points_per_voxel < 1 || c->max_points_per_voxel > kVP || c->max_num_iterations < 1) return false;
    if (!(c->min_range >= 0.0) || !(c->max_range > c->min_range) || !(c->voxel_size > 0.0)) return false;
    if (!(c->max_range / (0.5 * c->voxel_size) < (double)kHalf)) return false;
    if (!(c->initial_threshold > 0.0) || !(c->min_motion_th >= 0.0) || !(c->convergence_criterion > 0.0)) return false;
    return true;
}

Ws carve(const liso_odometry_cfg* c, void* base) {
    Ws w;
    Carver cv{base};
    const size_t S = (size_t)c->n_seq, N = (size_t)c->n_max, V = (size_t)c->map_voxels;
    w.H = pow2_at_least(2 * N);
    w.n_ds = cv.take<int32_t>(S), w.n_src = cv.take<int32_t>(S), w.n_map = cv.take<int32_t>(S), w.n_err = cv.take<int32_t>(S);
    w.sse = cv.take<double>(S);
    w.ds = cv.take<float>(S * N * 3), w.src = cv.take<float>(S * N * 3), w.qbuf = cv.take<float>(S * N * 3);
    w.pcur = cv.take<double>(S * N * 3);
    w.kbuf = cv.take<u64>(S * N);
    w.aux = cv.take<int32_t>(S * N), w.lslot = cv.take<int32_t>(S * N), w.lists = cv.take<int32_t>(S * N * kVP);
    w.hkeys = cv.take<u64>(S * w.H), w.hval = cv.take<uint32_t>(S * w.H), w.hid = cv.take<int32_t>(S * w.H);
    w.mkeys = cv.take<u64>(S * 2 * V), w.mcnt = cv.take<int32_t>(S * 2 * V), w.mpts = cv.take<float>(S * 2 * V * kVP * 3);
    w.bytes = cv.bytes;
    return w;
}

// ---- device helpers -----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ u64 load_key(const u64* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ uint32_t load_u32(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int32_t load_i32(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the voxel index of coordinate v / size, or INT_MIN outside [-2^20, 2^20) (NaN included)
__device__ __forceinline__ int voxel_index(double v, double size) {
    const double k = floor(v / size);
    return (k >= -(double)kHalf && k < (double)kHalf) ? (int)k : INT_MIN;
}

__device__ __forceinline__ u64 pack_key(int kx, int ky, int kz) {
    return (1ull << 63) | ((u64)(kx + kHalf) << 42) | ((u64)(ky + kHalf) << 21) | (u64)(kz + kHalf);
}

// key of the voxel of (x, y, z), 0 when an index leaves the span
__device__ __forceinline__ u64 point_key(double x, double y, double z, double size) {
    const int kx = voxel_index(x, size), ky = voxel_index(y, size), kz = voxel_index(z, size);
    return (kx == INT_MIN || ky == INT_MIN || kz == INT_MIN) ? 0ull : pack_key(kx, ky, kz);
}

__device__ __forceinline__ uint32_t hash_key(u64 key) { return (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> 32); }

// the slot of `key` in a table of mask + 1 slots, claiming an empty one when the key is not there; -1 when every slot holds another key
__device__ int claim_slot(u64* keys, uint32_t mask, u64 key) {
    uint32_t h = hash_key(key) & mask;
    for (uint32_t probe = 0; probe <= mask; ++probe) {
        u64 cur = load_key(keys + h);
        if (cur == 0) cur = atomicCAS(keys + h, 0ull, key);
        if (cur == 0 || cur == key) return (int)h;
        h = (h + 1) & mask;
    }
    return -1;
}

// the slot of `key`, -1 when it is not in the table
__device__ int find_slot(const u64* keys, uint32_t mask, u64 key) {
    uint32_t h = hash_key(key) & mask;
    for (uint32_t probe = 0; probe <= mask; ++probe) {
        const u64 cur = load_key(keys + h);
        if (cur == key) return (int)h;
        if (cur == 0) return -1;
        h = (h + 1) & mask;
    }
    return -1;
}

// exclusive prefix of `flag` over the block in lane order; `total` = the block's sum.  lds: kWaves ints.  Two barriers.
__device__ int block_scan(int flag, int* lds, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u64 ballot = __ballot(flag);
    const int before = __popcll(ballot & ((1ull << lane) - 1ull));
    if (lane == 0) lds[wave] = __popcll(ballot);
    __syncthreads();
    int off = 0, tot = 0;
    for (int w = 0; w < kWaves; ++w) {
        const int v = lds[w];
        if (w < wave) off += v;
        tot += v;
    }
    __syncthreads();
    total = tot;
    return off + before;
}

__device__ void block_clear(void* p, size_t bytes) {  // bytes a multiple of 16, p 16-byte aligned
    uint4* q = (uint4*)p;
    const uint4 z = make_uint4(0u, 0u, 0u, 0u);
    for (size_t i = threadIdx.x; i < bytes / 16; i += kThreads) q[i] = z;
}

__device__ __forceinline__ bool finite3(double x, double y, double z) { return isfinite(x) && isfinite(y) && isfinite(z); }

// First-come voxel downsample of rows in[0..n) (stride floats per row) at voxel `size` into out (3 floats per row), input order
// kept; with `filter` a row must be finite with min_range < norm < max_range.  Returns the number of rows kept (every lane).
__device__ int downsample(const float* in, int stride, int n, bool filter, double min_range, double max_range, double size, float* out,
                          u64* hkeys, uint32_t* hval, uint32_t hmask, int32_t* aux, int* lds) {
    block_clear(hkeys, ((size_t)hmask + 1) * 8);
    block_clear(hval, ((size_t)hmask + 1) * 4);
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += kThreads) {
        const double x = in[(size_t)i * stride], y = in[(size_t)i * stride + 1], z = in[(size_t)i * stride + 2];
        int slot = -1;
        bool ok = true;
        if (filter) {
            const double norm = sqrt((x * x + y * y) + z * z);
            ok = finite3(x, y, z) && norm > min_range && norm < max_range;
        }
        if (ok) {
            const u64 key = point_key(x, y, z, size);
            if (key) slot = claim_slot(hkeys, hmask, key);  // (2n <= slots: a free one exists)
            if (slot >= 0) atomicMax(hval + slot, ~(uint32_t)i);
        }
        aux[i] = slot;
    }
    __syncthreads();
    int kept = 0;
    for (int base = 0; base < n; base += kThreads) {
        const int i = base + threadIdx.x;
        int keep = 0;
        if (i < n) {
            const int slot = aux[i];
            keep = slot >= 0 && load_u32(hval + slot) == ~(uint32_t)i;
        }
        int total;
        const int at = kept + block_scan(keep, lds, total);
        if (keep) {
            out[(size_t)at * 3] = in[(size_t)i * stride], out[(size_t)at * 3 + 1] = in[(size_t)i * stride + 1];
            out[(size_t)at * 3 + 2] = in[(size_t)i * stride + 2];
        }
        kept += total;
    }
    __syncthreads();
    return kept;
}

__device__ __forceinline__ int frames_of(const int32_t* n_frames, int s, int F) {
    const int n = n_frames[s];
    return n < 0 ? 0 : (n > F ? F : n);
}

// ---- stage 1 ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void preprocess_kernel(liso_odometry_cfg c, int f, const float* __restrict__ clouds,
                                                              const int32_t* __restrict__ counts, const int32_t* __restrict__ n_frames,
                                                              int32_t* __restrict__ n_source, Ws w) {
    __shared__ int lds[kWaves];
    const int s = blockIdx.x, F = c.max_frames, N = c.n_max;
    if (f >= frames_of(n_frames, s, F)) return;
    const size_t sf = (size_t)s * F + f;
    const int n = cloud_rows(counts, (int)sf, N);
    u64* hkeys = w.hkeys + (size_t)s * w.H;
    uint32_t* hval = w.hval + (size_t)s * w.H;
    int32_t* aux = w.aux + (size_t)s * N;
    float* ds = w.ds + (size_t)s * N * 3;
    float* src = w.src + (size_t)s * N * 3;
    const uint32_t hmask = (uint32_t)(w.H - 1);
    const int n_ds = downsample(clouds + sf * N * c.point_stride, c.point_stride, n, true, c.min_range, c.max_range, 0.5 * c.voxel_size, ds,
                                hkeys, hval, hmask, aux, lds);
    const int n_src = downsample(ds, 3, n_ds, false, 0.0, 0.0, 1.5 * c.voxel_size, src, hkeys, hval, hmask, aux, lds);
    if (threadIdx.x == 0) w.n_ds[s] = n_ds, w.n_src[s] = n_src, n_source[sf] = n_src;
}

// ---- stage 2 ------------------------------------------------------------------------------------------------------------------
__device__ void identity4(double* M) {
    for (int i = 0; i < 16; ++i) M[i] = (i % 5 == 0) ? 1.0 : 0.0;
}

// 1 - x / (first (first + 1)) (1 - x / ((first + 2) (first + 3)) (1 - ...)), 10 factors, innermost first: products, quotients and
// differences only, so host and device get the same bits (liso_amd/odometry/host.py: _series)
__device__ double series(double x, int first) {
    double acc = 1.0;
    for (int k = 9; k >= 0; --k) acc = 1.0 - (x / (double)((first + 2 * k) * (first + 2 * k + 1))) * acc;
    return acc;
}

// E = exp of the twist (v, w): R = exp([w]x) = I + a W + b W^2, t = V(w) v, V = I + b W + c W^2; a, b, c by their series for |w| < 0.5
__device__ void exp_se3(const double* dx, double* E) {
    const double vx = dx[0], vy = dx[1], vz = dx[2], wx = dx[3], wy = dx[4], wz = dx[5];
    const double th2 = (wx * wx + wy * wy) + wz * wz;
    double a, b, cc;
    if (th2 < 0.25) {
        a = series(th2, 2), b = 0.5 * series(th2, 3), cc = series(th2, 4) / 6.0;
    } else {
        const double th = sqrt(th2);
        const double half = sin(0.5 * th) / (0.5 * th);  // (1 - cos th) / th^2 through the half angle
        a = sin(th) / th, b = 0.5 * (half * half), cc = (th - sin(th)) / (th2 * th);
    }
    const double W[9] = {0.0, -wz, wy, wz, 0.0, -wx, -wy, wx, 0.0};
    double W2[9];
    for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 3; ++k) W2[3 * r + k] = (W[3 * r] * W[k] + W[3 * r + 1] * W[3 + k]) + W[3 * r + 2] * W[6 + k];
    const double v[3] = {vx, vy, vz};
    for (int r = 0; r < 3; ++r) {
        double Vr[3];
        for (int k = 0; k < 3; ++k) {
            const double id = r == k ? 1.0 : 0.0;
            E[4 * r + k] = (id + a * W[3 * r + k]) + b * W2[3 * r + k];
            Vr[k] = (id + b * W[3 * r + k]) + cc * W2[3 * r + k];
        }
        E[4 * r + 3] = (Vr[0] * v[0] + Vr[1] * v[1]) + Vr[2] * v[2];
    }
    E[12] = 0.0, E[13] = 0.0, E[14] = 0.0, E[15] = 1.0;
}

// x = solve(A, rhs) by LDL^T for the symmetric 6x6 A; false when a pivot is not positive or x is not finite
__device__ bool solve_ldlt6(const double A[6][6], const double* rhs, double* x) {
    double L[6][6], d[6];
    for (int j = 0; j < 6; ++j) {
        double dj = A[j][j];
        for (int k = 0; k < j; ++k) dj -= L[j][k] * L[j][k] * d[k];
        if (!(dj > 0.0)) return false;
        d[j] = dj;
        for (int i = j + 1; i < 6; ++i) {
            double v = A[i][j];
            for (int k = 0; k < j; ++k) v -= L[i][k] * L[j][k] * d[k];
            L[i][j] = v / dj;
        }
    }
    double y[6];
    for (int i = 0; i < 6; ++i) {
        double v = rhs[i];
        for (int k = 0; k < i; ++k) v -= L[i][k] * y[k];
        y[i] = v;
    }
    for (int i = 5; i >= 0; --i) {
        double v = y[i] / d[i];
        for (int k = i + 1; k < 6; ++k) v -= L[k][i] * x[k];
        x[i] = v;
    }
    for (int i = 0; i < 6; ++i)
        if (!isfinite(x[i])) return false;
    return true;
}

__global__ __launch_bounds__(kThreads) void register_kernel(liso_odometry_cfg c, int f, const int32_t* __restrict__ n_frames,
                                                            const double* __restrict__ guess, const double* __restrict__ sigma_given,
                                                            double* __restrict__ poses, double* __restrict__ sigma_out,
                                                            int32_t* __restrict__ n_iterations, int32_t* __restrict__ converged, Ws w) {
    __shared__ double G[16], E[16], Ticp[16], red[kWaves][kSums], tot[kSums], sh_sigma;
    __shared__ int sh_state;  // 0 go on, 1 stop after this iteration (converged), 2 failed
    const int s = blockIdx.x, F = c.max_frames, N = c.n_max, V = c.map_voxels;
    if (f >= frames_of(n_frames, s, F)) return;
    const size_t sf = (size_t)s * F + f;
    double* P = poses + (size_t)s * F * 16;
    const bool given = guess != nullptr;
    if (threadIdx.x == 0) {
        double sig = c.initial_threshold;
        if (given) {
            for (int i = 0; i < 16; ++i) G[i] = guess[(size_t)s * 16 + i];
            sig = sigma_given[s];
        } else if (f == 0) {
            identity4(G);
            w.sse[s] = 0.0, w.n_err[s] = 0;
        } else {
            const double* T1 = P + (size_t)(f - 1) * 16;
            if (f < 2) {
                for (int i = 0; i < 16; ++i) G[i] = T1[i];
            } else {
                double inv2[16], pred[16];
                affine_inv(P + (size_t)(f - 2) * 16, inv2);
                mat4_mul(inv2, T1, pred);
                mat4_mul(T1, pred, G);
            }
            double inv0[16], D0[16];
            affine_inv(P, inv0);
            mat4_mul(inv0, T1, D0);
            const double moved = sqrt((D0[3] * D0[3] + D0[7] * D0[7]) + D0[11] * D0[11]);
            const int n_err = w.n_err[s];
            if (moved > 5.0 * c.min_motion_th && n_err > 0) sig = sqrt(w.sse[s] / (double)n_err);
        }
        sh_sigma = sig;
        identity4(Ticp);
        sh_state = 0;
    }
    __syncthreads();
    const double sig = sh_sigma, max_corr = 3.0 * sig, kappa = sig / 3.0, vs = c.voxel_size;
    const int n = w.n_src[s], n_map = (f == 0 && !given) ? 0 : w.n_map[s];
    const int tb = (f + 1) & 1;
    const u64* mkeys = w.mkeys + ((size_t)s * 2 + tb) * V;
    const int32_t* mcnt = w.mcnt + ((size_t)s * 2 + tb) * V;
    const float* mpts = w.mpts + ((size_t)s * 2 + tb) * V * kVP * 3;
    const float* src = w.src + (size_t)s * N * 3;
    double* pc = w.pcur + (size_t)s * N * 3;
    const uint32_t mmask = (uint32_t)V - 1u;
    int it = 0, conv = 1;
    if (n_map > 0) {
        for (int i = threadIdx.x; i < n; i += kThreads) {
            const double x = src[(size_t)i * 3], y = src[(size_t)i * 3 + 1], z = src[(size_t)i * 3 + 2];
            for (int r = 0; r < 3; ++r) pc[(size_t)i * 3 + r] = ((G[4 * r] * x + G[4 * r + 1] * y) + G[4 * r + 2] * z) + G[4 * r + 3];
        }
        conv = 0;
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        while (it < c.max_num_iterations) {
            double acc[kSums];
            for (int k = 0; k < kSums; ++k) acc[k] = 0.0;
            for (int i = threadIdx.x; i < n; i += kThreads) {
                const double px = pc[(size_t)i * 3], py = pc[(size_t)i * 3 + 1], pz = pc[(size_t)i * 3 + 2];
                const int bx = voxel_index(px, vs), by = voxel_index(py, vs), bz = voxel_index(pz, vs);
                if (bx == INT_MIN || by == INT_MIN || bz == INT_MIN) continue;
                double best = INFINITY, qx = 0.0, qy = 0.0, qz = 0.0;
                for (int dx = -1; dx <= 1; ++dx)
                    for (int dy = -1; dy <= 1; ++dy)
                        for (int dz = -1; dz <= 1; ++dz) {
                            const int kx = bx + dx, ky = by + dy, kz = bz + dz;
                            if (kx < -kHalf || kx >= kHalf || ky < -kHalf || ky >= kHalf || kz < -kHalf || kz >= kHalf) continue;
                            const int slot = find_slot(mkeys, mmask, pack_key(kx, ky, kz));
                            if (slot < 0) continue;
                            int cnt = mcnt[slot];
                            cnt = cnt > kVP ? kVP : cnt;
                            const float* q = mpts + (size_t)slot * kVP * 3;
                            for (int j = 0; j < cnt; ++j) {
                                const double x = q[3 * j], y = q[3 * j + 1], z = q[3 * j + 2];
                                const double ex = px - x, ey = py - y, ez = pz - z;
                                const double d2 = (ex * ex + ey * ey) + ez * ez;
                                if (d2 < best) best = d2, qx = x, qy = y, qz = z;
                            }
                        }
                if (!(sqrt(best) < max_corr)) continue;
                const double r[3] = {px - qx, py - qy, pz - qz};
                const double rr = (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2];
                const double wgt = (kappa * kappa) / ((kappa + rr) * (kappa + rr));
                const double J[3][6] = {{1.0, 0.0, 0.0, 0.0, pz, -py}, {0.0, 1.0, 0.0, -pz, 0.0, px}, {0.0, 0.0, 1.0, py, -px, 0.0}};
                int k = 0;
                for (int a = 0; a < 6; ++a)
                    for (int b = a; b < 6; ++b, ++k) acc[k] += wgt * ((J[0][a] * J[0][b] + J[1][a] * J[1][b]) + J[2][a] * J[2][b]);
                for (int a = 0; a < 6; ++a, ++k) acc[k] += wgt * ((J[0][a] * r[0] + J[1][a] * r[1]) + J[2][a] * r[2]);
                acc[27] += 1.0;
            }
            for (int k = 0; k < kSums; ++k) {
                double v = acc[k];
                for (int m = 1; m < 64; m <<= 1) v += shfl_xor_f64(v, m);
                if (lane == 0) red[wave][k] = v;
            }
            __syncthreads();
            if (threadIdx.x < kSums) {
                double v = 0.0;
                for (int wv = 0; wv < kWaves; ++wv) v += red[wv][threadIdx.x];
                tot[threadIdx.x] = v;
            }
            __syncthreads();
            if (threadIdx.x == 0) {
                int state = 2;
                if (tot[27] > 0.0) {
                    double A[6][6], rhs[6], dx[6];
                    int k = 0;
                    for (int a = 0; a < 6; ++a)
                        for (int b = a; b < 6; ++b, ++k) A[a][b] = tot[k], A[b][a] = tot[k];
                    for (int a = 0; a < 6; ++a, ++k) rhs[a] = -tot[k];
                    if (solve_ldlt6(A, rhs, dx)) {
                        double T2[16];
                        exp_se3(dx, E);
                        mat4_mul(E, Ticp, T2);
                        for (int i = 0; i < 16; ++i) Ticp[i] = T2[i];
                        double n2 = 0.0;
                        for (int i = 0; i < 6; ++i) n2 += dx[i] * dx[i];
                        state = sqrt(n2) < c.convergence_criterion ? 1 : 0;
                    }
                }
                sh_state = state;
            }
            __syncthreads();
            const int state = sh_state;
            if (state == 2) break;
            for (int i = threadIdx.x; i < n; i += kThreads) {
                const double x = pc[(size_t)i * 3], y = pc[(size_t)i * 3 + 1], z = pc[(size_t)i * 3 + 2];
                for (int r = 0; r < 3; ++r) pc[(size_t)i * 3 + r] = ((E[4 * r] * x + E[4 * r + 1] * y) + E[4 * r + 2] * z) + E[4 * r + 3];
            }
            ++it;
            if (state == 1) {
                conv = 1;
                break;
            }
            __syncthreads();  // (E and sh_state are rewritten in the next round)
        }
    }
    if (threadIdx.x == 0) {
        double T[16];
        if (n_map > 0 && sh_state != 2) {
            mat4_mul(Ticp, G, T);
        } else {
            for (int i = 0; i < 16; ++i) T[i] = G[i];
        }
        bool fin = true;
        for (int i = 0; i < 16; ++i) fin = fin && isfinite(T[i]);
        if (!fin) {
            for (int i = 0; i < 16; ++i) T[i] = G[i];
            conv = 0;
        }
        for (int i = 0; i < 16; ++i) P[(size_t)f * 16 + i] = T[i];
        sigma_out[sf] = sig, n_iterations[sf] = it, converged[sf] = conv;
        if (!given) {
            double Gi[16], D[16];
            affine_inv(G, Gi);
            mat4_mul(Gi, T, D);
            double ct = 0.5 * (((D[0] + D[5]) + D[10]) - 1.0);
            ct = ct < -1.0 ? -1.0 : (ct > 1.0 ? 1.0 : ct);
            // 2 max_range sin(theta / 2) with cos theta = ct, as max_range sqrt(2 (1 - ct)): no acos, no sin, the host's bits
            const double e = c.max_range * sqrt(2.0 * (1.0 - ct)) + sqrt((D[3] * D[3] + D[7] * D[7]) + D[11] * D[11]);
            if (e > c.min_motion_th) w.sse[s] += e * e, w.n_err[s] += 1;
        }
    }
}

// ---- stage 3 ------------------------------------------------------------------------------------------------------------------
// squared distance of the fp32 point q from t exceeds max_range^2
__device__ __forceinline__ bool beyond(const float* q, const double* t, double max_range) {
    const double ex = (double)q[0] - t[0], ey = (double)q[1] - t[1], ez = (double)q[2] - t[2];
    return (ex * ex + ey * ey) + ez * ez > max_range * max_range;
}

__global__ __launch_bounds__(kThreads) void map_update_kernel(liso_odometry_cfg c, int f, const int32_t* __restrict__ n_frames,
                                                              const double* __restrict__ poses, int32_t* __restrict__ map_overflow, Ws w) {
    __shared__ int lds[kWaves], sh_voxels, sh_overflow;
    __shared__ double T[16];
    const int s = blockIdx.x, F = c.max_frames, N = c.n_max, V = c.map_voxels, cap = c.max_points_per_voxel;
    if (f >= frames_of(n_frames, s, F)) return;
    const int tn = f & 1, to = (f + 1) & 1;
    u64* nkeys = w.mkeys + ((size_t)s * 2 + tn) * V;
    int32_t* ncnt = w.mcnt + ((size_t)s * 2 + tn) * V;
    float* npts = w.mpts + ((size_t)s * 2 + tn) * V * kVP * 3;
    const u64* okeys = w.mkeys + ((size_t)s * 2 + to) * V;
    const int32_t* ocnt = w.mcnt + ((size_t)s * 2 + to) * V;
    const float* opts = w.mpts + ((size_t)s * 2 + to) * V * kVP * 3;
    u64* hkeys = w.hkeys + (size_t)s * w.H;
    uint32_t* hval = w.hval + (size_t)s * w.H;
    int32_t* hid = w.hid + (size_t)s * w.H;
    int32_t* aux = w.aux + (size_t)s * N;
    int32_t* lslot = w.lslot + (size_t)s * N;
    int32_t* lists = w.lists + (size_t)s * N * kVP;
    float* qbuf = w.qbuf + (size_t)s * N * 3;
    u64* kbuf = w.kbuf + (size_t)s * N;
    const float* ds = w.ds + (size_t)s * N * 3;
    const uint32_t hmask = (uint32_t)(w.H - 1), mmask = (uint32_t)V - 1u;
    const bool old_empty = f == 0;
    const int n = w.n_ds[s], n_old = old_empty ? 0 : w.n_map[s];
    if (threadIdx.x < 16) T[threadIdx.x] = poses[((size_t)s * F + f) * 16 + threadIdx.x];
    if (threadIdx.x == 0) sh_voxels = 0, sh_overflow = 0;
    block_clear(hkeys, (w.H) * 8);
    block_clear(hval, (w.H) * 4);
    block_clear(nkeys, (size_t)V * 8);
    block_clear(ncnt, (size_t)V * 4);
    __syncthreads();
    const double t[3] = {T[3], T[7], T[11]};
    // 1. the old table's voxels whose first point is in range, payload in order
    if (!old_empty) {
        int mine = 0;
        for (int slot = threadIdx.x; slot < V; slot += kThreads) {
            const u64 key = okeys[slot];
            if (key == 0) continue;
            const float* q = opts + (size_t)slot * kVP * 3;
            if (beyond(q, t, c.max_range)) continue;
            const int ns = claim_slot(nkeys, mmask, key);  // (as many slots as the old table had voxels: one is free)
            if (ns < 0) continue;
            int cnt = ocnt[slot];
            cnt = cnt > kVP ? kVP : cnt;
            ncnt[ns] = cnt;
            float* d = npts + (size_t)ns * kVP * 3;
            for (int j = 0; j < 3 * cnt; ++j) d[j] = q[j];
            ++mine;
        }
        if (mine) atomicAdd(&sh_voxels, mine);
    }
    // 2. the frame's points in the world, their voxels, the first point of every voxel
    int lost = 0;
    for (int i = threadIdx.x; i < n; i += kThreads) {
        const double x = ds[(size_t)i * 3], y = ds[(size_t)i * 3 + 1], z = ds[(size_t)i * 3 + 2];
        double q[3];
        for (int r = 0; r < 3; ++r) q[r] = ((T[4 * r] * x + T[4 * r + 1] * y) + T[4 * r + 2] * z) + T[4 * r + 3];
        const u64 key = point_key(q[0], q[1], q[2], c.voxel_size);
        qbuf[(size_t)i * 3] = (float)q[0], qbuf[(size_t)i * 3 + 1] = (float)q[1], qbuf[(size_t)i * 3 + 2] = (float)q[2];
        kbuf[i] = key;
        int slot = -1;
        if (key) slot = claim_slot(hkeys, hmask, key);
        if (slot >= 0) atomicMax(hval + slot, ~(uint32_t)i);
        else ++lost;
        aux[i] = slot;
    }
    __syncthreads();
    // 3. voxel by voxel in the order of the first points: kept from the old table, gone with it, new and admitted, or new and refused
    int n_new = 0, n_lists = 0;
    for (int base = 0; base < n; base += kThreads) {
        const int i = base + threadIdx.x;
        int leader = 0, is_new = 0, in_range = 0, hs = -1, mslot = -1;
        u64 key = 0;
        if (i < n) {
            hs = aux[i];
            leader = hs >= 0 && load_u32(hval + hs) == ~(uint32_t)i;
        }
        if (leader) {
            key = kbuf[i];
            const int os = old_empty ? -1 : find_slot(okeys, mmask, key);
            if (os >= 0) {
                mslot = find_slot(nkeys, mmask, key);  // -1: the voxel left with its first point
            } else {
                is_new = 1;
                in_range = !beyond(qbuf + (size_t)i * 3, t, c.max_range);
            }
        }
        int total_new;
        const int rank = n_new + block_scan(is_new, lds, total_new);
        n_new += total_new;
        int status = -1;  // -1 dropped with its voxel, -2 no slot, >= 0 a list
        if (is_new) {
            if ((long long)n_old + rank >= (long long)V) status = -2;
            else if (in_range) mslot = claim_slot(nkeys, mmask, key);
        }
        const int present = leader && status != -2 && mslot >= 0;
        int total_lists;
        const int id = n_lists + block_scan(present, lds, total_lists);
        n_lists += total_lists;
        if (leader) {
            if (present) {
                status = id;
                lslot[id] = mslot;
                for (int j = 0; j < kVP; ++j) lists[(size_t)id * kVP + j] = INT_MAX;
                if (is_new) atomicAdd(&sh_voxels, 1);
            }
            hid[hs] = status;
        }
    }
    __syncthreads();
    // 4. every point offers its index to its voxel's list
    for (int i = threadIdx.x; i < n; i += kThreads) {
        const int hs = aux[i];
        if (hs < 0) continue;
        const int id = hid[hs];
        if (id == -2) ++lost;
        if (id < 0) continue;
        int v = i;
        for (int j = 0; j < kVP && v != INT_MAX; ++j) {
            const int old = atomicMin(lists + (size_t)id * kVP + j, v);
            v = old > v ? old : v;
        }
    }
    if (lost) atomicAdd(&sh_overflow, lost);
    __syncthreads();
    // 5. one lane per voxel appends its points in index order
    for (int id = threadIdx.x; id < n_lists; id += kThreads) {
        const int slot = lslot[id];
        int cnt = ncnt[slot];
        float* d = npts + (size_t)slot * kVP * 3;
        for (int j = 0; j < kVP && cnt < cap; ++j) {
            const int idx = load_i32(lists + (size_t)id * kVP + j);
            if (idx == INT_MAX) break;
            d[3 * cnt] = qbuf[(size_t)idx * 3], d[3 * cnt + 1] = qbuf[(size_t)idx * 3 + 1], d[3 * cnt + 2] = qbuf[(size_t)idx * 3 + 2];
            ++cnt;
        }
        ncnt[slot] = cnt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        w.n_map[s] = sh_voxels;
        map_overflow[s] = (old_empty ? 0 : map_overflow[s]) + sh_overflow;
    }
}

// ---- small kernels ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void identity_poses_kernel(double* __restrict__ poses, size_t count) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count * 16; i += (size_t)gridDim.x * blockDim.x)
        poses[i] = (i % 16) % 5 == 0 ? 1.0 : 0.0;
}

__global__ __launch_bounds__(64) void relative_kernel(int count, const double* __restrict__ a, const double* __restrict__ b,
                                                      double* __restrict__ out) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= count) return;
    double A[16], B[16], inv[16], C[16];
    for (int i = 0; i < 16; ++i) A[i] = a[(size_t)k * 16 + i], B[i] = b[(size_t)k * 16 + i];
    affine_inv(A, inv);
    mat4_mul(inv, B, C);
    for (int i = 0; i < 16; ++i) out[(size_t)k * 16 + i] = C[i];
}

__global__ __launch_bounds__(256) void correct_kitti_kernel(long n, const double* __restrict__ in, double* __restrict__ out) {
    const double angle = 0.205 * M_PI / 180.0;
    const double ca = cos(angle), sa = sin(angle);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const double x = in[3 * i], y = in[3 * i + 1], z = in[3 * i + 2];
        double ox = x, oy = y, oz = z;
        const double ax = y, ay = -x;  // p x e_z = (y, -x, 0)
        const double len = sqrt(ax * ax + ay * ay);
        if (len > 0.0) {
            const double kx = ax / len, ky = ay / len;
            const double kp = kx * x + ky * y;                         // k . p
            const double cx = ky * z, cy = -(kx * z), cz = kx * y - ky * x;  // k x p
            ox = (x * ca + cx * sa) + kx * kp * (1.0 - ca);
            oy = (y * ca + cy * sa) + ky * kp * (1.0 - ca);
            oz = z * ca + cz * sa;
        }
        out[3 * i] = ox, out[3 * i + 1] = oy, out[3 * i + 2] = oz;
    }
}

bool aligned256(const void* p) { return ((uintptr_t)p & 255) == 0; }

// LISO_OK when the workspace serves cfg, else the error
int check_ws(const liso_odometry_cfg* cfg, int frame, const void* workspace, size_t workspace_bytes) {
    if (!cfg_ok(cfg) || frame < 0 || frame >= cfg->max_frames) return LISO_EINVAL;
    if (cfg->n_seq == 0) return LISO_OK;
    if (!workspace || !aligned256(workspace)) return LISO_EINVAL;
    if (workspace_bytes < carve(cfg, nullptr).bytes) return LISO_EWORKSPACE;
    return LISO_OK;
}

}  // namespace

extern "C" {

size_t liso_odometry_workspace_bytes(const liso_odometry_cfg* cfg) {
    if (!cfg_ok(cfg)) return 0;
    const size_t b = carve(cfg, nullptr).bytes;
    return b ? b : 256;
}

int liso_odometry_workspace_layout(const liso_odometry_cfg* cfg, size_t* offsets) {
    if (!cfg_ok(cfg) || !offsets) return LISO_EINVAL;
    const Ws w = carve(cfg, nullptr);
    const void* at[10] = {w.ds, w.n_ds, w.src, w.n_src, w.mkeys, w.mcnt, w.mpts, w.n_map, w.sse, w.n_err};
    for (int i = 0; i < LISO_ODOM_N_LAYOUT; ++i) offsets[i] = i < 10 ? (size_t)(uintptr_t)at[i] : 0;
    return LISO_OK;
}

int liso_odometry_preprocess(const liso_odometry_cfg* cfg, int frame, const float* clouds, const int32_t* counts, const int32_t* n_frames,
                             int32_t* n_source, void* workspace, size_t workspace_bytes, void* stream) {
    const int rc = check_ws(cfg, frame, workspace, workspace_bytes);
    if (rc != LISO_OK) return rc;
    if (cfg->n_seq == 0) return LISO_OK;
    if (!clouds || !n_frames || !n_source) return LISO_EINVAL;
    preprocess_kernel<<<cfg->n_seq, kThreads, 0, (hipStream_t)stream>>>(*cfg, frame, clouds, counts, n_frames, n_source, carve(cfg, workspace));
    return check_launch();
}

int liso_odometry_register(const liso_odometry_cfg* cfg, int frame, const int32_t* n_frames, const double* guess, const double* sigma_given,
                           double* poses, double* sigma, int32_t* n_iterations, int32_t* converged, void* workspace, size_t workspace_bytes,
                           void* stream) {
    const int rc = check_ws(cfg, frame, workspace, workspace_bytes);
    if (rc != LISO_OK) return rc;
    if ((guess == nullptr) != (sigma_given == nullptr)) return LISO_EINVAL;
    if (cfg->n_seq == 0) return LISO_OK;
    if (!n_frames || !poses || !sigma || !n_iterations || !converged) return LISO_EINVAL;
    register_kernel<<<cfg->n_seq, kThreads, 0, (hipStream_t)stream>>>(*cfg, frame, n_frames, guess, sigma_given, poses, sigma, n_iterations,
                                                                      converged, carve(cfg, workspace));
    return check_launch();
}

int liso_odometry_map_update(const liso_odometry_cfg* cfg, int frame, const int32_t* n_frames, const double* poses, int32_t* map_overflow,
                             void* workspace, size_t workspace_bytes, void* stream) {
    const int rc = check_ws(cfg, frame, workspace, workspace_bytes);
    if (rc != LISO_OK) return rc;
    if (cfg->n_seq == 0) return LISO_OK;
    if (!n_frames || !poses || !map_overflow) return LISO_EINVAL;
    map_update_kernel<<<cfg->n_seq, kThreads, 0, (hipStream_t)stream>>>(*cfg, frame, n_frames, poses, map_overflow, carve(cfg, workspace));
    return check_launch();
}

int liso_odometry_sequences(const liso_odometry_cfg* cfg, const float* clouds, const int32_t* counts, const int32_t* n_frames, double* poses,
                            double* sigma, int32_t* n_source, int32_t* n_iterations, int32_t* converged, int32_t* map_overflow,
                            void* workspace, size_t workspace_bytes, void* stream) {
    const int rc = check_ws(cfg, 0, workspace, workspace_bytes);
    if (rc != LISO_OK) return rc;
    if (cfg->n_seq == 0) return LISO_OK;
    if (!clouds || !n_frames || !poses || !sigma || !n_source || !n_iterations || !converged || !map_overflow) return LISO_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const Ws w = carve(cfg, workspace);
    const size_t S = (size_t)cfg->n_seq, SF = S * cfg->max_frames, V = (size_t)cfg->map_voxels;
    // the per-sequence sums and counts (the workspace's head, up to the first point table), both tables' keys and counts, the outputs
    if (liso_zero::zero_async(workspace, (size_t)((char*)w.ds - (char*)workspace), st) != hipSuccess) return LISO_ELAUNCH;
    if (liso_zero::zero_async(w.mkeys, S * 2 * V * 8, st) != hipSuccess) return LISO_ELAUNCH;
    if (liso_zero::zero_async(w.mcnt, S * 2 * V * 4, st) != hipSuccess) return LISO_ELAUNCH;
    if (liso_zero::zero_async(sigma, SF * 8, st) != hipSuccess) return LISO_ELAUNCH;
    if (liso_zero::zero_async(n_source, SF * 4, st) != hipSuccess) return LISO_ELAUNCH;
    if (liso_zero::zero_async(n_iterations, SF * 4, st) != hipSuccess) return LISO_ELAUNCH;
    if (liso_zero::zero_async(converged, SF * 4, st) != hipSuccess) return LISO_ELAUNCH;
    if (liso_zero::zero_async(map_overflow, S * 4, st) != hipSuccess) return LISO_ELAUNCH;
    identity_poses_kernel<<<(unsigned)((SF * 16 + 255) / 256 > 1024 ? 1024 : (SF * 16 + 255) / 256), 256, 0, st>>>(poses, SF);
    if (check_launch() != LISO_OK) return LISO_ELAUNCH;
    for (int f = 0; f < cfg->max_frames; ++f) {
        preprocess_kernel<<<cfg->n_seq, kThreads, 0, st>>>(*cfg, f, clouds, counts, n_frames, n_source, w);
        register_kernel<<<cfg->n_seq, kThreads, 0, st>>>(*cfg, f, n_frames, nullptr, nullptr, poses, sigma, n_iterations, converged, w);
        map_update_kernel<<<cfg->n_seq, kThreads, 0, st>>>(*cfg, f, n_frames, poses, map_overflow, w);
        if (check_launch() != LISO_OK) return LISO_ELAUNCH;
    }
    return LISO_OK;
}

int liso_odometry_relative_f64(int count, const double* a, const double* b, double* out, void* stream) {
    if (count < 0) return LISO_EINVAL;
    if (count == 0) return LISO_OK;
    if (!a || !b || !out) return LISO_EINVAL;
    relative_kernel<<<(count + 63) / 64, 64, 0, (hipStream_t)stream>>>(count, a, b, out);
    return check_launch();
}

int liso_correct_kitti_scan_f64(long n, const double* points, double* out, void* stream) {
    if (n < 0) return LISO_EINVAL;
    if (n == 0) return LISO_OK;
    if (!points || !out) return LISO_EINVAL;
    const long blocks = (n + 255) / 256;
    correct_kitti_kernel<<<(unsigned)(blocks > 4096 ? 4096 : blocks), 256, 0, (hipStream_t)stream>>>(n, points, out);
    return check_launch();
}

}  // extern "C"
