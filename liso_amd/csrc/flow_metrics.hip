// Scene-flow validation metrics on gfx950.  C ABI, categories and per-point arithmetic: include/liso_flow_metrics.h.
//
// Launch 1 (grid kBlocks(rows) x n_flows, 256 threads): every wave walks 64-row tiles in a fixed order.  Per lane it keeps the
// label-category counts and sums of its own rows in registers (sequential in the lane's rows).  The range bins cannot be indexed
// registers, so per tile every lane stages (bin slot, EPE) of its row in LDS, and lane `category * 32 + bin` owns that slot: it
// walks the 64 staged rows in lane order and adds the ones of its slot.  At the end the per-thread values are staged in LDS and
// one thread per value adds the 256 threads in thread order; the 4 waves' bin slots are added in wave order; the block writes one
// record of kRec slots (96 f64 sums, 96 counts).  (Serial cross-lane xor butterflies for the same sums, ~60 per wave, made this
// launch a latency chain of ~41 us at 120k points x 3 flows.)
// Launch 2 (one wave per record slot and flow): lane l adds the records of blocks l, l + 64, ... in that order, the wave adds the
// 64 lane sums by an xor butterfly (identical bits in every lane: every level adds a pair in both orders, and IEEE addition
// commutes), and lane 0 adds the total into the state.  The grid of launch 1 depends on `rows` only (one 64-row tile per wave up
// to kMaxBlocks blocks), so the bits depend on the inputs only.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/liso_flow_metrics.h"
#include "../../include/liso_iou3d.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxBlocks = 512;  // per flow
constexpr int kRowsPerBlock = 64 * kWaves;
constexpr int kSums = 96, kRec = 192;  // record: [0, 96) f64 sums, [96, 192) u64 counts
constexpr int kMaxBins = LISO_FLOW_METRICS_MAX_BINS;
// record slots: sums [0,64) range bins (lane c*32+j, c: 0 still, 1 moving), [64,76) label moving, [76,88) label still,
// 88 / 89 range totals still / moving; counts (offset 96) [0,64) range bins, [64,69) label moving, [69,74) label still,
// 74 / 75 range totals still / moving
constexpr int kLabelSums = 64, kRangeTotalSums = 88, kLabelCounts = 64, kRangeTotalCounts = 74;
constexpr size_t kPartialsOffset = (sizeof(liso_flow_metrics_result) + 255) / 256 * 256;
constexpr size_t kStateBytes = kPartialsOffset + sizeof(double) * kRec * kMaxBlocks * LISO_FLOW_METRICS_MAX_FLOWS;

struct Edges {
    double e[kMaxBins + 1];
};

struct Args {
    const float* points;
    long points_stride;
    const float* gt;
    long gt_stride;
    const float* pred[LISO_FLOW_METRICS_MAX_FLOWS];
    long pred_stride[LISO_FLOW_METRICS_MAX_FLOWS];
    const uint8_t* valid;
    const uint8_t* moving;
    const uint8_t* label;
    long rows;
    int n_bins;
    float* point_epe;
    double* partials;
    Edges edges;
};

__device__ __forceinline__ float norm3(float x, float y, float z) {
    // np.linalg.norm(a, axis=-1) of an f32 [.., 3] array: sqrt(add.reduce(a * a)) = sqrt((x*x + y*y) + z*z), correctly rounded
    return sqrtf((x * x + y * y) + z * z);
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// LDS written by some lanes of this wave is read by other lanes of the same wave (LDS operations of one wave are processed in
// order; the fences keep the compiler from moving them across)
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

inline int blocks_for(long rows) {
    long b = (rows + kRowsPerBlock - 1) / kRowsPerBlock;
    return (int)(b < 1 ? 1 : (b > kMaxBlocks ? kMaxBlocks : b));
}

__global__ __launch_bounds__(kThreads) void flow_metrics_partials_kernel(Args a) {
    __shared__ double edges[kMaxBins + 1];
    __shared__ double s_bin[kWaves][64];
    __shared__ unsigned c_bin[kWaves][64];
    __shared__ float t_epe[kWaves][64];  // per-tile staging of (bin slot, EPE)
    __shared__ int t_slot[kWaves][64];
    __shared__ double s_stage[kThreads][13];  // end of block: per-thread sums, half of them at a time
    __shared__ unsigned c_stage[kThreads][12];
    __shared__ double s_oth[26];
    __shared__ unsigned c_oth[12];

    const int k = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nb = a.n_bins;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int j = 0; j <= kMaxBins; ++j) edges[j] = a.edges.e[j];  // (constant indices: the kernarg struct stays in SGPR loads)
    }
    __syncthreads();

    const float* __restrict__ pred = a.pred[k];
    const long ps = a.pred_stride[k];
    double acc_bin = 0.0;  // range bin (lane / 32, lane % 32)
    unsigned cnt_bin = 0;
    double lsum[2][12];
    unsigned lcnt[2][5];
    double rsum[2] = {0.0, 0.0};
    unsigned rcnt[2] = {0u, 0u};
#pragma unroll
    for (int c = 0; c < 2; ++c) {
#pragma unroll
        for (int f = 0; f < 12; ++f) lsum[c][f] = 0.0;
#pragma unroll
        for (int f = 0; f < 5; ++f) lcnt[c][f] = 0u;
    }

    const long ntiles = (a.rows + 63) / 64;
    for (long t = (long)blockIdx.x * kWaves + wave; t < ntiles; t += (long)gridDim.x * kWaves) {  // uniform per wave
        const long i = t * 64 + lane;
        bool valid = false, lab_mov = false, lab_still = false;
        float px = 0.f, py = 0.f, pz = 0.f, gx = 0.f, gy = 0.f, gz = 0.f, epe = 0.f;
        int bin = -1;
        if (i < a.rows) {
            valid = a.valid[i] != 0;
            const bool mov = a.moving[i] != 0;
            const bool lab = a.label == nullptr || a.label[i] != 0;
            lab_mov = mov && valid && lab;
            lab_still = !mov && valid && lab;
            px = pred[i * ps + 0], py = pred[i * ps + 1], pz = pred[i * ps + 2];
            gx = a.gt[i * a.gt_stride + 0], gy = a.gt[i * a.gt_stride + 1], gz = a.gt[i * a.gt_stride + 2];
            epe = norm3(px - gx, py - gy, pz - gz);
            if (a.point_epe) a.point_epe[(long)k * a.rows + i] = epe;
            if (valid && nb > 0) {
                const double r = (double)norm3(a.points[i * a.points_stride + 0], a.points[i * a.points_stride + 1],
                                               a.points[i * a.points_stride + 2]);
                for (int j = 0; j < nb; ++j)
                    if (edges[j] <= r && r < edges[j + 1]) {
                        bin = j;
                        break;
                    }
            }
        }
        if (lab_mov || lab_still) {
            const float gl = norm3(gx, gy, gz);
            const float rel = epe / gl;
            const int c = lab_mov ? 0 : 1;
            const unsigned f1 = (epe < 0.05f) || (rel < 0.05f);
            const unsigned f2 = (epe < 0.1f) || (rel < 0.1f);
            const unsigned f3 = (epe > 0.3f) || (rel > 0.1f);
            const unsigned f4 = (epe > 0.3f) && (rel > 0.3f);
            const float v[12] = {epe, px, py, pz, norm3(px, py, pz), gx, gy, gz, gl, px - gx, py - gy, pz - gz};
#pragma unroll
            for (int cc = 0; cc < 2; ++cc) {
                if (cc == c) {
                    lcnt[cc][0] += 1u, lcnt[cc][1] += f1, lcnt[cc][2] += f2, lcnt[cc][3] += f3, lcnt[cc][4] += f4;
#pragma unroll
                    for (int f = 0; f < 12; ++f) lsum[cc][f] += (double)v[f];
                }
            }
        }
        const bool rng_still = valid && !lab_mov;
        if (rng_still) rsum[0] += (double)epe, rcnt[0] += 1u;
        if (lab_mov) rsum[1] += (double)epe, rcnt[1] += 1u;
        if (nb > 0) {  // (bin >= 0 only for valid rows, which are range "still" or range "moving")
            t_epe[wave][lane] = epe;
            t_slot[wave][lane] = bin < 0 ? -1 : (lab_mov ? 32 : 0) + bin;
            wave_lds_sync();
            for (int j = 0; j < 64; ++j)
                if (t_slot[wave][j] == lane) acc_bin += (double)t_epe[wave][j], cnt_bin += 1u;
            wave_lds_sync();  // (the next tile overwrites the staging rows)
        }
    }

    const int t = threadIdx.x;
    s_bin[wave][lane] = acc_bin;
    c_bin[wave][lane] = cnt_bin;
#pragma unroll
    for (int f = 0; f < 5; ++f) c_stage[t][f] = lcnt[0][f], c_stage[t][5 + f] = lcnt[1][f];
    c_stage[t][10] = rcnt[0], c_stage[t][11] = rcnt[1];
#pragma unroll
    for (int c = 0; c < 2; ++c) {  // round c: the 12 sums of label category c and the EPE sum of range category c
#pragma unroll
        for (int f = 0; f < 12; ++f) s_stage[t][f] = lsum[c][f];
        s_stage[t][12] = rsum[c];
        __syncthreads();
        if (t < 13) {
            double s = 0.0;
            for (int i = 0; i < kThreads; ++i) s += s_stage[i][t];
            s_oth[t < 12 ? c * 12 + t : 24 + c] = s;
        } else if (c == 0 && t >= 64 && t < 64 + 12) {
            unsigned n = 0;
            for (int i = 0; i < kThreads; ++i) n += c_stage[i][t - 64];
            c_oth[t - 64] = n;
        }
        __syncthreads();
    }

    double* rec = a.partials + ((size_t)k * kMaxBlocks + blockIdx.x) * kRec;
    if (t < kSums) {
        double s = 0.0;
        if (t < 64) {
            for (int w = 0; w < kWaves; ++w) s += s_bin[w][t];
        } else if (t < 64 + 26) {
            s = s_oth[t - 64];
        }
        rec[t] = s;
    } else if (t < kRec) {
        const int u = t - kSums;
        uint64_t n = 0;
        if (u < 64) {
            for (int w = 0; w < kWaves; ++w) n += c_bin[w][u];
        } else if (u < 64 + 12) {
            n = c_oth[u - 64];
        }
        reinterpret_cast<uint64_t*>(rec)[t] = n;
    }
}

// one record slot of one flow: lane sums over blocks lane, lane + 64, ... (in order), then the butterfly over the lanes
template <typename T>
__device__ __forceinline__ T slot_total(const double* __restrict__ base, int slot, int n_blocks, int lane) {
    T acc = 0;
    for (int b = lane; b < n_blocks; b += 64) acc += reinterpret_cast<const T*>(base)[(size_t)b * kRec + slot];
    return wave_sum(acc);
}

__global__ __launch_bounds__(kThreads) void flow_metrics_finish_kernel(liso_flow_metrics_result* res, const double* __restrict__ partials,
                                                                       int n_blocks, int n_bins) {
    const int k = blockIdx.y, lane = threadIdx.x & 63;
    const int t = blockIdx.x * kWaves + (threadIdx.x >> 6);  // record slot of this wave
    const double* base = partials + (size_t)k * kMaxBlocks * kRec;
    if (t < kSums) {
        const double s = slot_total<double>(base, t, n_blocks, lane);
        if (lane != 0) return;
        if (t < 64) {
            if (t % 32 < n_bins) res->range_sum[k][t / 32][t % 32] += s;
        } else if (t < kRangeTotalSums) {
            res->label_sum[k][(t - kLabelSums) / 12][(t - kLabelSums) % 12] += s;
        } else if (t < kRangeTotalSums + 2) {
            res->range_sum[k][t - kRangeTotalSums][kMaxBins] += s;
        }
    } else if (t < kRec) {
        const int u = t - kSums;
        const uint64_t n = slot_total<uint64_t>(base, t, n_blocks, lane);
        if (u == kLabelCounts && k == 0) {  // this update's label union empty? (flow 0's moving + still point counts)
            const uint64_t n_still = slot_total<uint64_t>(base, kSums + kLabelCounts + 5, n_blocks, lane);
            if (lane == 0) {
                if (n + n_still == 0) res->empty_overall = 1u;
                res->updates += 1u;
            }
        }
        if (lane != 0) return;
        if (u < 64) {
            if (u % 32 < n_bins) res->range_count[k][u / 32][u % 32] += n;
        } else if (u < kRangeTotalCounts) {
            res->label_count[k][(u - kLabelCounts) / 5][(u - kLabelCounts) % 5] += n;
        } else if (u < kRangeTotalCounts + 2) {
            res->range_count[k][u - kRangeTotalCounts][kMaxBins] += n;
        }
    }
}

__global__ void flow_metrics_reset_kernel(uint64_t* res, int n) {
    for (int i = threadIdx.x; i < n; i += blockDim.x) res[i] = 0;
}

}  // namespace

static_assert(sizeof(liso_flow_metrics_result) % 16 == 0, "result size");
static_assert(kPartialsOffset % 16 == 0, "partials alignment");

extern "C" {

size_t liso_flow_metrics_state_bytes(void) { return kStateBytes; }

size_t liso_flow_metrics_result_bytes(void) { return sizeof(liso_flow_metrics_result); }

int liso_flow_metrics_reset(void* state, void* stream) {
    if (state == nullptr || ((uintptr_t)state & 15)) return LISO_EINVAL;
    hipLaunchKernelGGL(flow_metrics_reset_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (uint64_t*)state,
                       (int)(sizeof(liso_flow_metrics_result) / sizeof(uint64_t)));
    return hipGetLastError() == hipSuccess ? LISO_OK : LISO_ELAUNCH;
}

int liso_flow_metrics_update(void* state, long rows, const float* points, long points_stride, const float* gt_flow, long gt_stride,
                             int n_flows, const float* pred0, long pred0_stride, const float* pred1, long pred1_stride,
                             const float* pred2, long pred2_stride, const uint8_t* pcl_is_valid, const uint8_t* moving_mask,
                             const uint8_t* has_flow_label, const double* bin_edges, int n_bins, float* point_epe, void* stream) {
    if (state == nullptr || ((uintptr_t)state & 15) || rows < 0 || n_flows < 1 || n_flows > LISO_FLOW_METRICS_MAX_FLOWS) return LISO_EINVAL;
    if (n_bins < 0 || n_bins > kMaxBins || (n_bins > 0 && bin_edges == nullptr)) return LISO_EINVAL;
    for (int j = 0; j < n_bins; ++j)
        if (!(bin_edges[j] <= bin_edges[j + 1])) return LISO_EINVAL;  // non-decreasing, no NaN
    const float* pred[3] = {pred0, pred1, pred2};
    const long pstr[3] = {pred0_stride, pred1_stride, pred2_stride};
    Args a{};
    if (rows > 0) {
        if (gt_flow == nullptr || gt_stride < 3 || pcl_is_valid == nullptr || moving_mask == nullptr) return LISO_EINVAL;
        if (n_bins > 0 && (points == nullptr || points_stride < 3)) return LISO_EINVAL;
        for (int f = 0; f < n_flows; ++f)
            if (pred[f] == nullptr || pstr[f] < 3) return LISO_EINVAL;
    }
    a.points = points, a.points_stride = points_stride, a.gt = gt_flow, a.gt_stride = gt_stride;
    for (int f = 0; f < LISO_FLOW_METRICS_MAX_FLOWS; ++f) a.pred[f] = f < n_flows ? pred[f] : nullptr, a.pred_stride[f] = f < n_flows ? pstr[f] : 0;
    a.valid = pcl_is_valid, a.moving = moving_mask, a.label = has_flow_label, a.rows = rows, a.n_bins = n_bins;
    a.point_epe = point_epe;
    a.partials = reinterpret_cast<double*>((char*)state + kPartialsOffset);
    for (int j = 0; j <= kMaxBins; ++j) a.edges.e[j] = j <= n_bins && n_bins > 0 ? bin_edges[j] : 0.0;
    const int nblk = blocks_for(rows);
    hipLaunchKernelGGL(flow_metrics_partials_kernel, dim3(nblk, n_flows), dim3(kThreads), 0, (hipStream_t)stream, a);
    if (hipGetLastError() != hipSuccess) return LISO_ELAUNCH;
    hipLaunchKernelGGL(flow_metrics_finish_kernel, dim3(kRec / kWaves, n_flows), dim3(kThreads), 0, (hipStream_t)stream,
                       (liso_flow_metrics_result*)state, (const double*)a.partials, nblk, n_bins);
    return hipGetLastError() == hipSuccess ? LISO_OK : LISO_ELAUNCH;
}

int liso_flow_metrics_read(const void* state, liso_flow_metrics_result* out, void* stream) {
    if (state == nullptr || ((uintptr_t)state & 15) || out == nullptr) return LISO_EINVAL;
    if (hipMemcpyAsync(out, state, sizeof(liso_flow_metrics_result), hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess)
        return LISO_ELAUNCH;
    return hipStreamSynchronize((hipStream_t)stream) == hipSuccess ? LISO_OK : LISO_ELAUNCH;
}

}  // extern "C"
