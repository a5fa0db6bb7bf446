// Detections -> tracker tables for every frame of many padded sequences (gfx950).  C ABI, reference lines and the arithmetic of
// every step: include/liso_frame_prep.h.
//
// frame_points_kernel: one block = one chunk of kChunk points of one frame x one tile of kTile boxes held in LDS (the rows of
// box_inside.h, read as LDS broadcasts: every lane of a wavefront tests the same box against its own point).  The fp32 circle
// rejects most (point, box) pairs; a pair that passes takes both exact tests.  A box's counts are formed per wavefront (ballot)
// and added to LDS by one lane, the flow of a point inside goes to LDS as 2^-24 m int64; the block then STORES its sums of the
// chunk -- zeros included -- so nothing in HBM is accumulated across blocks and nothing has to be cleared beforehand.
// frame_finalize_kernel: one block per frame adds the chunks (integers: any order gives the same sum), decides, compacts in
// rounds of 256 boxes (ballot prefix within a wavefront, wavefront totals through LDS) and writes the rows.
// 20 frames x 120k points x 100 boxes: 59 chunks x 1 tile x 20 frames = 1180 blocks of 256 threads (256 CUs).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/liso_frame_prep.h"
#include "box_inside.h"
#include "dev_common.h"

namespace {

using liso_box::BoxRow;
using liso_box::PreRow;
using liso_box::inside;
using liso_dev::Carver;

constexpr int kThreads = 256;
constexpr int kTile = 128;                     // boxes per block (LDS tile)
constexpr int kChunk = LISO_FRAME_PREP_CHUNK;  // points per block
constexpr double kFixedScale = 16777216.0;     // 2^24 per metre, as box_points.hip
// the camera's opening angles of count_box_points_in_kitti_annotated_fov (eval_ours.py:98-107), compared in fp32
constexpr float kFovMin = (float)(-41.95 / 180.0 * 3.141592653589793);
constexpr float kFovMax = (float)(40.16 / 180.0 * 3.141592653589793);

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

struct Sizes {
    int S, T, P, cap;
};

// FOV = false: cnt0 <- precision-0 count, cnt1 <- precision-1 count, fsum <- flow sums of the precision-1 points that are valid.
// FOV = true: cnt0 <- precision-0 count of the points inside the camera's opening angle; cnt1, fsum, point_valid, flow unused.
// Partial tables: [frame][chunk][P] (fsum: x 3).
template <bool FOV>
__global__ __launch_bounds__(kThreads) void frame_points_kernel(Sizes z, long N, int stride, int chunks,
                                                                const int32_t* __restrict__ n_frames, const int32_t* __restrict__ n_box,
                                                                const float* __restrict__ boxes, const float* __restrict__ clouds,
                                                                const int32_t* __restrict__ counts, const uint8_t* __restrict__ point_valid,
                                                                const float* __restrict__ flow, int* __restrict__ cnt0,
                                                                int* __restrict__ cnt1, long long* __restrict__ fsum,
                                                                int32_t* __restrict__ overflow) {
    __shared__ BoxRow rows[kTile];
    __shared__ PreRow pre[kTile];  // .count: the precision-0 count
    __shared__ int c1[kTile];
    __shared__ long long fs[kTile][3];
    const int f = blockIdx.z, s = f / z.T, t = f - s * z.T;
    const int tid = threadIdx.x, lane = tid & 63;
    // the only table the last launch accumulates across blocks is cleared here, a launch earlier
    if (!FOV && overflow != nullptr && t == 0 && blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) overflow[s] = 0;
    if (t >= clampi(n_frames[s], z.T)) return;
    const int nb = clampi(n_box[f], z.P), tile0 = blockIdx.y * kTile;
    if (tile0 >= nb) return;
    const int tk = min(kTile, nb - tile0);
    if (tid < tk) {
        liso_box::make_box_row(boxes + ((size_t)f * z.P + tile0 + tid) * 7, 1.0f, rows[tid], pre[tid]);
        c1[tid] = 0;
        fs[tid][0] = fs[tid][1] = fs[tid][2] = 0;
    }
    __syncthreads();
    const long np = counts[f] < 0 ? 0 : ((long)counts[f] > N ? N : (long)counts[f]);
    const long base = (long)blockIdx.x * kChunk;
    for (int it = 0; it < kChunk / kThreads; ++it) {
        const long i0 = base + (long)it * kThreads;
        if (i0 >= np) break;  // (the same for every thread of the block)
        const long i = i0 + tid;  // consecutive lanes read consecutive rows
        bool live = i < np;
        float px = 0.f, py = 0.f, pz = 0.f;
        long long fx[3] = {0, 0, 0};
        if (live) {
            const float* p = clouds + ((size_t)f * N + i) * stride;
            px = p[0], py = p[1], pz = p[2];
            live = isfinite(px) && isfinite(py) && isfinite(pz);
            if (FOV) {
                const float a = atan2f(py, px);
                live = live && a >= kFovMin && a <= kFovMax;
            } else if (live && point_valid[(size_t)f * N + i]) {
                const float* fl = flow + ((size_t)f * N + i) * 3;
                for (int a = 0; a < 3; ++a) fx[a] = isfinite(fl[a]) ? (long long)llrint((double)fl[a] * kFixedScale) : 0;
            }
        }
        for (int j = 0; j < tk; ++j) {
            const float ex = px - pre[j].x, ey = py - pre[j].y;
            bool in0 = false, in1 = false;
            if (live && ex * ex + ey * ey < pre[j].r2) {
                in0 = inside<0>(rows[j], px, py, pz);
                if (!FOV) in1 = inside<1>(rows[j], px, py, pz);
            }
            const unsigned long long m0 = __ballot(in0), m1 = FOV ? 0ull : __ballot(in1);
            if (m0 | m1) {  // rare: a point lies in at most a few boxes
                if (lane == 0) {
                    if (m0) atomicAdd(&pre[j].count, __popcll(m0));
                    if (m1) atomicAdd(&c1[j], __popcll(m1));
                }
                if (in1)
                    for (int a = 0; a < 3; ++a)
                        if (fx[a] != 0) atomicAdd((unsigned long long*)&fs[j][a], (unsigned long long)fx[a]);
            }
        }
    }
    __syncthreads();
    if (tid < tk) {
        const size_t o = ((size_t)f * chunks + blockIdx.x) * z.P + tile0 + tid;
        cnt0[o] = pre[tid].count;
        if (!FOV) {
            cnt1[o] = c1[tid];
            for (int a = 0; a < 3; ++a) fsum[3 * o + a] = fs[tid][a];
        }
    }
}

struct Out {
    int32_t* n_det;
    float* boxes;
    double* rot;
    float* conf;
    double* velo;
    double* into_prev;
    double* into_next;
    uint8_t* in_fov;
    int32_t* src;
    int32_t* n_points;
    float* mean_flow;
    int32_t* dropped_bev;
    int32_t* dropped_points;
    int32_t* overflow;
};

__device__ void blank_row(const Out& o, size_t r) {
    for (int a = 0; a < 7; ++a) o.boxes[7 * r + a] = 0.f;
    o.rot[r] = 0.0;
    o.conf[r] = 0.f;
    for (int a = 0; a < 3; ++a) o.velo[3 * r + a] = 0.0, o.mean_flow[3 * r + a] = 0.f;
    for (int a = 0; a < 16; ++a) o.into_prev[16 * r + a] = 0.0, o.into_next[16 * r + a] = 0.0;
    o.in_fov[r] = 0;
    o.src[r] = -1;
    o.n_points[r] = 0;
}

__global__ __launch_bounds__(kThreads) void frame_finalize_kernel(Sizes z, liso_frame_prep_cfg c, int chunks, int fov_chunks,
                                                                  const int32_t* __restrict__ n_frames, const int32_t* __restrict__ n_box,
                                                                  const float* __restrict__ boxes, const float* __restrict__ conf,
                                                                  const double* __restrict__ odom, const int* __restrict__ cnt0,
                                                                  const int* __restrict__ cnt1, const long long* __restrict__ fsum,
                                                                  const int* __restrict__ fov_cnt, Out o) {
    __shared__ int wave_kept[kThreads / 64];
    __shared__ int drops[2];
    const int f = blockIdx.x, s = f / z.T, t = f - s * z.T;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool active = t < clampi(n_frames[s], z.T);
    const int nb = active ? clampi(n_box[f], z.P) : 0;
    if (tid < 2) drops[tid] = 0;
    __syncthreads();
    int kept = 0;  // boxes kept in the rounds so far (the same in every thread)
    for (int j0 = 0; j0 < nb; j0 += kThreads) {
        const int j = j0 + tid;
        const bool have = j < nb;
        bool keep = false, bev_ok = true, pts_ok = true;
        int n0 = 0, n1 = 0, nf = 0;
        long long fl[3] = {0, 0, 0};
        const float* box = boxes + ((size_t)f * z.P + (have ? j : 0)) * 7;
        if (have) {
            for (int g = 0; g < chunks; ++g) {
                const size_t q = ((size_t)f * chunks + g) * z.P + j;
                n0 += cnt0[q], n1 += cnt1[q];
                for (int a = 0; a < 3; ++a) fl[a] += fsum[3 * q + a];
            }
            for (int g = 0; g < fov_chunks; ++g) nf += fov_cnt[((size_t)f * fov_chunks + g) * z.P + j];
            if (c.drop_on_bev_boundaries) {  // is_boxes_clearly_in_bev_range (shape_utils.py:554-555), fp32
                const float half = box[3] / 2.f;
                bev_ok = fabsf(fabsf(box[0]) - half) < c.bev_range_x / 2.f && fabsf(fabsf(box[1]) - half) < c.bev_range_y / 2.f;
            }
            if (c.min_points_in_box > 0) pts_ok = n0 >= c.min_points_in_box;  // tracking.py:798-801
            keep = bev_ok && pts_ok;
        }
        const unsigned long long mk = __ballot(keep), mb = __ballot(have && !bev_ok), mp = __ballot(have && bev_ok && !pts_ok);
        if (lane == 0) {
            wave_kept[wave] = __popcll(mk);
            if (mb) atomicAdd(&drops[0], __popcll(mb));
            if (mp) atomicAdd(&drops[1], __popcll(mp));
        }
        __syncthreads();
        int before = kept, total = 0;
        for (int w = 0; w < kThreads / 64; ++w) {
            if (w < wave) before += wave_kept[w];
            total += wave_kept[w];
        }
        const int dest = before + __popcll(mk & ((1ull << lane) - 1ull));
        if (keep && dest < z.cap) {
            const size_t r = (size_t)f * z.cap + dest;
            // step 4: the mean of liso_points_in_boxes_f32 (box_points.hip: mean_flow_kernel)
            const float denom = fmaxf((float)n1, 1.f);
            float mean[3];
            for (int a = 0; a < 3; ++a) mean[a] = (float)((double)fl[a] / kFixedScale) / denom;
            // step 5: P = [Rz(yaw) | pos] (Shape.get_poses), F(m) P = P with m added to its translation
            const double x = box[0], y = box[1], zc = box[2], yaw = box[6];
            const double cs = cos(yaw), sn = sin(yaw);
            const double rotm[12] = {cs, -sn, 0.0, 0.0, sn, cs, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0};
            const double pos[3] = {x, y, zc};
            double tn[3];
            for (int a = 0; a < 12; ++a) o.into_next[16 * r + a] = rotm[a], o.into_prev[16 * r + a] = rotm[a];
            for (int a = 0; a < 3; ++a) {
                tn[a] = pos[a] + (double)mean[a];
                o.into_next[16 * r + 4 * a + 3] = tn[a];
                o.into_prev[16 * r + 4 * a + 3] = pos[a] + (double)(-mean[a]);
            }
            for (int a = 0; a < 4; ++a) o.into_next[16 * r + 12 + a] = o.into_prev[16 * r + 12 + a] = a == 3 ? 1.0 : 0.0;
            // step 6: soft_align_box_flip_orientation_with_motion_trafo (shape_utils.py:608-644)
            float yaw32 = box[6];
            double rot = (double)yaw32, disp = 0.0;
            if (c.align) {
                const double* O = odom + (size_t)f * 16;
                double d[3];  // translation of odom * into_next, minus the box position
                for (int a = 0; a < 3; ++a) d[a] = (((O[4 * a] * tn[0] + O[4 * a + 1] * tn[1]) + O[4 * a + 2] * tn[2]) + O[4 * a + 3]) - pos[a];
                double bx = cs * d[0] + sn * d[1], by = cs * d[1] - sn * d[0];  // rows of inv(P) = [Rz^T | -Rz^T pos]
                disp = sqrt(bx * bx + by * by);
                const bool flip = bx < 0.0 && disp > c.no_align_below_m;
                if (flip) bx = -bx, by = -by, yaw32 = yaw32 + 3.14159274101257324f;  // rot + pi in fp32 (:633)
                double ratio = (disp - c.no_align_below_m) / (c.full_align_above_m - c.no_align_below_m);
                ratio = ratio < 0.0 ? 0.0 : (ratio > 1.0 ? 1.0 : ratio);  // (NaN stays NaN, as torch.clip leaves it)
                rot = (double)yaw32 + ratio * atan2(by, bx);
            }
            for (int a = 0; a < 6; ++a) o.boxes[7 * r + a] = box[a];
            o.boxes[7 * r + 6] = (float)rot;
            o.rot[r] = rot;
            o.conf[r] = conf[(size_t)f * z.P + j];
            o.velo[3 * r] = disp, o.velo[3 * r + 1] = 0.0, o.velo[3 * r + 2] = 0.0;
            o.in_fov[r] = fov_cnt != nullptr ? (nf >= c.fov_min_points ? 1 : 0) : 1;
            o.src[r] = j;
            o.n_points[r] = n1;
            for (int a = 0; a < 3; ++a) o.mean_flow[3 * r + a] = mean[a];
        }
        kept += total;
        __syncthreads();  // wave_kept is rewritten by the next round
    }
    const int n_det = min(kept, z.cap);
    for (int r = n_det + tid; r < z.cap; r += kThreads) blank_row(o, (size_t)f * z.cap + r);
    if (tid == 0) {
        o.n_det[f] = n_det;
        o.dropped_bev[f] = drops[0];
        o.dropped_points[f] = drops[1];
        if (kept > z.cap) atomicAdd(&o.overflow[s], kept - z.cap);  // cleared by the first launch; integer: any order, the same sum
    }
}

int chunks_of(long n) { return n <= 0 ? 1 : (int)((n + kChunk - 1) / kChunk); }

struct Plan {
    int* cnt0;
    int* cnt1;
    long long* fsum;
    int* fov;
    size_t bytes;
};

bool sizes_ok(const liso_frame_prep_cfg* c) {
    if (c == nullptr || c->n_seq < 0 || c->max_frames < 1 || c->max_box < 1 || c->max_box > LISO_FRAME_PREP_MAX_BOX || c->cap < 1) return false;
    if ((long)c->n_seq * c->max_frames > 65535) return false;  // one grid layer per frame
    if (c->n_points < 0 || c->point_stride < 3) return false;
    if (c->n_fov_points >= 0 && c->fov_stride < 3) return false;
    if ((c->n_points + kChunk - 1) / kChunk > 0x7fffffffL || (c->n_fov_points + kChunk - 1) / kChunk > 0x7fffffffL) return false;
    return true;
}

Plan plan(const liso_frame_prep_cfg* c, void* base) {
    Carver w{base};
    const size_t rows = (size_t)c->n_seq * c->max_frames * c->max_box;
    Plan p;
    p.cnt0 = w.take<int>(rows * chunks_of(c->n_points));
    p.cnt1 = w.take<int>(rows * chunks_of(c->n_points));
    p.fsum = w.take<long long>(rows * chunks_of(c->n_points) * 3);
    p.fov = c->n_fov_points >= 0 ? w.take<int>(rows * chunks_of(c->n_fov_points)) : nullptr;
    p.bytes = w.bytes > 0 ? w.bytes : 256;  // (an empty batch: a size that is not the refusal)
    return p;
}

}  // namespace

extern "C" size_t liso_frame_prep_workspace_bytes(const liso_frame_prep_cfg* c) {
    if (!sizes_ok(c)) return 0;
    return plan(c, nullptr).bytes;
}

extern "C" int liso_prepare_tracker_frames(const liso_frame_prep_cfg* c, const int32_t* n_frames, const int32_t* n_box, const float* boxes,
                                           const float* conf, const double* odom, const float* clouds, const int32_t* counts,
                                           const uint8_t* point_valid, const float* flow, const float* fov_clouds,
                                           const int32_t* fov_counts, int32_t* n_det, float* out_boxes, double* rot, float* out_conf,
                                           double* velo, double* into_prev, double* into_next, uint8_t* in_fov, int32_t* src,
                                           int32_t* n_points, float* mean_flow, int32_t* dropped_bev, int32_t* dropped_points,
                                           int32_t* overflow, void* workspace, size_t workspace_bytes, void* stream) {
    if (!sizes_ok(c)) return LISO_EINVAL;
    if (c->align && !(c->no_align_below_m < c->full_align_above_m)) return LISO_EINVAL;  // the reference's assert (:618)
    if (c->n_seq == 0) return LISO_OK;
    const bool fov = c->n_fov_points >= 0;
    if (n_frames == nullptr || n_box == nullptr || boxes == nullptr || conf == nullptr || odom == nullptr || counts == nullptr) return LISO_EINVAL;
    if (c->n_points > 0 && (clouds == nullptr || point_valid == nullptr || flow == nullptr)) return LISO_EINVAL;
    if (fov != (fov_counts != nullptr) || (!fov && fov_clouds != nullptr) || (fov && c->n_fov_points > 0 && fov_clouds == nullptr)) return LISO_EINVAL;
    if (n_det == nullptr || out_boxes == nullptr || rot == nullptr || out_conf == nullptr || velo == nullptr || into_prev == nullptr ||
        into_next == nullptr || in_fov == nullptr || src == nullptr || n_points == nullptr || mean_flow == nullptr || dropped_bev == nullptr ||
        dropped_points == nullptr || overflow == nullptr)
        return LISO_EINVAL;
    if (workspace == nullptr || ((uintptr_t)workspace & 255) != 0) return LISO_EINVAL;
    const Plan p = plan(c, workspace);
    if (workspace_bytes < p.bytes) return LISO_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const Sizes z{c->n_seq, c->max_frames, c->max_box, c->cap};
    const int frames = c->n_seq * c->max_frames, tiles = (c->max_box + kTile - 1) / kTile;
    const int chunks = chunks_of(c->n_points), fov_chunks = fov ? chunks_of(c->n_fov_points) : 0;
    hipLaunchKernelGGL(frame_points_kernel<false>, dim3((unsigned)chunks, (unsigned)tiles, (unsigned)frames), dim3(kThreads), 0, st, z,
                       c->n_points, c->point_stride, chunks, n_frames, n_box, boxes, clouds, counts, point_valid, flow, p.cnt0, p.cnt1,
                       p.fsum, overflow);
    if (fov)
        hipLaunchKernelGGL(frame_points_kernel<true>, dim3((unsigned)fov_chunks, (unsigned)tiles, (unsigned)frames), dim3(kThreads), 0, st, z,
                           c->n_fov_points, c->fov_stride, fov_chunks, n_frames, n_box, boxes, fov_clouds, fov_counts,
                           (const uint8_t*)nullptr, (const float*)nullptr, p.fov, (int*)nullptr, (long long*)nullptr, (int32_t*)nullptr);
    const Out o{n_det, out_boxes, rot, out_conf, velo, into_prev, into_next, in_fov, src, n_points, mean_flow, dropped_bev, dropped_points, overflow};
    hipLaunchKernelGGL(frame_finalize_kernel, dim3((unsigned)frames), dim3(kThreads), 0, st, z, *c, chunks, fov_chunks, n_frames, n_box, boxes,
                       conf, odom, p.cnt0, p.cnt1, p.fsum, p.fov, o);
    return liso_dev::check_launch();
}
