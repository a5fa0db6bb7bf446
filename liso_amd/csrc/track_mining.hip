// Track mining on gfx950: the tracks of a batch of tracked sequences selected, refined and exported into the per-frame tables of the
// mined-box database.  C ABI and semantics: include/liso_track_mining.h.  Compiled without FMA contraction: the distances, the
// thresholds they are compared to and the fp64 pose products are the header's expressions, operation by operation.
//
// select : one wavefront per (sequence, track).  The track's rows are compacted in frame order (ballot scan), their confidences and
//          dims staged in LDS; the median and the two quantile neighbours of each dims column are picked by rank (a count over the
//          column, ties by index: a selection, not a full sort -- at most T^2 / 64 comparisons per lane and column).
// apply  : one thread per track row -- the fit's correction, the resize about the nearest bottom corner, the world box.
// export : one workgroup per (sequence, frame) -- the sensor box of row k = frame of every track, then the frame's tracks ranked by a
//          32-bit key (smoothed, T - age, index) held in LDS; every element of every output table is written by exactly one thread.
// The stages are launch bound (a few thousand track rows); what matters is that nothing is read back between them.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/liso_track_mining.h"
#include "dev_common.h"
#include "zero_fill.h"

namespace {

using liso_dev::affine_inv;
using liso_dev::Carver;
using liso_dev::check_launch;
using liso_dev::mat4_mul;

constexpr int kMaxT = LISO_MINE_MAX_FRAMES;
constexpr int kMaxM = LISO_MINE_MAX_TRACKS;
constexpr int kThreads = 256;

struct Tables {
    int32_t* trow;  // [S,M,T] the row of a track's k-th row, -1 behind its age
    size_t bytes;
};

Tables carve(int S, int T, int M, void* base) {
    Tables t;
    Carver ws{base};
    t.trow = ws.take<int32_t>((size_t)S * M * T);
    t.bytes = ws.bytes;
    return t;
}

bool sizes_ok(int S, int T, int K, int cap, int M) {
    return S >= 0 && T >= 1 && T <= kMaxT && K >= 1 && cap >= 1 && M >= 1 && M <= kMaxM && (long)T * K <= (1L << 29) &&
           (double)S * M <= (double)(1L << 30) && (double)S * T <= (double)(1L << 30) &&  // one block per track / per frame
           (double)S * T * ((double)M + cap + K) <= (double)(1L << 36);
}

// the yaw-only pose of Shape.get_poses
__device__ __forceinline__ void pose_of(double x, double y, double z, double yaw, double* P) {
    const double c = cos(yaw), s = sin(yaw);
    P[0] = c, P[1] = -s, P[2] = 0.0, P[3] = x;
    P[4] = s, P[5] = c, P[6] = 0.0, P[7] = y;
    P[8] = 0.0, P[9] = 0.0, P[10] = 1.0, P[11] = z;
    P[12] = 0.0, P[13] = 0.0, P[14] = 0.0, P[15] = 1.0;
}

// pos / rot of inv(W) @ pose(x, y, z, yaw)
__device__ void into_sensor(const double* W, double x, double y, double z, double yaw, double* pos, double* rot) {
    double Wi[16], P[16], R[16];
    affine_inv(W, Wi);
    pose_of(x, y, z, yaw, P);
    mat4_mul(Wi, P, R);
    pos[0] = R[3], pos[1] = R[7], pos[2] = R[11];
    *rot = atan2(R[4], R[0]);
}

struct SelectArgs {
    int T, K, cap, M;
    const int64_t* rows;
    const double *pos_world, *rot_world;
    const int32_t* src;
    const double* w_T;
    const float *boxes, *conf;
    int min_track_age;
    float conf_threshold;
    double min_speed, dt;
    int is_fcd;
    double min_travel, min_dist_smooth;
    int use_smoothing;
    double q;
    int32_t *age, *start;
    float* median_conf;
    double* dist;
    uint8_t* verdict;
    float* refined_dims;
    double *world_raw_pos, *world_raw_rot, *sensor_raw_pos, *sensor_raw_rot;
    float *raw_dims, *raw_probs, *fit_boxes;
    int32_t* trow;
};

__global__ __launch_bounds__(64) void select_kernel(SelectArgs a) {
    __shared__ float vals[4][kMaxT];  // confidence, dx, dy, dz of the track's rows
    __shared__ int lrow[kMaxT];
    __shared__ float picked[7];  // median; lo, hi of each dims column
    const int T = a.T, K = a.K, cap = a.cap, M = a.M;
    const int s = blockIdx.x / M, m = blockIdx.x % M, lane = threadIdx.x;
    const size_t sm = (size_t)s * M + m;
    const unsigned long long below = (1ull << lane) - 1ull;
    const int64_t* rows = a.rows + sm * T;
    int32_t* trow = a.trow + sm * T;
    // ---- the track's rows in frame order
    int age = 0, start = 0;
    for (int t0 = 0; t0 < T; t0 += 64) {
        const int t = t0 + lane;
        const int64_t r = t < T ? rows[t] : -1;
        const bool present = r >= 0 && r < cap;
        const unsigned long long bal = __ballot(present);
        if (present) lrow[age + __popcll(bal & below)] = (int)r;
        if (age == 0 && bal) start = t0 + __ffsll((long long)bal) - 1;
        age += __popcll(bal);
    }
    __syncthreads();
    for (int k = lane; k < T; k += 64) trow[k] = k < age ? lrow[k] : -1;
    const size_t frame0 = (size_t)s * T;
    for (int k = lane; k < age; k += 64) {
        const size_t at = (frame0 + start + k) * cap + lrow[k];
        const int sf = a.src[2 * at], sk = a.src[2 * at + 1];
        const bool det = sf >= 0 && sf < T && sk >= 0 && sk < K;  // (a blank row has no detection: zeros)
        const size_t from = (frame0 + (det ? sf : 0)) * K + (det ? sk : 0);
        vals[0][k] = det ? a.conf[from] : 0.f;
        for (int c = 0; c < 3; ++c) vals[1 + c][k] = det ? a.boxes[from * 7 + 3 + c] : 0.f;
    }
    __syncthreads();
    // ---- order statistics by rank
    const double qpos = age > 0 ? a.q * (double)(age - 1) : 0.0;
    const int lo = (int)floor(qpos), hi = (int)ceil(qpos), mid = age > 0 ? (age - 1) / 2 : 0;
    const float frac = (float)(qpos - (double)lo);
    for (int col = 0; col < 4; ++col) {
        const float* v = vals[col];
        for (int k = lane; k < age; k += 64) {
            const float mine = v[k];
            int rank = 0;
            for (int j = 0; j < age; ++j) rank += (v[j] < mine || (v[j] == mine && j < k)) ? 1 : 0;
            if (col == 0) {
                if (rank == mid) picked[0] = mine;
            } else {
                if (rank == lo) picked[2 * col - 1] = mine;
                if (rank == hi) picked[2 * col] = mine;
            }
        }
    }
    __syncthreads();
    // ---- the verdict (every lane computes the same)
    float median = 0.f;
    double dist = 0.0;
    float refined[3] = {0.f, 0.f, 0.f};
    if (age > 0) {
        median = picked[0];
        for (int c = 0; c < 3; ++c) {
            const float vlo = picked[2 * c + 1], vhi = picked[2 * c + 2];
            refined[c] = vlo + (vhi - vlo) * frac;
        }
        const size_t first = (frame0 + start) * cap + lrow[0], last = (frame0 + start + age - 1) * cap + lrow[age - 1];
        const double dx = a.pos_world[3 * last] - a.pos_world[3 * first], dy = a.pos_world[3 * last + 1] - a.pos_world[3 * first + 1];
        dist = sqrt(dx * dx + dy * dy);
    }
    int verdict = 0;
    if (age > 0 && age >= a.min_track_age) {
        verdict |= LISO_MINE_AGE_OK;
        if (median >= a.conf_threshold) {
            verdict |= LISO_MINE_CONF_OK;
            bool keep = true;
            if (a.min_speed > 0.0) keep = dist / ((double)age * a.dt) >= a.min_speed;
            if (keep && a.is_fcd) keep = dist >= a.min_travel;
            if (keep) {
                verdict |= LISO_MINE_KEPT;
                if (dist > a.min_dist_smooth && a.use_smoothing && age >= LISO_MINE_MIN_TRACK_LEN_FOR_SMOOTHING) verdict |= LISO_MINE_SMOOTHED;
            }
        }
    }
    if (lane == 0) {
        a.age[sm] = age, a.start[sm] = start, a.median_conf[sm] = median, a.dist[sm] = dist, a.verdict[sm] = (uint8_t)verdict;
        for (int c = 0; c < 3; ++c) a.refined_dims[3 * sm + c] = refined[c];
    }
    // ---- the raw boxes of a kept track's rows, and its entries of the per-frame box lists
    const bool kept = verdict & LISO_MINE_KEPT;
    const float nanf_ = nanf("");
    for (int k = lane; k < T; k += 64) {
        const size_t o = sm * T + k;
        const bool row = kept && k < age;
        double wp[3] = {0.0, 0.0, 0.0}, wr = 0.0, sp[3] = {0.0, 0.0, 0.0}, sr = 0.0;
        float d[3] = {0.f, 0.f, 0.f}, p = 0.f;
        if (row) {
            const size_t at = (frame0 + start + k) * cap + lrow[k];
            for (int c = 0; c < 3; ++c) wp[c] = a.pos_world[3 * at + c], d[c] = vals[1 + c][k];
            wr = a.rot_world[at], p = vals[0][k];
            into_sensor(a.w_T + (frame0 + start + k) * 16, wp[0], wp[1], wp[2], wr, sp, &sr);
            float* fb = a.fit_boxes + ((frame0 + start + k) * M + m) * 7;
            for (int c = 0; c < 3; ++c) fb[c] = (float)sp[c], fb[3 + c] = d[c];
            fb[6] = (float)sr;
        }
        for (int c = 0; c < 3; ++c) a.world_raw_pos[3 * o + c] = wp[c], a.sensor_raw_pos[3 * o + c] = sp[c], a.raw_dims[3 * o + c] = d[c];
        a.world_raw_rot[o] = wr, a.sensor_raw_rot[o] = sr, a.raw_probs[o] = p;
        // (k as a frame index:) the frames in which this track contributes no box
        if (!(kept && k >= start && k < start + age)) {
            float* fb = a.fit_boxes + ((frame0 + k) * M + m) * 7;
            for (int c = 0; c < 7; ++c) fb[c] = nanf_;
        }
    }
}

struct ApplyArgs {
    int S, T, M;
    const uint8_t* verdict;
    const int32_t *age, *start;
    const float* median_conf;
    const double* dist;
    const float* refined_dims;
    const double *sensor_raw_pos, *sensor_raw_rot;
    const float* raw_dims;
    const double* w_T;
    const int32_t* fit_count;
    const double* fit;
    int fit_rot, fit_pos;
    double dt;
    double *sensor_pos, *sensor_rot, *world_pos, *world_rot;
    float *dims, *probs, *velo;
};

__global__ __launch_bounds__(kThreads) void apply_kernel(ApplyArgs a) {
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    const int T = a.T, M = a.M;
    if (i >= (size_t)a.S * M * T) return;
    const int k = (int)(i % T);
    const size_t sm = i / T;
    const int s = (int)(sm / M), m = (int)(sm % M);
    const int verdict = a.verdict[sm], age = a.age[sm], start = a.start[sm];
    double sp[3] = {0.0, 0.0, 0.0}, sr = 0.0, wp[3] = {0.0, 0.0, 0.0}, wr = 0.0;
    float nd[3] = {0.f, 0.f, 0.f}, probs = 0.f, velo = 0.f;
    if ((verdict & LISO_MINE_KEPT) && k < age) {
        const size_t frame = (size_t)s * T + start + k;
        float d[3];
        for (int c = 0; c < 3; ++c) sp[c] = a.sensor_raw_pos[3 * i + c], d[c] = a.raw_dims[3 * i + c], nd[c] = a.refined_dims[3 * sm + c];
        sr = a.sensor_raw_rot[i];
        if (a.fit_count && a.fit_count[frame * M + m] > 0) {
            const double* f = a.fit + (frame * M + m) * 5;
            if (a.fit_rot) sr = sr + (f[4] - sr);
            if (a.fit_pos) sp[0] = f[0], sp[1] = f[1];
        }
        // the bottom corner nearest the sensor stays where it is
        const double c = cos(sr), sn = sin(sr);
        const float sx[4] = {0.5f, 0.5f, -0.5f, -0.5f}, sy[4] = {-0.5f, 0.5f, -0.5f, 0.5f};
        double best = 0.0, cx = 0.0, cy = 0.0;
        for (int q = 0; q < 4; ++q) {
            const double ux = (double)(sx[q] * d[0]), uy = (double)(sy[q] * d[1]);
            const double x = (c * ux + (-sn) * uy) + sp[0], y = (sn * ux + c * uy) + sp[1];
            const double r = sqrt(x * x + y * y);
            if (q == 0 || r < best) best = r, cx = x, cy = y;
        }
        const double corner[3] = {cx, cy, (double)(-0.5f * d[2]) + sp[2]};
        for (int q = 0; q < 3; ++q) sp[q] = corner[q] + (double)(nd[q] / d[q]) * (sp[q] - corner[q]);
        double P[16], R[16];
        pose_of(sp[0], sp[1], sp[2], sr, P);
        mat4_mul(a.w_T + frame * 16, P, R);
        wp[0] = R[3], wp[1] = R[7], wp[2] = R[11];
        wr = atan2(R[4], R[0]);
        probs = a.median_conf[sm];
        if (!(verdict & LISO_MINE_SMOOTHED)) velo = (float)a.dist[sm] / ((float)age * (float)a.dt);
    }
    for (int c = 0; c < 3; ++c) a.sensor_pos[3 * i + c] = sp[c], a.world_pos[3 * i + c] = wp[c], a.dims[3 * i + c] = nd[c];
    a.sensor_rot[i] = sr, a.world_rot[i] = wr, a.probs[i] = probs, a.velo[i] = velo;
}

struct ExportArgs {
    int T, K, cap, M, cap_out;
    const uint8_t* verdict;
    const int32_t *age, *start;
    const double *world_pos, *world_rot;
    const float *dims, *probs, *velo;
    const double* w_T;
    const int32_t* src;
    const uint8_t* in_fov;
    int fov_only;
    double *sensor_pos, *sensor_rot;
    int32_t* n_boxes;
    double *out_pos, *out_rot;
    float *out_dims, *out_probs, *out_velo;
    int64_t* out_track_id;
    double* out_T;
    float* max_conf;
    uint8_t* out_valid;
    int32_t* overflow;
    const int32_t* trow;
};

__global__ __launch_bounds__(kThreads) void export_kernel(ExportArgs a) {
    __shared__ int key[kMaxM];  // (smoothed, T - age, index) of the tracks with a row in this frame, -1 for the others
    __shared__ float wave_max[kThreads / 64];
    __shared__ int total;
    const int T = a.T, K = a.K, cap = a.cap, M = a.M, cap_out = a.cap_out;
    const int s = blockIdx.x / T, t = blockIdx.x % T, tid = threadIdx.x;
    const size_t frame0 = (size_t)s * T;
    if (tid == 0) total = 0;
    // ---- row k = t of every track: the sensor box from the world box
    for (int m = tid; m < M; m += kThreads) {
        const size_t sm = (size_t)s * M + m, i = sm * T + t;
        const int verdict = a.verdict[sm], age = a.age[sm], start = a.start[sm];
        double sp[3] = {0.0, 0.0, 0.0}, sr = 0.0;
        if ((verdict & LISO_MINE_KEPT) && t < age)
            into_sensor(a.w_T + (frame0 + start + t) * 16, a.world_pos[3 * i], a.world_pos[3 * i + 1], a.world_pos[3 * i + 2], a.world_rot[i], sp, &sr);
        for (int c = 0; c < 3; ++c) a.sensor_pos[3 * i + c] = sp[c];
        a.sensor_rot[i] = sr;
    }
    // ---- the tracks of frame t
    int mine = 0;
    for (int m = tid; m < M; m += kThreads) {
        const size_t sm = (size_t)s * M + m;
        const int verdict = a.verdict[sm], age = a.age[sm], k = t - a.start[sm];
        bool in = (verdict & LISO_MINE_KEPT) && k >= 0 && k < age;
        if (in && a.fov_only) {
            const int r = a.trow[sm * T + k];
            const size_t at = (frame0 + t) * cap + (r >= 0 && r < cap ? r : 0);
            const int sf = a.src[2 * at], sk = a.src[2 * at + 1];
            in = r >= 0 && r < cap && sf >= 0 && sf < T && sk >= 0 && sk < K && a.in_fov[(frame0 + sf) * K + sk] != 0;
        }
        key[m] = in ? ((((verdict & LISO_MINE_SMOOTHED) ? 1 : 0) << 24) | ((T - age) << 13) | m) : -1;
        mine += in ? 1 : 0;
    }
    __syncthreads();
    if (mine) atomicAdd(&total, mine);
    float best = -INFINITY;
    const size_t o0 = (frame0 + t) * cap_out;
    for (int m = tid; m < M; m += kThreads) {
        const int mykey = key[m];
        if (mykey < 0) continue;
        int rank = 0;
        for (int j = 0; j < M; ++j) rank += (key[j] >= 0 && key[j] < mykey) ? 1 : 0;
        if (rank >= cap_out) continue;
        const size_t sm = (size_t)s * M + m, i = sm * T + (t - a.start[sm]), o = o0 + rank;
        double sp[3], sr;
        into_sensor(a.w_T + (frame0 + t) * 16, a.world_pos[3 * i], a.world_pos[3 * i + 1], a.world_pos[3 * i + 2], a.world_rot[i], sp, &sr);
        for (int c = 0; c < 3; ++c) a.out_pos[3 * o + c] = sp[c], a.out_dims[3 * o + c] = a.dims[3 * i + c];
        a.out_rot[o] = sr, a.out_probs[o] = a.probs[i], a.out_velo[o] = a.velo[i], a.out_track_id[o] = m + 1, a.out_valid[o] = 1;
        pose_of(sp[0], sp[1], sp[2], sr, a.out_T + 16 * o);
        best = fmaxf(best, a.probs[i]);
    }
    for (int sh = 32; sh > 0; sh >>= 1) best = fmaxf(best, __shfl_xor(best, sh));
    if ((tid & 63) == 0) wave_max[tid >> 6] = best;
    __syncthreads();
    const int n = min(total, cap_out);
    for (int r = n + tid; r < cap_out; r += kThreads) {
        const size_t o = o0 + r;
        for (int c = 0; c < 3; ++c) a.out_pos[3 * o + c] = 0.0, a.out_dims[3 * o + c] = 0.f;
        a.out_rot[o] = 0.0, a.out_probs[o] = 0.f, a.out_velo[o] = 0.f, a.out_track_id[o] = -1, a.out_valid[o] = 0;
        for (int c = 0; c < 16; ++c) a.out_T[16 * o + c] = 0.0;
    }
    if (tid == 0) {
        float mx = wave_max[0];
        for (int w = 1; w < kThreads / 64; ++w) mx = fmaxf(mx, wave_max[w]);
        a.n_boxes[frame0 + t] = n, a.max_conf[frame0 + t] = mx;
        if (total > cap_out) atomicAdd(a.overflow + s, total - cap_out);  // (an integer sum: the order does not matter)
    }
}

}  // namespace

extern "C" {

size_t liso_track_mining_workspace_bytes(int n_seq, int max_frames, int max_det, int cap, int max_tracks) {
    if (!sizes_ok(n_seq, max_frames, max_det, cap, max_tracks)) return 0;
    return carve(n_seq, max_frames, max_tracks, nullptr).bytes + 256;  // never 0 for valid sizes
}

int liso_select_tracks(int n_seq, int max_frames, int max_det, int cap, int max_tracks, const int64_t* rows, const double* pos_world,
                       const double* rot_world, const int32_t* src, const double* w_T_sensor, const float* boxes, const float* conf,
                       int min_track_age, float conf_threshold, double min_speed, double dt, int is_flow_cluster_detector,
                       double min_travel_dist, double min_dist_for_smoothing, int use_track_smoothing, double dims_quantile,
                       int32_t* age, int32_t* start, float* median_conf, double* dist, uint8_t* verdict, float* refined_dims,
                       double* world_raw_pos, double* world_raw_rot, double* sensor_raw_pos, double* sensor_raw_rot, float* raw_dims,
                       float* raw_probs, float* fit_boxes, void* workspace, size_t workspace_bytes, void* stream) {
    const int S = n_seq, T = max_frames, K = max_det, M = max_tracks;
    if (!sizes_ok(S, T, K, cap, M) || !(dims_quantile >= 0.0 && dims_quantile <= 1.0)) return LISO_EINVAL;
    if (S == 0) return LISO_OK;
    if (!rows || !pos_world || !rot_world || !src || !w_T_sensor || !boxes || !conf) return LISO_EINVAL;
    if (!age || !start || !median_conf || !dist || !verdict || !refined_dims || !world_raw_pos || !world_raw_rot || !sensor_raw_pos ||
        !sensor_raw_rot || !raw_dims || !raw_probs || !fit_boxes)
        return LISO_EINVAL;
    if (!workspace || ((uintptr_t)workspace & 7) != 0) return LISO_EINVAL;
    const Tables tb = carve(S, T, M, workspace);
    if (workspace_bytes < tb.bytes + 256) return LISO_EWORKSPACE;
    const SelectArgs a = {T, K, cap, M, rows, pos_world, rot_world, src, w_T_sensor, boxes, conf, min_track_age, conf_threshold, min_speed, dt,
                          is_flow_cluster_detector, min_travel_dist, min_dist_for_smoothing, use_track_smoothing, dims_quantile, age, start,
                          median_conf, dist, verdict, refined_dims, world_raw_pos, world_raw_rot, sensor_raw_pos, sensor_raw_rot, raw_dims,
                          raw_probs, fit_boxes, tb.trow};
    select_kernel<<<(unsigned)((size_t)S * M), 64, 0, (hipStream_t)stream>>>(a);
    return check_launch();
}

int liso_refine_tracks_apply(int n_seq, int max_frames, int max_tracks, const uint8_t* verdict, const int32_t* age, const int32_t* start,
                             const float* median_conf, const double* dist, const float* refined_dims, const double* sensor_raw_pos,
                             const double* sensor_raw_rot, const float* raw_dims, const double* w_T_sensor, const int32_t* fit_count,
                             const double* fit, int fit_rot, int fit_pos, double dt, double* sensor_pos, double* sensor_rot,
                             double* world_pos, double* world_rot, float* dims, float* probs, float* velo, void* stream) {
    const int S = n_seq, T = max_frames, M = max_tracks;
    if (!sizes_ok(S, T, 1, 1, M)) return LISO_EINVAL;
    if (S == 0) return LISO_OK;
    if (!verdict || !age || !start || !median_conf || !dist || !refined_dims || !sensor_raw_pos || !sensor_raw_rot || !raw_dims || !w_T_sensor)
        return LISO_EINVAL;
    if ((fit_count == nullptr) != (fit == nullptr) || ((fit_rot || fit_pos) && !fit)) return LISO_EINVAL;
    if (!sensor_pos || !sensor_rot || !world_pos || !world_rot || !dims || !probs || !velo) return LISO_EINVAL;
    const ApplyArgs a = {S, T, M, verdict, age, start, median_conf, dist, refined_dims, sensor_raw_pos, sensor_raw_rot, raw_dims, w_T_sensor,
                         fit_count, fit, fit_rot, fit_pos, dt, sensor_pos, sensor_rot, world_pos, world_rot, dims, probs, velo};
    const size_t n = (size_t)S * M * T;
    apply_kernel<<<(unsigned)((n + kThreads - 1) / kThreads), kThreads, 0, (hipStream_t)stream>>>(a);
    return check_launch();
}

int liso_export_tracks(int n_seq, int max_frames, int max_det, int cap, int max_tracks, int cap_out, const uint8_t* verdict,
                       const int32_t* age, const int32_t* start, const double* world_pos, const double* world_rot, const float* dims,
                       const float* probs, const float* velo, const double* w_T_sensor, const int32_t* src, const uint8_t* in_fov,
                       int fov_only, double* sensor_pos, double* sensor_rot, int32_t* n_boxes, double* out_pos, double* out_rot,
                       float* out_dims, float* out_probs, float* out_velo, int64_t* out_track_id, double* out_lidar_T_box,
                       float* max_conf, uint8_t* out_valid, int32_t* overflow, void* workspace, size_t workspace_bytes, void* stream) {
    const int S = n_seq, T = max_frames, K = max_det, M = max_tracks;
    if (!sizes_ok(S, T, K, cap, M) || cap_out < 1 || (double)S * T * cap_out > (double)(1L << 36)) return LISO_EINVAL;
    if (S == 0) return LISO_OK;
    if (!verdict || !age || !start || !world_pos || !world_rot || !dims || !probs || !velo || !w_T_sensor) return LISO_EINVAL;
    if (fov_only && (!in_fov || !src)) return LISO_EINVAL;
    if (!sensor_pos || !sensor_rot || !n_boxes || !out_pos || !out_rot || !out_dims || !out_probs || !out_velo || !out_track_id ||
        !out_lidar_T_box || !max_conf || !out_valid || !overflow)
        return LISO_EINVAL;
    if (!workspace || ((uintptr_t)workspace & 7) != 0) return LISO_EINVAL;
    const Tables tb = carve(S, T, M, workspace);
    if (workspace_bytes < tb.bytes + 256) return LISO_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    if (liso_zero::zero_async(overflow, (size_t)S * sizeof(int32_t), st) != hipSuccess) return LISO_ELAUNCH;
    const ExportArgs a = {T, K, cap, M, cap_out, verdict, age, start, world_pos, world_rot, dims, probs, velo, w_T_sensor, src, in_fov, fov_only,
                          sensor_pos, sensor_rot, n_boxes, out_pos, out_rot, out_dims, out_probs, out_velo, out_track_id, out_lidar_T_box,
                          max_conf, out_valid, overflow, tb.trow};
    export_kernel<<<(unsigned)((size_t)S * T), kThreads, 0, st>>>(a);
    return check_launch();
}

}  // extern "C"
