// Sequence tracker on gfx950: the boxes of every frame of a sequence associated into tracks, many sequences per call.  C ABI and
// semantics: include/liso_tracking.h (liso_track_sequences).  Compiled without FMA contraction: the world transforms, the fp32
// distance and the constant-velocity step are the header's expressions, operation by operation.
//
// chain : one thread per sequence -- world_T_sensor of every frame, the odometries multiplied up in fp64.
// world : one thread per detection -- world position / yaw, and the fp32 x, y of its two propagated poses in the world.
// walk  : one workgroup per sequence, the frames in order, the state (previous frame, the one before, the one being built) in LDS.
//         Per frame: all threads load the detections and rank the alive rows (confidence descending, row index ascending);
//         wave 0 walks the ranked rows, each pick an argmin on (distance, index) over the free detections, 64 per pass, the taken
//         ones a bit per pass in a register; wave 0 numbers the unmatched detections and packs the lost rows behind the
//         detections (ballot scans).  The forward walk leaves every frame's rows in the workspace; after the backward walk, which
//         only advances the id counter, the carried rows that were re-detected later are appended to their frames by ascending id.
// The walk keeps min(3 K, LISO_TRACK_MAX_CAP) rows per frame whatever the result's `cap` is, so `cap` shortens the tables and never
// changes the tracks.  Three launches, no host read.  The walk is latency bound (one dependent pick per alive row and frame); the
// parallelism is the batch.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/liso_tracking.h"
#include "dev_common.h"
#include "per_device.h"

namespace {

using liso_dev::Carver;
using liso_dev::check_launch;
using liso_dev::mat4_mul;

constexpr int kThreads = 256;
// the constants of liso_amd/tracker/global_box_tracker.py, stated in the header (tests/test_device_tracker_host.py ties the two)
constexpr int kMaxPropagationTime = LISO_TRACK_MAX_PROPAGATION_TIME;
constexpr float kInitialConf = LISO_TRACK_INITIAL_CONF;
constexpr float kMinAliveConf = LISO_TRACK_MIN_ALIVE_CONF;
constexpr float kConfStep = kInitialConf / kMaxPropagationTime;
constexpr int kLost = -1, kDead = -2;     // match[] of a previous row that took no detection: alive / not alive

struct Tables {
    double* w_pos;       // [S,T,K,3] world position of every detection
    double* w_rot;       // [S,T,K]
    float* past_xy;      // [S,T,K,2] into_prev in the world, fp32
    float* next_xy;      // [S,T,K,2] into_next in the world, fp32
    double* st_pos;      // [S,T,rows,3] rows of the forward walk (only the carried rows are written); rows = state_rows(K)
    int32_t* st_id;      // [S,T,rows]
    int32_t* st_src;     // [S,T,rows] frame * K + slot
    int32_t* st_parent;  // [S,T,rows] row of the previous frame a carried row continues, -1 for a detection
    int32_t* st_n;       // [S,T] rows
    uint8_t* st_fill;    // [S,T,rows] carried row of a track that is detected again later
    size_t bytes;
};

// Rows per frame of the walk.  A frame holds its detections and the boxes carried from the previous frame's alive rows, which are
// that frame's detections and the detections of earlier frames carried at most kMaxPropagationTime times: (kMaxPropagationTime + 2) K
// rows always suffice (3 K).  The result's `cap` only
// limits what is written out, so a small `cap` never changes the tracks.
int state_rows(int K) { return (int)std::min<long>((kMaxPropagationTime + 2L) * K, LISO_TRACK_MAX_CAP); }

Tables carve(int S, int T, int K, void* base) {
    const int cap = state_rows(K);
    Tables t;
    Carver ws{base};
    const size_t d = (size_t)S * T * K, r = (size_t)S * T * cap;
    t.w_pos = ws.take<double>(d * 3);
    t.w_rot = ws.take<double>(d);
    t.past_xy = ws.take<float>(d * 2);
    t.next_xy = ws.take<float>(d * 2);
    t.st_pos = ws.take<double>(r * 3);
    t.st_id = ws.take<int32_t>(r);
    t.st_src = ws.take<int32_t>(r);
    t.st_parent = ws.take<int32_t>(r);
    t.st_n = ws.take<int32_t>((size_t)S * T);
    t.st_fill = ws.take<uint8_t>(r);
    t.bytes = ws.bytes;
    return t;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ __launch_bounds__(64) void chain_kernel(int S, int T, const int32_t* n_frames, const double* odom, double* w_T) {
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= S) return;
    const int nf = clampi(n_frames[s], 0, T);
    double cur[16], nxt[16];
    for (int a = 0; a < 16; ++a) cur[a] = (a % 5 == 0) ? 1.0 : 0.0;
    for (int t = 0; t < T; ++t) {
        double* o = w_T + ((size_t)s * T + t) * 16;
        for (int a = 0; a < 16; ++a) o[a] = cur[a];
        if (t + 1 < nf) {
            mat4_mul(cur, odom + ((size_t)s * T + t) * 16, nxt);
            for (int a = 0; a < 16; ++a) cur[a] = nxt[a];
        } else {
            for (int a = 0; a < 16; ++a) cur[a] = (a % 5 == 0) ? 1.0 : 0.0;  // frames behind the sequence: identity
        }
    }
}

// x, y of (W * P)[:, 3], fp64 in matmul order, rounded to fp32
__device__ __forceinline__ void world_xy(const double* W, const double* P, float* xy) {
    xy[0] = (float)(((W[0] * P[3] + W[1] * P[7]) + W[2] * P[11]) + W[3] * P[15]);
    xy[1] = (float)(((W[4] * P[3] + W[5] * P[7]) + W[6] * P[11]) + W[7] * P[15]);
}

__global__ __launch_bounds__(kThreads) void world_kernel(int S, int T, int K, const int32_t* n_frames, const int32_t* n_det,
                                                         const float* boxes, const double* into_prev, const double* into_next,
                                                         const double* w_T, Tables tb) {
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= (size_t)S * T * K) return;
    const int k = (int)(i % K), t = (int)((i / K) % T), s = (int)(i / ((size_t)K * T));
    const int nf = clampi(n_frames[s], 0, T);
    if (t >= nf || k >= clampi(n_det[(size_t)s * T + t], 0, K)) return;
    const double* W = w_T + ((size_t)s * T + t) * 16;
    const float* b = boxes + i * 7;
    const double x = b[0], y = b[1], z = b[2], yaw = b[6];
    for (int r = 0; r < 3; ++r) tb.w_pos[i * 3 + r] = ((W[4 * r] * x + W[4 * r + 1] * y) + W[4 * r + 2] * z) + W[4 * r + 3];
    const double c = cos(yaw), sn = sin(yaw);
    tb.w_rot[i] = atan2(W[4] * c + W[5] * sn, W[0] * c + W[1] * sn);
    const int tp = t > 0 ? t - 1 : 0, tn = t + 1 < nf ? t + 1 : nf - 1;
    world_xy(w_T + ((size_t)s * T + tp) * 16, into_prev + i * 16, tb.past_xy + i * 2);
    world_xy(w_T + ((size_t)s * T + tn) * 16, into_next + i * 16, tb.next_xy + i * 2);
}

// the LDS plan: three frames of state_rows(K) rows (being built, previous, the one before), the current detections' propagated x, y, the
// visiting order of the previous frame's alive rows and what each previous row took
constexpr int kRowBytes = 3 * (3 * 8 + 4 + 4 + 4) + 8 + 4 + 4;
static_assert(kRowBytes * LISO_TRACK_MAX_CAP + 64 <= 160 * 1024, "the LDS plan must hold LISO_TRACK_MAX_CAP rows");

struct Frame {
    double *x, *y, *z;
    int32_t *id, *src;
    float* conf;
};

__global__ __launch_bounds__(kThreads) void walk_kernel(int T, int K, int out_cap, int cap, const int32_t* n_frames, const int32_t* n_det,
                                                        double threshold, Tables tb, int32_t* n_out, int64_t* track_ids,
                                                        double* pos_world, double* rot_world, int32_t* src_out, uint8_t* is_fill,
                                                        int64_t* id_counter, int32_t* overflow) {
    extern __shared__ double lds[];
    __shared__ int sh_alive, sh_counter, sh_rows, sh_over;
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const bool wave0 = tid < 64;
    const unsigned long long below = (1ull << lane) - 1ull;
    int32_t* const ints = (int32_t*)(lds + 9 * (size_t)cap);
    auto frame = [&](int b) {
        Frame f;
        f.x = lds + 3 * (size_t)cap * b, f.y = f.x + cap, f.z = f.y + cap;
        f.id = ints + 3 * (size_t)cap * b, f.src = f.id + cap, f.conf = (float*)(f.src + cap);
        return f;
    };
    int32_t* const w = ints + 9 * (size_t)cap;
    float* det_xy = (float*)w;        // [cap][2] the current detections' propagated x, y
    int32_t* order = w + 2 * (size_t)cap;  // [cap] alive rows of the previous frame in visiting order
    int32_t* match = order + cap;     // [cap] per previous row: the detection it took, kLost or kDead

    const int nf = clampi(n_frames[s], 0, T);
    const size_t row0 = (size_t)s * T;  // first (sequence, frame) row of the per-frame tables
    if (tid == 0) sh_counter = 0, sh_over = 0;
    __syncthreads();

    for (int dir = 0; dir < 2; ++dir) {
        const bool fwd = dir == 0;
        const float* prop = fwd ? tb.past_xy : tb.next_xy;
        int m_prev = 0, m_pp = 0, n_prev = 0;  // rows of the previous frame, of the one before, detections of the previous frame
        for (int f = 0; f < nf; ++f) {
            const int t = fwd ? f : nf - 1 - f, t_prev = fwd ? t - 1 : t + 1;
            const int n_all = clampi(n_det[row0 + t], 0, K), n = min(n_all, cap);
            const Frame cur = frame(f % 3), prev = frame((f + 2) % 3), pp = frame((f + 1) % 3);
            const size_t det0 = (row0 + t) * K;
            const int counter = sh_counter;
            // ---- A: the detections; the visiting order of the previous frame's alive rows
            if (tid == 0) sh_alive = 0;
            for (int k = tid; k < n; k += kThreads) {
                cur.x[k] = tb.w_pos[(det0 + k) * 3], cur.y[k] = tb.w_pos[(det0 + k) * 3 + 1], cur.z[k] = tb.w_pos[(det0 + k) * 3 + 2];
                cur.conf[k] = kInitialConf, cur.src[k] = t * K + k;
                cur.id[k] = f == 0 ? counter + 1 + k : -1;
                det_xy[2 * k] = prop[(det0 + k) * 2], det_xy[2 * k + 1] = prop[(det0 + k) * 2 + 1];
            }
            __syncthreads();
            int alive_mine = 0;
            for (int i = tid; i < m_prev; i += kThreads) {
                const float ci = prev.conf[i];
                if (!(ci >= kMinAliveConf)) {
                    match[i] = kDead;
                    continue;
                }
                int rank = 0;
                for (int j = 0; j < m_prev; ++j) {
                    const float cj = prev.conf[j];
                    rank += (cj >= kMinAliveConf && (cj > ci || (cj == ci && j < i))) ? 1 : 0;
                }
                order[rank] = i, match[i] = kLost, ++alive_mine;
            }
            if (alive_mine) atomicAdd(&sh_alive, alive_mine);
            __syncthreads();
            // ---- B: wave 0 serves the alive rows in order; each takes the nearest free detection, the first index on a tie
            if (wave0 && f > 0) {
                const int n_alive = sh_alive, passes = (n + 63) / 64;
                uint32_t taken = 0;  // bit p: detection p * 64 + lane
                for (int a = 0; a < n_alive; ++a) {
                    const int r = order[a];
                    const float ax = (float)prev.x[r], ay = (float)prev.y[r];
                    float best = INFINITY;
                    int bi = INT_MAX;
                    for (int p = 0; p < passes; ++p) {
                        const int k = p * 64 + lane;
                        if (k < n && !((taken >> p) & 1u)) {
                            const float dx = det_xy[2 * k] - ax, dy = det_xy[2 * k + 1] - ay;
                            const float d = sqrtf(dx * dx + dy * dy);
                            if (d < best) best = d, bi = k;
                        }
                    }
                    for (int sh = 1; sh < 64; sh <<= 1) {
                        const float od = __shfl_xor(best, sh);
                        const int oi = __shfl_xor(bi, sh);
                        if (od < best || (od == best && oi < bi)) best = od, bi = oi;
                    }
                    if ((double)best < threshold) {
                        if ((bi & 63) == lane) taken |= 1u << (bi >> 6);
                        if (lane == 0) match[r] = bi;
                    }
                }
            }
            __syncthreads();
            // ---- C: matched detections inherit the id; a carried row that is taken belongs to a track with a hole
            for (int i = tid; i < m_prev; i += kThreads) {
                const int k = match[i];
                if (k < 0) continue;
                cur.id[k] = prev.id[i];
                if (fwd && i >= n_prev) tb.st_fill[(row0 + t_prev) * cap + i] = 1;
            }
            __syncthreads();
            // ---- D: wave 0 numbers the unmatched detections and packs the lost rows behind the detections
            if (wave0) {
                int born = 0;
                if (f > 0)
                    for (int k0 = 0; k0 < n; k0 += 64) {
                        const int k = k0 + lane;
                        const bool un = k < n && cur.id[k] < 0;
                        const unsigned long long bal = __ballot(un);
                        if (un) cur.id[k] = counter + 1 + born + __popcll(bal & below);
                        born += __popcll(bal);
                    }
                int lost_n = 0;
                for (int i0 = 0; i0 < m_prev; i0 += 64) {
                    const int i = i0 + lane;
                    const bool lost = i < m_prev && match[i] == kLost;
                    const unsigned long long bal = __ballot(lost);
                    const int to = n + lost_n + __popcll(bal & below);
                    lost_n += __popcll(bal);
                    if (lost && to < cap) {
                        double x = prev.x[i], y = prev.y[i], z = prev.z[i];
                        const int id = prev.id[i];
                        for (int j = 0; j < m_pp; ++j)
                            if (pp.id[j] == id) {  // the displacement since the frame before, once more
                                x = x + (x - pp.x[j]), y = y + (y - pp.y[j]), z = z + (z - pp.z[j]);
                                break;
                            }
                        cur.x[to] = x, cur.y[to] = y, cur.z[to] = z, cur.id[to] = id, cur.src[to] = prev.src[i];
                        cur.conf[to] = (0.0001f + prev.conf[i]) - kConfStep;
                        if (fwd) tb.st_parent[(row0 + t) * cap + to] = i;
                    }
                }
                if (lane == 0) {
                    const int want = n_all + lost_n;
                    sh_counter = counter + (f == 0 ? n : born);
                    sh_rows = min(want, cap);
                    if (fwd && want > cap) sh_over += want - cap;
                }
            }
            __syncthreads();
            const int m_cur = sh_rows;
            if (fwd) {  // the frame's rows, for the hole filling
                const size_t r0 = (row0 + t) * cap;
                for (int r = tid; r < m_cur; r += kThreads) {
                    tb.st_id[r0 + r] = cur.id[r], tb.st_src[r0 + r] = cur.src[r], tb.st_fill[r0 + r] = 0;
                    if (r < n) tb.st_parent[r0 + r] = -1;
                    else tb.st_pos[(r0 + r) * 3] = cur.x[r], tb.st_pos[(r0 + r) * 3 + 1] = cur.y[r], tb.st_pos[(r0 + r) * 3 + 2] = cur.z[r];
                }
                if (tid == 0) tb.st_n[row0 + t] = m_cur;
            }
            m_pp = m_prev, m_prev = m_cur, n_prev = n;
            __syncthreads();  // (st_fill of this frame is zero before the next frame marks it; the next frame reuses the tables)
        }
    }

    // ---- holes: a carried row whose own carried continuation is part of a hole is part of it too (longer propagation times)
    for (int t = nf - 1; t >= 1; --t) {
        const size_t r0 = (row0 + t) * cap, q0 = (row0 + t - 1) * cap;
        const int n = min(clampi(n_det[row0 + t], 0, K), cap), n_before = min(clampi(n_det[row0 + t - 1], 0, K), cap);
        for (int r = n + tid; r < tb.st_n[row0 + t]; r += kThreads) {
            const int p = tb.st_parent[r0 + r];
            if (tb.st_fill[r0 + r] && p >= n_before) tb.st_fill[q0 + p] = 1;
        }
        __syncthreads();
    }
    // ---- the result: a frame's detections, then its hole-filling rows by ascending track id, as far as out_cap rows reach; unused
    // rows are blank
    for (int t = 0; t < T; ++t) {
        const size_t r0 = (row0 + t) * cap, o0 = (row0 + t) * out_cap;
        const int n = t < nf ? min(clampi(n_det[row0 + t], 0, K), cap) : 0, m = t < nf ? tb.st_n[row0 + t] : 0;
        int fills_mine = 0;
        if (tid == 0) sh_alive = 0;
        __syncthreads();
        for (int r = tid; r < m; r += kThreads) {  // (r is a row of the walk, `to` a row of the result)
            const bool det = r < n, fill = r >= n && tb.st_fill[r0 + r];
            if (!det && !fill) continue;
            int to = r;
            const int id = tb.st_id[r0 + r], sc = tb.st_src[r0 + r];
            if (fill) {
                to = n, ++fills_mine;
                for (int q = n; q < m; ++q) to += (tb.st_fill[r0 + q] && tb.st_id[r0 + q] < id) ? 1 : 0;
            }
            if (to >= out_cap) continue;
            const size_t o = o0 + to, from = (row0 + sc / K) * K + sc % K;
            track_ids[o] = id, rot_world[o] = tb.w_rot[from], src_out[2 * o] = sc / K, src_out[2 * o + 1] = sc % K, is_fill[o] = fill;
            for (int a = 0; a < 3; ++a) pos_world[3 * o + a] = det ? tb.w_pos[from * 3 + a] : tb.st_pos[(r0 + r) * 3 + a];
        }
        if (fills_mine) atomicAdd(&sh_alive, fills_mine);
        __syncthreads();
        const int rows = n + sh_alive;
        for (int r = rows + tid; r < out_cap; r += kThreads) {
            const size_t o = o0 + r;
            track_ids[o] = -1, rot_world[o] = 0.0, src_out[2 * o] = -1, src_out[2 * o + 1] = -1, is_fill[o] = 0;
            for (int a = 0; a < 3; ++a) pos_world[3 * o + a] = 0.0;
        }
        if (tid == 0) {
            n_out[row0 + t] = min(rows, out_cap);
            if (rows > out_cap) sh_over += rows - out_cap;
        }
        __syncthreads();
    }
    if (tid == 0) id_counter[s] = sh_counter, overflow[s] = sh_over;
}

bool sizes_ok(int S, int T, int K, int cap) {
    return S >= 0 && T >= 1 && K >= 1 && cap >= 1 && cap <= LISO_TRACK_MAX_CAP && (long)T * K <= (1L << 29) &&
           (double)S * T * K <= (double)(1L << 36) &&  // one thread per detection: the grid of 256-thread blocks stays below 2^31
           (double)S * T * ((double)K + cap) <= (double)(1L << 40);
}

liso_dev::PerDeviceFlag g_lds;

}  // namespace

extern "C" {

size_t liso_track_sequences_workspace_bytes(int n_seq, int max_frames, int max_det, int cap) {
    if (!sizes_ok(n_seq, max_frames, max_det, cap)) return 0;
    return carve(n_seq, max_frames, max_det, nullptr).bytes + 256;  // never 0 for valid sizes
}

int liso_track_sequences(int n_seq, int max_frames, int max_det, int cap, const int32_t* n_frames, const int32_t* n_det,
                         const float* boxes, const float* conf, const double* odom, const double* into_prev, const double* into_next,
                         double threshold, int32_t* n_out, int64_t* track_ids, double* pos_world, double* rot_world, int32_t* src,
                         uint8_t* is_fill, double* w_T_sensor, int64_t* id_counter, int32_t* overflow, void* workspace,
                         size_t workspace_bytes, void* stream) {
    (void)conf;  // carried through by `src`; the association does not read it
    const int S = n_seq, T = max_frames, K = max_det;
    if (!sizes_ok(S, T, K, cap)) return LISO_EINVAL;
    if (S == 0) return LISO_OK;
    if (!n_frames || !n_det || !boxes || !odom || !into_prev || !into_next) return LISO_EINVAL;
    if (!n_out || !track_ids || !pos_world || !rot_world || !src || !is_fill || !w_T_sensor || !id_counter || !overflow) return LISO_EINVAL;
    if (!workspace || ((uintptr_t)workspace & 7) != 0) return LISO_EINVAL;
    const Tables tb = carve(S, T, K, workspace);
    const int rows = state_rows(K);
    if (workspace_bytes < tb.bytes + 256) return LISO_EWORKSPACE;
    if (!liso_dev::lds_opt_in(g_lds, (const void*)walk_kernel, kRowBytes * LISO_TRACK_MAX_CAP + 64)) return LISO_ELAUNCH;
    hipStream_t st = (hipStream_t)stream;
    chain_kernel<<<(S + 63) / 64, 64, 0, st>>>(S, T, n_frames, odom, w_T_sensor);
    const size_t dets = (size_t)S * T * K;
    world_kernel<<<(unsigned)((dets + kThreads - 1) / kThreads), kThreads, 0, st>>>(S, T, K, n_frames, n_det, boxes, into_prev, into_next,
                                                                                  w_T_sensor, tb);
    walk_kernel<<<S, kThreads, (size_t)kRowBytes * rows + 64, st>>>(T, K, cap, rows, n_frames, n_det, threshold, tb, n_out, track_ids, pos_world,
                                                                  rot_world, src, is_fill, id_counter, overflow);
    return check_launch();
}

}  // extern "C"
