// Summary pictures on the device (include/liso_visu.h): flow wheel, top-down intensity image, occupancy image, bird's-eye box
// corners, per-box colours and the anti-aliased lines of the box drawings.  Built with -ffp-contract=off: the blend and the corner
// products round like the numpy restatement in liso_amd/visu.
#include <math.h>

#include "../../include/liso_visu.h"
#include "dev_common.h"

using liso_dev::Carver;
using liso_dev::check_launch;
using liso_dev::to_i32;
using liso_dev::up256;

namespace {

constexpr int kBlock = 256;
constexpr int kWalk = LISO_VISU_WALK_LINES;

// ---- block reductions (kBlock threads, every thread calls) ------------------------------------------------------------------------
__device__ float block_max(float v, float* lds) {
    const int t = threadIdx.x;
    lds[t] = v;
    __syncthreads();
    for (int s = kBlock / 2; s > 0; s >>= 1) {
        if (t < s) lds[t] = fmaxf(lds[t], lds[t + s]);
        __syncthreads();
    }
    const float r = lds[0];
    __syncthreads();
    return r;
}

__device__ float block_min(float v, float* lds) {
    const int t = threadIdx.x;
    lds[t] = v;
    __syncthreads();
    for (int s = kBlock / 2; s > 0; s >>= 1) {
        if (t < s) lds[t] = fminf(lds[t], lds[t + s]);
        __syncthreads();
    }
    const float r = lds[0];
    __syncthreads();
    return r;
}

// ---- 1. flow wheel ----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float flow_mag(const float* f, size_t cells, size_t i) {
    const float fx = f[i], fy = f[cells + i];
    return sqrtf(fx * fx + fy * fy);
}

__global__ __launch_bounds__(kBlock) void flow_max_kernel(int cells, const float* flow, float* max_mag) {
    __shared__ float lds[kBlock];
    const float* f = flow + (size_t)blockIdx.x * 2 * cells;
    // torch.amax carries a NaN; fmaxf would drop it, so it is tracked apart
    float m = -INFINITY, nan = 0.f;
    for (int i = threadIdx.x; i < cells; i += kBlock) {
        const float v = flow_mag(f, cells, i);
        if (v != v) nan = 1.f;
        m = fmaxf(m, v);
    }
    m = block_max(m, lds);
    nan = block_max(nan, lds);
    if (threadIdx.x == 0) max_mag[blockIdx.x] = nan != 0.f ? NAN : m;
}

__global__ __launch_bounds__(kBlock) void flow_wheel_kernel(int cells, const float* flow, const float* max_mag, float* rgb) {
    const int b = blockIdx.y;
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= cells) return;
    const float* f = flow + (size_t)b * 2 * cells;
    const float two_pi = 6.283185307179586f;
    const float mag = flow_mag(f, cells, i);
    const float ang = atan2f(f[cells + i], f[i]);
    const float hue = (ang >= 0.f ? ang : ang + two_pi) / two_pi;
    const float q = mag / max_mag[b];
    const float val = q < 1.f ? q : 1.f;
    const float h6 = hue * 6.f;
    const float x = val * (-fabsf(fmodf(h6, 2.f) - 1.f) + 1.f);
    const float m = val - val;  // the reference's value minus chroma, saturation 1: 0, or NaN with val
    const int sector = (int)(unsigned char)(int)h6 % 6;
    float r = 0.f, g = 0.f, bl = 0.f;
    switch (sector) {
        case 0: r = val, g = x; break;
        case 1: r = x, g = val; break;
        case 2: g = val, bl = x; break;
        case 3: g = x, bl = val; break;
        case 4: r = x, bl = val; break;
        default: r = val, bl = x; break;
    }
    float* o = rgb + (size_t)b * 3 * cells;
    o[i] = r + m, o[cells + i] = g + m, o[2 * (size_t)cells + i] = bl + m;
}

// ---- 2. top-down image ------------------------------------------------------------------------------------------------------------
struct Extent {
    float min_x, min_y, max_x, max_y, f;
};

__device__ __forceinline__ Extent load_extent(const float* e, int h, int w) {
    Extent x{e[0], e[1], e[2], e[3], 0.f};
    const float fr = (float)h / (x.max_x - x.min_x), fc = (float)w / (x.max_y - x.min_y);
    x.f = fr < fc ? fr : fc;  // torch.min: a NaN factor wins
    if (fr != fr || fc != fc) x.f = NAN;
    return x;
}

// blocks [0, batch): lo / hi of one cloud's intensities; the blocks behind them zero the pixel keys
__global__ __launch_bounds__(kBlock) void topdown_prepare_kernel(int batch, int n_max, int stride, const float* pcl, const float* intensity,
                                                                 float* lohi, unsigned long long* keys, size_t n_keys) {
    __shared__ float lds[kBlock];
    if ((int)blockIdx.x >= batch) {
        const size_t step = (size_t)(gridDim.x - batch) * kBlock;
        for (size_t i = (size_t)(blockIdx.x - batch) * kBlock + threadIdx.x; i < n_keys; i += step) keys[i] = 0ull;
        return;
    }
    const int b = blockIdx.x;
    const float* p = pcl + (size_t)b * n_max * stride;
    const float* in = intensity + (size_t)b * n_max;
    float lo = INFINITY, hi = -INFINITY;
    for (int i = threadIdx.x; i < n_max; i += kBlock) {
        const float x = p[(size_t)i * stride], y = p[(size_t)i * stride + 1];
        if (x != x || y != y) continue;
        lo = fminf(lo, in[i]), hi = fmaxf(hi, in[i]);
    }
    lo = block_min(lo, lds);
    hi = block_max(hi, lds);
    if (threadIdx.x == 0) lohi[2 * b] = lo, lohi[2 * b + 1] = hi;
}

__global__ __launch_bounds__(kBlock) void topdown_scatter_kernel(int n_max, int stride, int h, int w, const float* pcl, const float* intensity,
                                                                 const float* extent, const float* lohi, unsigned long long* keys) {
    const int b = blockIdx.y;
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n_max) return;
    const float* p = pcl + ((size_t)b * n_max + i) * stride;
    const float x = p[0], y = p[1];
    if (x != x || y != y) return;
    const Extent e = load_extent(extent, h, w);
    const float eps = 0.01f;
    if (!((e.min_x + eps < x) && (e.min_y + eps < y) && (x < e.max_x - eps) && (y < e.max_y - eps))) return;
    const float pr = (x - e.min_x) * e.f, pc = (y - e.min_y) * e.f;
    if (!(pr > -1.f && pr < (float)h && pc > -1.f && pc < (float)w)) return;
    const int row = (int)pr, col = (int)pc;
    if (row < 0 || row >= h || col < 0 || col >= w) return;
    float v = intensity[(size_t)b * n_max + i];
    const float lo = lohi[2 * b], hi = lohi[2 * b + 1];
    if (lo < 0.f || hi > 1.f) v = (v - lo) / (hi - lo);
    const unsigned long long key = ((unsigned long long)(unsigned)(i + 1) << 32) | (unsigned long long)__float_as_uint(v);
    atomicMax(&keys[((size_t)b * h + row) * w + col], key);
}

__global__ __launch_bounds__(kBlock) void topdown_resolve_kernel(size_t n_keys, const unsigned long long* keys, float* image, uint8_t* occupied) {
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n_keys) return;
    const unsigned long long k = keys[i];
    image[i] = k ? __uint_as_float((unsigned)(k & 0xffffffffull)) : 0.f;
    occupied[i] = k ? 1 : 0;
}

// ---- 3. occupancy image -----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int pillar_coord(double p, double range, int n) {
    int v = to_i32(((p + 0.5 * range) / range) * (double)n);
    v = v < n - 1 ? v : n - 1;
    return v > 0 ? v : 0;
}

__global__ __launch_bounds__(kBlock) void zero_f32_kernel(size_t n, float* out) {
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBlock) out[i] = 0.f;
}

__global__ __launch_bounds__(kBlock) void occupancy_kernel(int n, int stride, int h, int w, double range_x, double range_y, const double* pts,
                                                           const uint8_t* valid, float* image) {
    const int b = blockIdx.y;
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n || (valid && !valid[(size_t)b * n + i])) return;
    const double* p = pts + ((size_t)b * n + i) * stride;
    image[((size_t)b * h + pillar_coord(p[0], range_x, h)) * w + pillar_coord(p[1], range_y, w)] = 1.f;
}

// ---- 4. bird's-eye box corners ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ int f32_to_i32(float v) { return (v >= -2147483648.f && v < 2147483648.f) ? (int)v : INT_MIN; }

__global__ __launch_bounds__(kBlock) void box_corners_kernel(int total, int h, int w, int range_form, const float* extent, int pose_f32, double dims_lo,
                                                             double dims_hi, const double* pos, const double* dims, const double* rot,
                                                             int32_t* rowcol) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= total) return;
    double dx = dims[3 * (size_t)i], dy = dims[3 * (size_t)i + 1];
    if (dims_lo > 0.0) {  // torch.clamp: NaN stays NaN
        dx = dx < dims_lo ? dims_lo : (dx > dims_hi ? dims_hi : dx);
        dy = dy < dims_lo ? dims_lo : (dy > dims_hi ? dims_hi : dy);
    }
    const double tx = pos[3 * (size_t)i], ty = pos[3 * (size_t)i + 1], th = rot[i];
    float px[5], py[5];
    if (pose_f32) {
        const float c = (float)cos((double)(float)th), s = (float)sin((double)(float)th);
        const float hx = 0.5f * (float)dx, hy = 0.5f * (float)dy, fx = (float)tx, fy = (float)ty;
        const float lx[5] = {hx, -hx, -hx, hx, hx + hy}, ly[5] = {hy, hy, -hy, -hy, 0.f};
        for (int k = 0; k < 5; ++k) {
            px[k] = (c * lx[k] + (-s) * ly[k]) + fx;
            py[k] = (s * lx[k] + c * ly[k]) + fy;
        }
    } else {
        const double c = cos(th), s = sin(th);
        const double hx = 0.5 * dx, hy = 0.5 * dy;
        const double lx[5] = {hx, -hx, -hx, hx, hx + hy}, ly[5] = {hy, hy, -hy, -hy, 0.0};
        for (int k = 0; k < 5; ++k) {
            px[k] = (float)((c * lx[k] + (-s) * ly[k]) + tx);
            py[k] = (float)((s * lx[k] + c * ly[k]) + ty);
        }
    }
    int32_t* o = rowcol + 10 * (size_t)i;
    if (range_form == 2) {
        const float rx = extent[0], ry = extent[1];
        for (int k = 0; k < 5; ++k) {
            o[2 * k] = f32_to_i32(rintf(((px[k] + 0.5f * rx) * (float)h) / rx));
            o[2 * k + 1] = f32_to_i32(rintf(((py[k] + 0.5f * ry) * (float)w) / ry));
        }
    } else {
        const Extent e = load_extent(extent, h, w);
        for (int k = 0; k < 5; ++k) {
            o[2 * k] = f32_to_i32((px[k] - e.min_x) * e.f);
            o[2 * k + 1] = f32_to_i32((py[k] - e.min_y) * e.f);
        }
    }
}

// ---- 5. per-box colours -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void box_colors_kernel(int n_slots, int mode, const float* scalar, const uint8_t* valid, const double* table,
                                                            double* colors) {
    __shared__ float lds[kBlock];
    const int b = blockIdx.x;
    const float* sc = scalar + (size_t)b * n_slots;
    const uint8_t* va = valid + (size_t)b * n_slots;
    float lo = INFINITY, hi = -INFINITY, nan = 0.f;
    for (int i = threadIdx.x; i < n_slots; i += kBlock)
        if (va[i]) {
            if (sc[i] != sc[i]) nan = 1.f;  // numpy's min / max carry a NaN
            lo = fminf(lo, sc[i]), hi = fmaxf(hi, sc[i]);
        }
    lo = block_min(lo, lds);
    hi = block_max(hi, lds);
    nan = block_max(nan, lds);
    const bool none = lo > hi;  // no valid slot (and no NaN: fmin / fmax dropped those)
    if (nan != 0.f) lo = hi = NAN;
    for (int i = threadIdx.x; i < n_slots; i += kBlock) {
        float t;
        if (mode == 0)
            t = (lo != hi) ? (sc[i] - lo) / (hi - lo) : 1.f;
        else if (none)
            t = 0.5f;
        else {
            const float d = hi - lo;
            t = (sc[i] - lo) / (d > 1e-6f || d != d ? d : 1e-6f);  // np.maximum carries a NaN
        }
        double* o = colors + 3 * ((size_t)b * n_slots + i);
        if (t != t) {
            o[0] = o[1] = o[2] = 0.0;
            continue;
        }
        const float x = t * 256.f;
        const int idx = x >= 256.f ? 255 : (x < 0.f ? 0 : (int)x);
        o[0] = table[3 * idx], o[1] = table[3 * idx + 1], o[2] = table[3 * idx + 2];
    }
}

// ---- 6. anti-aliased lines --------------------------------------------------------------------------------------------------------
__host__ __device__ inline long long line_cap(int h, int w, int max_reach) { return 3ll * ((h > w ? h : w) + 2ll * max_reach + 1); }

struct Entry {
    int pix;  // clipped row * w + col
    int num;  // the entry's value is |num| / ed
};

// One lane walks one line into its slice of the entry list; returns the number of entries.  `cap` bounds the slice: a walk of
// n steps emits at most 3 n entries and n <= max(dr, dc) + 1, which the caller's reach test keeps within cap / 3.
__device__ int walk_line(int r0, int c0, int r1, int c1, int h, int w, Entry* out, int cap, double* ed_out) {
    const int dc = abs(c0 - c1), dr = abs(r0 - r1);
    const int sc = c0 < c1 ? 1 : -1, sr = r0 < r1 ? 1 : -1;
    const double ed = (dc + dr == 0) ? 1.0 : (double)(float)sqrt((double)((long long)dc * dc + (long long)dr * dr));
    *ed_out = ed;
    int err = dc - dr, c = c0, r = r0, n = 0;
    auto emit = [&](int rr, int cc, int num) {
        if (n < cap) {
            rr = rr < 0 ? 0 : (rr > h - 1 ? h - 1 : rr);
            cc = cc < 0 ? 0 : (cc > w - 1 ? w - 1 : cc);
            out[n] = Entry{rr * w + cc, num};
            ++n;
        }
    };
    for (long long step = (long long)dc + dr + 2; step > 0; --step) {  // (the walk stops by itself; the count only bounds it)
        emit(r, c, err - dc + dr);
        const int e = err, cp = c;
        if (2 * e >= -dc) {
            if (c == c1) break;
            if ((double)(e + dr) < ed) emit(r + sr, c, e + dr);
            err -= dr;
            c += sc;
        }
        if (2 * e <= dr) {
            if (r == r1) break;
            if ((double)(dc - e) < ed) emit(r, cp + sc, dc - e);
            err += dc;
            r += sr;
        }
    }
    return n;
}

template <int C>
__global__ __launch_bounds__(kBlock) void draw_lines_kernel(int h, int w, int n_lines, int group, int closed, int max_reach, int cap, const int32_t* endpoints,
                                                            const uint8_t* valid, const double* colors, float* canvas, int32_t* overflow,
                                                            unsigned* keys_all, Entry* entries_all) {
    __shared__ int s_cnt[kWalk];
    __shared__ double s_ed[kWalk];
    __shared__ int s_over;
    const int b = blockIdx.x, t = threadIdx.x;
    const int n_groups = n_lines / group;
    unsigned* keys = keys_all + (size_t)b * h * w;
    Entry* entries = entries_all + (size_t)b * kWalk * cap;
    float* img = canvas + (size_t)b * h * w * C;
    for (int i = t; i < h * w; i += kBlock) __hip_atomic_store(&keys[i], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (t == 0) s_over = 0;
    unsigned seq = 0;  // entries applied so far: a pixel's key is 1 + the running index of the last entry that fell on it
    for (int base = 0; base < n_lines; base += kWalk) {
        __syncthreads();  // the chunk before is applied: its entry list and counts may go
        if (t < kWalk) {
            int cnt = 0;
            const int l = base + t;
            if (l < n_lines && (!valid || valid[(size_t)b * n_groups + l / group])) {
                int32_t p[4];
                if (closed) {  // corner l to the next corner of its group, the last one back to the first
                    const int l1 = l - l % group + (l % group + 1) % group;
                    const int32_t *q0 = endpoints + 2 * ((size_t)b * n_lines + l), *q1 = endpoints + 2 * ((size_t)b * n_lines + l1);
                    p[0] = q0[0], p[1] = q0[1], p[2] = q1[0], p[3] = q1[1];
                } else {
                    const int32_t* q = endpoints + 4 * ((size_t)b * n_lines + l);
                    p[0] = q[0], p[1] = q[1], p[2] = q[2], p[3] = q[3];
                }
                const long long lo = -(long long)max_reach, hr = (long long)h - 1 + max_reach, hc = (long long)w - 1 + max_reach;
                if (p[0] < lo || p[0] > hr || p[2] < lo || p[2] > hr || p[1] < lo || p[1] > hc || p[3] < lo || p[3] > hc)
                    atomicAdd(&s_over, 1);
                else
                    cnt = walk_line(p[0], p[1], p[2], p[3], h, w, entries + (size_t)t * cap, cap, &s_ed[t]);
            }
            s_cnt[t] = cnt;
        }
        __syncthreads();
        const int in_chunk = n_lines - base < kWalk ? n_lines - base : kWalk;
        for (int j = 0; j < in_chunk; ++j) {
            const int cnt = s_cnt[j];
            if (cnt == 0) continue;  // (uniform over the block)
            const Entry* e = entries + (size_t)j * cap;
            for (int k = t; k < cnt; k += kBlock) atomicMax(&keys[e[k].pix], seq + (unsigned)k + 1u);
            __syncthreads();
            const double ed = s_ed[j];
            const double* col = colors + ((size_t)b * n_groups + (base + j) / group) * C;
            for (int k = t; k < cnt; k += kBlock) {
                const int pix = e[k].pix;
                // (the keys are only ever touched by atomics, which act at the L2: no stale copy in the vector cache)
                if (__hip_atomic_load(&keys[pix], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != seq + (unsigned)k + 1u) continue;  // a later entry owns the pixel
                const double wgt = 1.0 - fabs((double)e[k].num) / ed;
                float* px = img + (size_t)pix * C;
#pragma unroll
                for (int ch = 0; ch < C; ++ch) px[ch] = (float)((1.0 - wgt) * (double)px[ch] + wgt * col[ch]);
            }
            __syncthreads();  // the next line reads what this one wrote
            seq += (unsigned)cnt;
        }
    }
    __syncthreads();
    if (t == 0 && overflow && s_over) atomicAdd(&overflow[b], s_over);
}

bool cells_ok(int h, int w) { return h >= 1 && w >= 1 && (long long)h * w <= LISO_VISU_MAX_CELLS; }

}  // namespace

extern "C" {

int liso_visu_flow_wheel_f32(int batch, int h, int w, const float* flow, float* max_mag, float* rgb, void* stream) {
    if (batch < 0 || !cells_ok(h, w) || batch > 65535) return LISO_EINVAL;
    if (batch == 0) return LISO_OK;
    if (!flow || !max_mag || !rgb) return LISO_EINVAL;
    const int cells = h * w;
    hipStream_t s = (hipStream_t)stream;
    flow_max_kernel<<<batch, kBlock, 0, s>>>(cells, flow, max_mag);
    flow_wheel_kernel<<<dim3((cells + kBlock - 1) / kBlock, batch), kBlock, 0, s>>>(cells, flow, max_mag, rgb);
    return check_launch();
}

size_t liso_visu_topdown_workspace_bytes(int batch, int h, int w) {
    if (batch < 1 || !cells_ok(h, w)) return 0;
    Carver c{nullptr};
    c.take<unsigned long long>((size_t)batch * h * w);
    c.take<float>(2 * (size_t)batch);
    return c.bytes;
}

int liso_visu_topdown_f32(int batch, int n_max, int point_stride, int h, int w, const float* pcl, const float* intensity,
                          const float* extent, float* image, uint8_t* occupied, void* workspace, size_t workspace_bytes, void* stream) {
    if (batch < 0 || batch > 65535 || n_max < 0 || n_max > LISO_VISU_MAX_N || point_stride < 2 || !cells_ok(h, w)) return LISO_EINVAL;
    if (batch == 0) return LISO_OK;
    if (!extent || !image || !occupied || !workspace || (n_max > 0 && (!pcl || !intensity))) return LISO_EINVAL;
    if (workspace_bytes < liso_visu_topdown_workspace_bytes(batch, h, w)) return LISO_EWORKSPACE;
    Carver c{workspace};
    const size_t n_keys = (size_t)batch * h * w;
    unsigned long long* keys = c.take<unsigned long long>(n_keys);
    float* lohi = c.take<float>(2 * (size_t)batch);
    hipStream_t s = (hipStream_t)stream;
    size_t zero_blocks = (n_keys + kBlock - 1) / kBlock;
    if (zero_blocks > 1024) zero_blocks = 1024;
    topdown_prepare_kernel<<<batch + (int)zero_blocks, kBlock, 0, s>>>(batch, n_max, point_stride, pcl, intensity, lohi, keys, n_keys);
    if (n_max > 0)
        topdown_scatter_kernel<<<dim3((n_max + kBlock - 1) / kBlock, batch), kBlock, 0, s>>>(n_max, point_stride, h, w, pcl, intensity, extent, lohi,
                                                                                              keys);
    topdown_resolve_kernel<<<(unsigned)((n_keys + kBlock - 1) / kBlock), kBlock, 0, s>>>(n_keys, keys, image, occupied);
    return check_launch();
}

int liso_visu_occupancy_f64(int batch, int n, int pt_stride, int h, int w, double range_x, double range_y, const double* pts,
                            const uint8_t* valid, float* image, void* stream) {
    if (batch < 0 || batch > 65535 || n < 0 || n > LISO_VISU_MAX_N || pt_stride < 2 || !cells_ok(h, w)) return LISO_EINVAL;
    if (batch == 0) return LISO_OK;
    if (!image || (n > 0 && !pts)) return LISO_EINVAL;
    const size_t cells = (size_t)batch * h * w;
    size_t zb = (cells + kBlock - 1) / kBlock;
    zero_f32_kernel<<<(unsigned)(zb > 1024 ? 1024 : zb), kBlock, 0, (hipStream_t)stream>>>(cells, image);
    if (n > 0) occupancy_kernel<<<dim3((n + kBlock - 1) / kBlock, batch), kBlock, 0, (hipStream_t)stream>>>(n, pt_stride, h, w, range_x, range_y, pts, valid, image);
    return check_launch();
}

int liso_visu_box_corners_bev(int batch, int n_slots, int h, int w, int range_form, const float* extent, int pose_f32, double dims_lo,
                              double dims_hi, const double* pos, const double* dims, const double* rot, int32_t* rowcol, void* stream) {
    if (batch < 0 || n_slots < 0 || n_slots > LISO_VISU_MAX_LINES || !cells_ok(h, w) || (range_form != 2 && range_form != 4) ||
        !(dims_lo <= dims_hi) || (long long)batch * n_slots > (1ll << 30))
        return LISO_EINVAL;
    const int total = batch * n_slots;
    if (total == 0) return LISO_OK;
    if (!extent || !pos || !dims || !rot || !rowcol) return LISO_EINVAL;
    box_corners_kernel<<<(total + kBlock - 1) / kBlock, kBlock, 0, (hipStream_t)stream>>>(total, h, w, range_form, extent, pose_f32, dims_lo, dims_hi,
                                                                                           pos, dims, rot, rowcol);
    return check_launch();
}

int liso_visu_box_colors(int batch, int n_slots, int mode, const float* scalar, const uint8_t* valid, const double* table, double* colors,
                         void* stream) {
    if (batch < 0 || n_slots < 0 || n_slots > LISO_VISU_MAX_LINES || (mode != 0 && mode != 1)) return LISO_EINVAL;
    if (batch == 0 || n_slots == 0) return LISO_OK;
    if (!scalar || !valid || !table || !colors) return LISO_EINVAL;
    box_colors_kernel<<<batch, kBlock, 0, (hipStream_t)stream>>>(n_slots, mode, scalar, valid, table, colors);
    return check_launch();
}

size_t liso_visu_lines_workspace_bytes(int batch, int h, int w, int max_reach) {
    if (batch < 1 || !cells_ok(h, w) || max_reach < 0 || max_reach > (1 << 20)) return 0;
    Carver c{nullptr};
    c.take<unsigned>((size_t)batch * h * w);
    c.take<Entry>((size_t)batch * kWalk * (size_t)line_cap(h, w, max_reach));
    return c.bytes;
}

int liso_visu_draw_lines_f32(int batch, int h, int w, int channels, int n_lines, int group, int closed, int max_reach, const int32_t* endpoints,
                             const uint8_t* valid, const double* colors, float* canvas, int32_t* overflow, void* workspace,
                             size_t workspace_bytes, void* stream) {
    if (batch < 0 || !cells_ok(h, w) || (channels != 1 && channels != 3 && channels != 4) || n_lines < 0 || n_lines > LISO_VISU_MAX_LINES ||
        group < 1 || n_lines % group || max_reach < 0 || max_reach > (1 << 20))
        return LISO_EINVAL;
    const long long cap = line_cap(h, w, max_reach);
    if (cap * (long long)n_lines > 0xfffffff0ll) return LISO_EINVAL;  // the running entry index is 32 bits
    if (batch == 0 || n_lines == 0) return LISO_OK;
    if (!endpoints || !colors || !canvas || !workspace) return LISO_EINVAL;
    if (workspace_bytes < liso_visu_lines_workspace_bytes(batch, h, w, max_reach)) return LISO_EWORKSPACE;
    Carver c{workspace};
    unsigned* keys = c.take<unsigned>((size_t)batch * h * w);
    Entry* entries = c.take<Entry>((size_t)batch * kWalk * (size_t)cap);
    hipStream_t s = (hipStream_t)stream;
#define LISO_DRAW(C) \
    draw_lines_kernel<C><<<batch, kBlock, 0, s>>>(h, w, n_lines, group, closed, max_reach, (int)cap, endpoints, valid, colors, canvas, overflow, keys, entries)
    if (channels == 1)
        LISO_DRAW(1);
    else if (channels == 3)
        LISO_DRAW(3);
    else
        LISO_DRAW(4);
#undef LISO_DRAW
    return check_launch();
}

}  // extern "C"
