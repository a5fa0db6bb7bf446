// DBSCAN over the dynamic BEV pillars + region moments, on the device, for gfx950.  C ABI + reference lines:
// include/liso_flow_cluster.h.
//
// The reference clusters the M dynamic pillars in the 5-D space (x, y, 2 fx, 2 fy, 2 fz) with sklearn's DBSCAN
// (eps 1 m, min_samples 5) on the host.  eps bounds the BEV distance, so every eps-neighbour of a pillar lies inside a
// (2R+1)^2 window of the dense grid (R = 6 at 0.195 m pillars): no neighbour lists, no KD-tree, no M^2 pairs.
//
//   dyn_count / dyn_place  the dynamic cells listed in row-major order in the workspace (no host read, fixed grids)
//   dbscan_core     one wave per listed cell: counts eps-neighbours in the window (self included) -> core flag
//   dbscan_union    lock-free union-find (always link the larger root under the smaller: atomicMin on the parent) of every
//                   core cell with every core eps-neighbour of smaller index: in LDS per tile (16 waves per tile), then one
//                   global hook per cell; windows above 8 hook every edge in the global array
//   dbscan_flatten  one thread per core cell: is_root flag (the root is the smallest cell index of its component)
//   dbscan_label    one wave per listed cell: core -> rank of its root; border -> smallest rank among its core
//                   eps-neighbours; no core neighbour -> 0 (noise).  rank = 1-based position of the root among all
//                   roots in row-major order (an inclusive scan of the root flags, done by the caller).
// Why this equals sklearn's labelling: sklearn visits points in input (row-major) order, starts cluster k at the k-th
// still unlabelled core point and grows it completely (depth-first over core points, labelling every neighbour) before
// it moves on -- so clusters are the connected components of the core graph numbered by their smallest member, and a
// border point reachable from several clusters keeps the first one that reached it, i.e. the smallest number.
//
//   region_moments  6 exact integer moments per label (n, sum r, sum c, sum r^2, sum c^2, sum rc): per-block sums in LDS
//                   added by a second launch; above 1024 labels 64-bit global atomics (integers: order independent)
//   region_props    one thread per label: centroid, orientation, axis lengths from the second central moments
//                   (skimage.measure.regionprops formulas, fp64)
#include <hip/hip_runtime.h>
#include "zero_fill.h"
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../include/liso_flow_cluster.h"
#include "../../include/liso_iou3d.h"
#include "dev_common.h"

namespace {

using liso_dev::check_launch;

struct Cfg {
    int batch, gx, gy, win, min_samples;
    double eps_sqr;
    float flow_weight;
};

// squared 5-D distance exactly as the host code builds it: float32 features (centre coordinates, flow_weight * flow)
// promoted to float64, differences squared and summed in feature order
__device__ __forceinline__ double dist_sqr(const float* __restrict__ xs, const float* __restrict__ ys,
                                           const float* __restrict__ flow, float fw, int r0, int c0, size_t i0, int r1, int c1,
                                           size_t i1) {
    const double d0 = (double)xs[r0] - (double)xs[r1];
    const double d1 = (double)ys[c0] - (double)ys[c1];
    const double d2 = (double)(fw * flow[3 * i0 + 0]) - (double)(fw * flow[3 * i1 + 0]);
    const double d3 = (double)(fw * flow[3 * i0 + 1]) - (double)(fw * flow[3 * i1 + 1]);
    const double d4 = (double)(fw * flow[3 * i0 + 2]) - (double)(fw * flow[3 * i1 + 2]);
    return d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3 + d4 * d4;
}

// Wave-cooperative window walk: the 64 lanes of a wave share the 13 x 13 window of ONE cell `me` (3 iterations, consecutive
// columns = coalesced reads) instead of one lane walking it alone (169 dependent iterations).  f(nb) runs on the lanes whose
// window cell nb is a neighbour (dynamic, within eps) of `me`.
template <typename F>
__device__ __forceinline__ void wave_for_each_neighbour(const Cfg& c, const uint8_t* __restrict__ dyn, const float* __restrict__ xs,
                                                        const float* __restrict__ ys, const float* __restrict__ flow, size_t me,
                                                        int lane, F&& f) {
    const size_t per = (size_t)c.gx * c.gy;
    const int b = (int)(me / per), r = (int)((me % per) / c.gy), col = (int)(me % c.gy);
    const size_t base = (size_t)b * per;
    const int r_lo = max(r - c.win, 0), r_hi = min(r + c.win, c.gx - 1);
    const int c_lo = max(col - c.win, 0), c_hi = min(col + c.win, c.gy - 1);
    const int wc = c_hi - c_lo + 1, n = (r_hi - r_lo + 1) * wc;
    for (int k = lane; k < n; k += 64) {
        const int rr = r_lo + k / wc, cc = c_lo + k % wc;
        const size_t nb = base + (size_t)rr * c.gy + cc;
        if (dyn[nb] && dist_sqr(xs, ys, flow, c.flow_weight, r, col, me, rr, cc, nb) <= c.eps_sqr) f(nb);
    }
}

// parents only ever move to smaller indices; device-scope loads keep concurrent hooks visible (fewer retries)
__device__ __forceinline__ int find_root(const int* parent, int x) {
    int p = __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while (p != x) { x = p; p = __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    return x;
}

// find + one-step compression: the start node is re-parented to the root that was found (an ancestor with a smaller index:
// parents still only ever decrease, so concurrent hooks stay valid); the next walk from this node is one hop
__device__ __forceinline__ int find_root_compress(int* parent, int x0) {
    const int r = find_root(parent, x0);
    if (r != x0) atomicMin(&parent[x0], r);
    return r;
}

// joins the trees of x and y in the global forest of one sample: the larger root goes under the smaller one
__device__ __forceinline__ void hook(int* par, int x, int y) {
    while (true) {
        x = find_root_compress(par, x);
        y = find_root_compress(par, y);
        if (x == y) break;
        if (x < y) { const int t = x; x = y; y = t; }  // x: larger root, linked under y
        const int old = atomicMin(&par[x], y);
        if (old == x) break;  // x was still a root: linked
        x = old;              // somebody re-parented x meanwhile: retry from there
    }
}

// the union for windows above kMaxWin (the tiled kernel's LDS region holds no wider halo): every (core cell, smaller core
// eps-neighbour) pair is hooked in the global parent array.  A wave takes the core cells among its 64 consecutive cells one after
// the other and its lanes share the window of that cell.
__global__ __launch_bounds__(256) void dbscan_union_kernel(Cfg c, const uint8_t* __restrict__ dyn, const uint8_t* __restrict__ core,
                                                           const float* __restrict__ xs, const float* __restrict__ ys,
                                                           const float* __restrict__ flow, int* __restrict__ parent) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t per = (size_t)c.gx * c.gy, total = per * c.batch;
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(i < total && core[i]);
    while (todo) {  // (the final forest -- every tree rooted at its smallest cell -- does not depend on the order of the hooks)
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const size_t cell = i - lane + src;
        int* par = parent + (cell / per) * per;
        const int me = (int)(cell % per);
        wave_for_each_neighbour(c, dyn, xs, ys, flow, cell, lane, [&](size_t nb) {
            const int other = (int)(nb % per);
            if (core[nb] && other < me) hook(par, me, other);  // every undirected edge once
        });
    }
}

// ---- union-find in two levels: LDS inside a tile (+ halo), global atomics for one edge per cell ----------------------------------------
// dbscan_union_kernel hooks every (core cell, smaller core eps-neighbour) pair with device-scope atomics on the global parent array: a
// blob of 150 cells is ~10 000 hooks, each a chain of dependent L2 round trips (round-5 measurement on the bench's sweeps: 4 000 core
// cells, 107 us).  Here a block owns a kTR x kTC tile: the core flags and flows of the tile and its eps halo go to LDS, every edge
// (x in the tile, y in x's window, y < x) is hooked in an LDS parent array (values = per-sample cell indices, so local roots are the
// smallest cell of the local component, the order the global forest uses), and then every core cell of the region is hooked ONCE in
// the global array: with its local root.  Each eps edge lies inside the region of the tile that holds its larger end, so the global
// forest connects exactly the components of the core graph; tiles without a core cell (almost all of them) leave after one load.
constexpr int kTR = 16, kTC = 32, kUfThreads = 1024, kMaxWin = 8;
constexpr int kRegMax = (kTR + 2 * kMaxWin) * (kTC + 2 * kMaxWin);

__device__ __forceinline__ int lds_find(const int* par, int l, int r0, int c0, int RW, int gy) {
    // par[l] = per-sample cell index of the parent; a root points at itself
    while (true) {
        const int me = (r0 + l / RW) * gy + (c0 + l % RW);
        const int p = par[l];
        if (p == me) return l;
        l = (p / gy - r0) * RW + (p % gy - c0);
    }
}

__global__ __launch_bounds__(kUfThreads) void dbscan_union_tiled_kernel(Cfg c, const uint8_t* __restrict__ dyn,
                                                                        const uint8_t* __restrict__ core, const float* __restrict__ xs,
                                                                        const float* __restrict__ ys, const float* __restrict__ flow,
                                                                        int* __restrict__ parent, int tiles_r, int tiles_c) {
    __shared__ int s_par[kRegMax];
    __shared__ float s_f[kRegMax][3];
    __shared__ uint8_t s_core[kRegMax];
    __shared__ int s_any;
    const int b = blockIdx.y;
    const int tr = blockIdx.x / tiles_c, tc = blockIdx.x % tiles_c;
    const int tid = threadIdx.x;
    const size_t per = (size_t)c.gx * c.gy, base = (size_t)b * per;
    // does the TILE hold a core cell?
    if (tid == 0) s_any = 0;
    __syncthreads();
    int any = 0;
    for (int q = tid; q < kTR * kTC; q += kUfThreads) {
        const int r = tr * kTR + q / kTC, col = tc * kTC + q % kTC;
        if (r < c.gx && col < c.gy && core[base + (size_t)r * c.gy + col]) any = 1;
    }
    if (any) s_any = 1;
    __syncthreads();
    if (!s_any) return;
    // region = tile + halo, clipped to the grid
    const int r0 = max(tr * kTR - c.win, 0), r1 = min(tr * kTR + kTR + c.win, c.gx);
    const int c0 = max(tc * kTC - c.win, 0), c1 = min(tc * kTC + kTC + c.win, c.gy);
    const int RW = c1 - c0, RH = r1 - r0, RN = RW * RH;
    for (int l = tid; l < RN; l += kUfThreads) {
        const int r = r0 + l / RW, col = c0 + l % RW;
        const size_t g = base + (size_t)r * c.gy + col;
        const uint8_t co = core[g];
        s_core[l] = co;
        s_par[l] = r * c.gy + col;
        if (co) {
            s_f[l][0] = c.flow_weight * flow[3 * g + 0];
            s_f[l][1] = c.flow_weight * flow[3 * g + 1];
            s_f[l][2] = c.flow_weight * flow[3 * g + 2];
        }
    }
    __syncthreads();
    // local hooks: every core cell of the tile with its smaller core eps-neighbours.  The tile's core cells are listed first; a wave takes
    // a cell at a time and its 64 lanes share the cell's window (the half with smaller indices: <= (2 win + 1) win + win cells)
    __shared__ int s_list[kTR * kTC];
    __shared__ int s_n;
    if (tid == 0) s_n = 0;
    __syncthreads();
    for (int q = tid; q < kTR * kTC; q += kUfThreads) {
        const int r = tr * kTR + q / kTC, col = tc * kTC + q % kTC;
        if (r < c.gx && col < c.gy && s_core[(r - r0) * RW + (col - c0)]) s_list[atomicAdd(&s_n, 1)] = q;
    }
    __syncthreads();
    const int n_list = s_n, lane = tid & 63, wave = tid >> 6;
    const int ww = 2 * c.win + 1;
    for (int e = wave; e < n_list; e += kUfThreads / 64) {
        const int q = s_list[e];
        const int r = tr * kTR + q / kTC, col = tc * kTC + q % kTC;
        const int lx = (r - r0) * RW + (col - c0);
        const double x0 = (double)xs[r], y0 = (double)ys[col];
        const double f0 = (double)s_f[lx][0], f1 = (double)s_f[lx][1], f2 = (double)s_f[lx][2];
        const int n_win = c.win * ww + c.win;  // window cells in front of the centre, row-major
        for (int k = lane; k < n_win; k += 64) {
            const int rr = r - c.win + k / ww, cc = col - c.win + k % ww;
            if (rr < 0 || cc < 0 || cc >= c.gy) continue;  // (rr <= r < gx)
            const int ly = (rr - r0) * RW + (cc - c0);
            if (!s_core[ly]) continue;
            // the 5-D distance exactly as dist_sqr builds it (fp32 features promoted to fp64, summed in feature order)
            const double d0 = x0 - (double)xs[rr], d1 = y0 - (double)ys[cc];
            const double d2 = f0 - (double)s_f[ly][0], d3 = f1 - (double)s_f[ly][1], d4 = f2 - (double)s_f[ly][2];
            if (d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3 + d4 * d4 > c.eps_sqr) continue;
            int a = lx, bq = ly;
            while (true) {
                a = lds_find(s_par, a, r0, c0, RW, c.gy);
                bq = lds_find(s_par, bq, r0, c0, RW, c.gy);
                if (a == bq) break;
                const int ga = (r0 + a / RW) * c.gy + (c0 + a % RW), gb = (r0 + bq / RW) * c.gy + (c0 + bq % RW);
                int hi = a, lo_g = gb, hi_g = ga;
                if (ga < gb) { hi = bq; lo_g = ga; hi_g = gb; }
                const int old = atomicMin(&s_par[hi], lo_g);  // the larger root under the smaller one
                if (old == hi_g) break;                       // it was still a root: linked
                // somebody re-parented it meanwhile, to `old`.  The atomicMin has already stored min(old, lo_g) there, so when
                // lo_g < old the edge hi -> old is GONE: go on with the pair (old, lo_g), as hook() does with `x = old`
                // (walking on from hi would find hi and lo_g joined and leave old's tree cut off)
                a = (old / c.gy - r0) * RW + (old % c.gy - c0);
                bq = (lo_g / c.gy - r0) * RW + (lo_g % c.gy - c0);
            }
        }
    }
    __syncthreads();
    // one global hook per core cell of the region: the cell with its local root
    int* par = parent + base;
    for (int l = tid; l < RN; l += kUfThreads) {
        if (!s_core[l]) continue;
        const int me = (r0 + l / RW) * c.gy + (c0 + l % RW);
        const int lr = lds_find(s_par, l, r0, c0, RW, c.gy);
        const int root = (r0 + lr / RW) * c.gy + (c0 + lr % RW);
        if (root != me) hook(par, me, root);
    }
}

__global__ void dbscan_flatten_kernel(Cfg c, const uint8_t* __restrict__ core, int* __restrict__ parent,
                                      int* __restrict__ is_root) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t per = (size_t)c.gx * c.gy;
    if (i >= per * c.batch) return;
    int root_flag = 0;
    if (core[i]) {
        const int* par = parent + (i / per) * per;
        const int root = find_root(par, (int)(i % per));
        root_flag = root == (int)(i % per);  // no path compression: the label pass walks the (short) chains again
    }
    is_root[i] = root_flag;
}

// ---- the list of dynamic cells, and the core count and the labelling that walk it --------------------------------------------------------
// A few thousand of the 512 x 512 cells are dynamic, in blobs: with one thread (or wave) per stretch of the dense grid the handful of
// waves that hold a blob do all the work while 99 % of the waves leave at once, and the launch lasts as long as its busiest wave.  So
// the dynamic cells are listed first, in row-major order (block counts, then every block places its cells behind the blocks in front
// of it: the same list whatever the schedule), and a fixed grid of waves takes the listed cells one per wave, so a blob spreads over
// the chip.  The results are per cell: they do not depend on which wave takes which cell.
constexpr int kListThreads = 256, kListPasses = 8, kListTile = kListThreads * kListPasses;  // cells per block of the two list passes
constexpr int kListGrid = 1024;                                                             // blocks of 4 waves that walk the list

__global__ __launch_bounds__(kListThreads) void dyn_count_kernel(const uint8_t* __restrict__ dyn, unsigned total, int* __restrict__ block_cnt) {
    __shared__ int wsum[kListThreads / 64];
    const unsigned base = blockIdx.x * (unsigned)kListTile;
    int n = 0;
#pragma unroll
    for (int k = 0; k < kListPasses; k++) {
        const unsigned i = base + k * kListThreads + threadIdx.x;
        n += (i < total && dyn[i]) ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) block_cnt[blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

// list[rank of the cell among the dynamic cells] = cell (index into the whole batch); the cells that are not dynamic get their core flag and
// parent here (0, -1); *n_list = number of dynamic cells
__global__ __launch_bounds__(kListThreads) void dyn_place_kernel(const uint8_t* __restrict__ dyn, unsigned total, const int* __restrict__ block_cnt,
                                                                 int* __restrict__ list, int* __restrict__ n_list, uint8_t* __restrict__ core,
                                                                 int* __restrict__ parent) {
    __shared__ int s_red[kListThreads / 64];
    __shared__ int s_seg[kListPasses][kListThreads / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int before = 0;  // dynamic cells in the blocks in front of this one
    for (int q = threadIdx.x; q < (int)blockIdx.x; q += kListThreads) before += block_cnt[q];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) before += __shfl_xor(before, o);
    if (lane == 0) s_red[wave] = before;
    const unsigned base = blockIdx.x * (unsigned)kListTile;
    unsigned long long mine[kListPasses];
#pragma unroll
    for (int k = 0; k < kListPasses; k++) {
        const unsigned i = base + k * kListThreads + threadIdx.x;
        const bool d = i < total && dyn[i];
        mine[k] = __ballot(d);
        if (lane == 0) s_seg[k][wave] = __popcll(mine[k]);
        if (i < total && !d) { core[i] = 0; parent[i] = -1; }
    }
    __syncthreads();
    int pos = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
#pragma unroll
    for (int k = 0; k < kListPasses; k++) {
        // (cells of pass k, wave w come behind all passes < k and the waves < w of pass k: row-major order)
        if ((mine[k] >> lane) & 1ull) {
            int p = pos + __popcll(mine[k] & ((1ull << lane) - 1ull));
            for (int w = 0; w < wave; w++) p += s_seg[k][w];
            list[p] = (int)(base + k * kListThreads + threadIdx.x);
        }
        pos += (s_seg[k][0] + s_seg[k][1]) + (s_seg[k][2] + s_seg[k][3]);
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) *n_list = pos;
}

// core flag and initial parent of the listed cells: eps-neighbours in the window, the cell itself included, counted by one wave
__global__ __launch_bounds__(256) void dbscan_core_kernel(Cfg c, const uint8_t* __restrict__ dyn, const float* __restrict__ xs,
                                                          const float* __restrict__ ys, const float* __restrict__ flow,
                                                          const int* __restrict__ list, const int* __restrict__ n_list,
                                                          uint8_t* __restrict__ core, int* __restrict__ parent) {
    const int lane = threadIdx.x & 63, n = *n_list;
    const size_t per = (size_t)c.gx * c.gy;
    for (int e = blockIdx.x * 4 + (threadIdx.x >> 6); e < n; e += gridDim.x * 4) {
        const size_t cell = (size_t)list[e];
        int count = 0;
        wave_for_each_neighbour(c, dyn, xs, ys, flow, cell, lane, [&](size_t) { count++; });
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) count += __shfl_xor(count, o);
        if (lane == 0) {
            const int is_core = count >= c.min_samples;
            core[cell] = (uint8_t)is_core;
            parent[cell] = is_core ? (int)(cell % per) : -1;  // per-sample cell index
        }
    }
}

// labels of the listed cells (the others were zero-filled): core -> rank of its root; border -> smallest rank among its core eps-neighbours
__global__ __launch_bounds__(256) void dbscan_label_kernel(Cfg c, const uint8_t* __restrict__ dyn, const uint8_t* __restrict__ core,
                                                           const float* __restrict__ xs, const float* __restrict__ ys,
                                                           const float* __restrict__ flow, const int* __restrict__ parent,
                                                           const int* __restrict__ root_rank, const int* __restrict__ list,
                                                           const int* __restrict__ n_list, int* __restrict__ labels) {
    const int lane = threadIdx.x & 63, n = *n_list;
    const size_t per = (size_t)c.gx * c.gy;
    for (int e = blockIdx.x * 4 + (threadIdx.x >> 6); e < n; e += gridDim.x * 4) {
        const size_t cell = (size_t)list[e];
        const int* par = parent + (cell / per) * per;
        const int* rank = root_rank + (cell / per) * per;
        int best = 0x7fffffff;
        if (core[cell]) {  // (the same cell in every lane: a wave-uniform branch)
            best = rank[find_root(par, (int)(cell % per))];
        } else {
            wave_for_each_neighbour(c, dyn, xs, ys, flow, cell, lane, [&](size_t nb) {
                if (core[nb]) best = min(best, rank[find_root(par, (int)(nb % per))]);
            });
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) best = min(best, __shfl_xor(best, o));
        }
        if (lane == 0) labels[cell] = best == 0x7fffffff ? 0 : best;
    }
}

// Integer moments of every labelled region.  A wave covers 64 consecutive cells, which carry at most a few distinct labels:
// the wave reduces the six sums per label (butterfly) and ONE lane issues the atomics -- 6 per (wave, label) instead of 6 per
// cell, which serialised on the few dozen label rows (243 us at 512 x 512).  Integer sums: any order gives the same bits.
__global__ __launch_bounds__(256) void region_moments_kernel(const int* __restrict__ labels, int batch, int gx, int gy, int max_labels,
                                                             unsigned long long* __restrict__ mom) {
    // (32-bit index arithmetic: batch * gx * gy < 2^31 is checked by the caller; three 64-bit divisions per cell were most of this
    // kernel's instructions)
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned per = (unsigned)gx * (unsigned)gy;
    const int lane = threadIdx.x & 63;
    int l = i < per * (unsigned)batch ? labels[i] : 0;
    if (l > max_labels) l = 0;
    const unsigned bi = i / per, rem = i - bi * per, ri = rem / (unsigned)gy;
    const long key = l > 0 ? (long)bi * max_labels + (l - 1) : -1;
    const unsigned long long r = ri, col = rem - ri * (unsigned)gy;
    unsigned long long todo = __ballot(key >= 0);
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        const long k = __shfl(key, src);
        const bool mine = key == k;
        unsigned long long v[6] = {mine ? 1ull : 0ull, mine ? r : 0ull, mine ? col : 0ull, mine ? r * r : 0ull, mine ? col * col : 0ull,
                                   mine ? r * col : 0ull};
#pragma unroll
        for (int o = 32; o > 0; o >>= 1)
#pragma unroll
            for (int q = 0; q < 6; q++) v[q] += __shfl_xor(v[q], o);
        if (lane == src) {
            unsigned long long* m = mom + (size_t)k * 6;
#pragma unroll
            for (int q = 0; q < 6; q++) atomicAdd(m + q, v[q]);
        }
        todo &= ~__ballot(mine);
    }
}

// The same sums without global atomics, for label maps whose labelled cells are SCATTERED (a frozen flow network on real data gives
// blobs; an untrained one marks single pillars all over the map): round-5 measurement on the bench's sweeps -- 4 306 labelled cells in
// 30 clusters, nearly every one in a wave of its own -> 26 k 64-bit atomics on 180 addresses, 75 us; 30 compact blobs of the same
// area: 4 us.  Here a block owns kRmCells consecutive cells of one sample, adds into LDS ([max_labels][6] u64, ds_add_u64) and writes
// its rows to partial[sample][block][label][6] (plain stores, zeros included: no fill pass); region_props_kernel adds the blocks'
// rows (integers: any order gives the same bits) before it evaluates the moments.
constexpr int kRmCells = 2048, kRmThreads = 256, kRmMaxLabels = 1024;
__global__ __launch_bounds__(kRmThreads) void region_moments_lds_kernel(const int* __restrict__ labels, int gx, int gy, int max_labels,
                                                                         int blocks_per_sample, unsigned long long* __restrict__ partial) {
    extern __shared__ unsigned long long s_mom[];  // [max_labels][6]
    const int b = blockIdx.y, blk = blockIdx.x;
    const unsigned per = (unsigned)gx * (unsigned)gy;
    for (int q = threadIdx.x; q < max_labels * 6; q += kRmThreads) s_mom[q] = 0ull;
    __syncthreads();
    const unsigned c0 = (unsigned)blk * kRmCells;
    for (unsigned c = c0 + threadIdx.x; c < c0 + kRmCells && c < per; c += kRmThreads) {
        int l = labels[(size_t)b * per + c];
        if (l <= 0 || l > max_labels) continue;
        const unsigned long long r = c / (unsigned)gy, col = c - (unsigned)r * (unsigned)gy;
        unsigned long long* m = s_mom + (size_t)(l - 1) * 6;
        atomicAdd(m + 0, 1ull); atomicAdd(m + 1, r); atomicAdd(m + 2, col);
        atomicAdd(m + 3, r * r); atomicAdd(m + 4, col * col); atomicAdd(m + 5, r * col);
    }
    __syncthreads();
    unsigned long long* out = partial + ((size_t)b * blocks_per_sample + blk) * max_labels * 6;
    for (int q = threadIdx.x; q < max_labels * 6; q += kRmThreads) out[q] = s_mom[q];
}

// mom[region][6] = sum over the sample's blocks of partial[sample][block][label][6]: one wave per region, lanes stride over the blocks
__global__ __launch_bounds__(256) void region_moments_sum_kernel(const unsigned long long* __restrict__ partial, int batch, int max_labels,
                                                                 int blocks_per_sample, unsigned long long* __restrict__ mom) {
    const int region = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (region >= batch * max_labels) return;
    const int b = region / max_labels, l = region - b * max_labels;
    unsigned long long v[6] = {0, 0, 0, 0, 0, 0};
    for (int blk = lane; blk < blocks_per_sample; blk += 64) {
        const unsigned long long* p = partial + (((size_t)b * blocks_per_sample + blk) * max_labels + l) * 6;
#pragma unroll
        for (int q = 0; q < 6; q++) v[q] += p[q];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
#pragma unroll
        for (int q = 0; q < 6; q++) v[q] += __shfl_xor(v[q], o);
    if (lane < 6) {
        unsigned long long w = v[0];
#pragma unroll
        for (int q = 1; q < 6; q++) w = lane == q ? v[q] : w;
        mom[(size_t)region * 6 + lane] = w;
    }
}

__global__ void region_props_kernel(const unsigned long long* __restrict__ mom, long n_regions, double* __restrict__ props) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_regions) return;
    const unsigned long long* m = mom + (size_t)i * 6;
    double* p = props + (size_t)i * 5;
    const double n = (double)m[0];
    if (m[0] == 0) { p[0] = p[1] = p[2] = p[3] = p[4] = 0.0; return; }
    const double sr = (double)m[1], sc = (double)m[2];
    const double cr = sr / n, cc = sc / n;  // centroid (row, col)
    // central second moments, normalised by the area (skimage: inertia_tensor = [[mu02, -mu11], [-mu11, mu20]] / mu00)
    const double mu20 = ((double)m[3] - sr * sr / n) / n;  // rows
    const double mu02 = ((double)m[4] - sc * sc / n) / n;  // cols
    const double mu11 = ((double)m[5] - sr * sc / n) / n;
    const double a = mu02, b = -mu11, c = mu20;
    double orientation;
    if (a - c == 0.0)
        orientation = b < 0.0 ? -M_PI / 4.0 : M_PI / 4.0;
    else
        orientation = 0.5 * atan2(-2.0 * b, c - a);
    const double tr = a + c, disc = sqrt((a - c) * (a - c) + 4.0 * b * b);
    const double l1 = fmax(0.5 * (tr + disc), 0.0), l2 = fmax(0.5 * (tr - disc), 0.0);
    p[0] = cr; p[1] = cc; p[2] = orientation; p[3] = 4.0 * sqrt(l1); p[4] = 4.0 * sqrt(l2);
}

inline bool cfg_ok(const liso_dbscan_cfg* c) {
    return c && c->batch >= 1 && c->gx >= 1 && c->gy >= 1 && c->window >= 0 && c->min_samples >= 1 && c->eps > 0.f &&
           (long)c->gx * c->gy < (1L << 31);
}
inline Cfg to_cfg(const liso_dbscan_cfg* c) {
    Cfg k;
    k.batch = c->batch; k.gx = c->gx; k.gy = c->gy; k.win = c->window; k.min_samples = c->min_samples;
    k.eps_sqr = (double)c->eps * (double)c->eps;
    k.flow_weight = c->flow_weight;
    return k;
}

// the list workspace: list[total] | block_cnt[blocks] | n_list
struct ListWs {
    int *list, *block_cnt, *n_list;
    unsigned blocks;
};
inline size_t carve_list(void* base, size_t total, ListWs& w) {
    liso_dev::Carver cv{base};
    w.blocks = (unsigned)((total + kListTile - 1) / kListTile);
    w.list = cv.take<int>(total);
    w.block_cnt = cv.take<int>(w.blocks);
    w.n_list = cv.take<int>(1);
    return cv.bytes;
}
inline unsigned list_grid(size_t total) { return (unsigned)(total / 4 + 1 < (size_t)kListGrid ? total / 4 + 1 : (size_t)kListGrid); }

// the checks the two DBSCAN calls share (their pointers apart): *total = cells of the batch, w = the carved workspace
inline int open_list(const liso_dbscan_cfg* cfg, void* workspace, size_t workspace_bytes, size_t* total, ListWs& w) {
    const size_t need = liso_dbscan_workspace_bytes(cfg);
    if (need == 0) return LISO_EINVAL;  // a bad cfg, or 2^31 cells or more
    if (!workspace || workspace_bytes < need) return LISO_EWORKSPACE;
    *total = (size_t)cfg->batch * cfg->gx * cfg->gy;
    carve_list(workspace, *total, w);
    return LISO_OK;
}

}  // namespace

extern "C" {

size_t liso_dbscan_workspace_bytes(const liso_dbscan_cfg* cfg) {
    if (!cfg_ok(cfg) || (size_t)cfg->batch * cfg->gx * cfg->gy >= (1ull << 31)) return 0;
    ListWs w{};
    return carve_list(nullptr, (size_t)cfg->batch * cfg->gx * cfg->gy, w);
}

int liso_dbscan_components(const liso_dbscan_cfg* cfg, const uint8_t* dynamic_mask, const float* row_coords,
                           const float* col_coords, const float* flow, uint8_t* core, int32_t* parent, int32_t* is_root,
                           void* workspace, size_t workspace_bytes, void* stream) {
    if (!dynamic_mask || !row_coords || !col_coords || !flow || !core || !parent || !is_root) return LISO_EINVAL;
    size_t total;
    ListWs w{};
    if (const int rc = open_list(cfg, workspace, workspace_bytes, &total, w)) return rc;
    const Cfg c = to_cfg(cfg);
    const unsigned blocks = (unsigned)((total + 255) / 256);
    hipStream_t st = (hipStream_t)stream;
    dyn_count_kernel<<<w.blocks, kListThreads, 0, st>>>(dynamic_mask, (unsigned)total, w.block_cnt);
    dyn_place_kernel<<<w.blocks, kListThreads, 0, st>>>(dynamic_mask, (unsigned)total, w.block_cnt, w.list, w.n_list, core, parent);
    dbscan_core_kernel<<<list_grid(total), 256, 0, st>>>(c, dynamic_mask, row_coords, col_coords, flow, w.list, w.n_list, core, parent);
    if (c.win <= kMaxWin) {
        const int tiles_r = (c.gx + kTR - 1) / kTR, tiles_c = (c.gy + kTC - 1) / kTC;
        dbscan_union_tiled_kernel<<<dim3(tiles_r * tiles_c, c.batch), kUfThreads, 0, st>>>(c, dynamic_mask, core, row_coords, col_coords,
                                                                                         flow, parent, tiles_r, tiles_c);
    } else {
        dbscan_union_kernel<<<blocks, 256, 0, st>>>(c, dynamic_mask, core, row_coords, col_coords, flow, parent);
    }
    dbscan_flatten_kernel<<<blocks, 256, 0, st>>>(c, core, parent, is_root);
    return check_launch();
}

int liso_dbscan_labels(const liso_dbscan_cfg* cfg, const uint8_t* dynamic_mask, const float* row_coords, const float* col_coords,
                       const float* flow, const uint8_t* core, const int32_t* parent, const int32_t* root_rank, int32_t* labels,
                       const void* workspace, size_t workspace_bytes, void* stream) {
    if (!dynamic_mask || !row_coords || !col_coords || !flow || !core || !parent || !root_rank || !labels) return LISO_EINVAL;
    size_t total;
    ListWs w{};
    if (const int rc = open_list(cfg, (void*)workspace, workspace_bytes, &total, w)) return rc;
    const Cfg c = to_cfg(cfg);
    hipStream_t st = (hipStream_t)stream;
    if (liso_zero::zero_async(labels, total * sizeof(int32_t), st) != hipSuccess) return LISO_ELAUNCH;
    dbscan_label_kernel<<<list_grid(total), 256, 0, st>>>(c, dynamic_mask, core, row_coords, col_coords, flow, parent, root_rank, w.list,
                                                         w.n_list, labels);
    return check_launch();
}

size_t liso_region_props_workspace_bytes(int batch, int gx, int gy, int max_labels) {
    if (batch < 1 || gx < 1 || gy < 1 || max_labels < 1 || max_labels > kRmMaxLabels) return 0;
    const size_t per = (size_t)gx * gy;
    if (per * batch >= (1ull << 31)) return 0;
    const size_t blocks = (per + kRmCells - 1) / kRmCells;
    return (size_t)batch * blocks * max_labels * 6 * sizeof(uint64_t);
}

int liso_region_props(const int32_t* labels, int batch, int gx, int gy, int max_labels, uint64_t* moments, double* props,
                      void* workspace, size_t workspace_bytes, void* stream) {
    if (!labels || batch < 1 || gx < 1 || gy < 1 || max_labels < 1 || !moments || !props) return LISO_EINVAL;
    const size_t total = (size_t)batch * gx * gy;
    if (total >= (1ull << 31)) return LISO_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const long regions = (long)batch * max_labels;
    const size_t need = liso_region_props_workspace_bytes(batch, gx, gy, max_labels);
    if (need == 0) {  // more than 1024 labels: the atomics path, no workspace
        if (liso_zero::zero_async(moments, (size_t)regions * 6 * sizeof(uint64_t), st) != hipSuccess) return LISO_ELAUNCH;
        region_moments_kernel<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(labels, batch, gx, gy, max_labels,
                                                                              (unsigned long long*)moments);
    } else {
        if (!workspace || workspace_bytes < need) return LISO_EWORKSPACE;
        const int blocks = (int)(((size_t)gx * gy + kRmCells - 1) / kRmCells);
        region_moments_lds_kernel<<<dim3(blocks, batch), kRmThreads, (size_t)max_labels * 6 * sizeof(uint64_t), st>>>(
            labels, gx, gy, max_labels, blocks, (unsigned long long*)workspace);
        region_moments_sum_kernel<<<(unsigned)((regions + 3) / 4), 256, 0, st>>>((const unsigned long long*)workspace, batch, max_labels,
                                                                                blocks, (unsigned long long*)moments);
    }
    region_props_kernel<<<(unsigned)((regions + 255) / 256), 256, 0, st>>>((const unsigned long long*)moments, regions, props);
    return check_launch();
}

}  // extern "C"
