// Rotated-BEV box geometry of the reference's iou3d_nms on the device: the per-box quantities and the pair overlap
// (iou3d_nms/src/iou3d_cpu.cpp:59-229).  Shared by iou3d_nms.hip (overlap / IoU matrices, full-mask NMS) and det_nms.hip
// (survivor-bounded NMS), so both suppress with the same predicate, bit for bit.
//
// The geometry must round like the reference's host code: no FMA contraction.  The including files are also compiled with
// -ffp-contract=off (Makefile); the pragma keeps this true for any other includer.
#ifndef LISO_RBEV_GEOM_H
#define LISO_RBEV_GEOM_H

#include <hip/hip_runtime.h>
#include <math.h>

#pragma clang fp contract(off)

namespace liso_rbev {

constexpr int kPolyThreads = 256;  // PolyLds columns: the block size of every kernel that calls box_overlap_dev
constexpr int kMaxPoly = 16;     // reference: Point cross_points[16] (iou3d_cpu.cpp:168)
constexpr float kEps = 1e-8f;    // iou3d_cpu.cpp:38

// per-box derived quantities, SoA in LDS: g[field][box]
enum GeoField { G_CX, G_CY, G_LIMX, G_LIMY, G_COS, G_SIN, G_AREA, G_RAD, G_PX0, G_PX1, G_PX2, G_PX3, G_PY0, G_PY1, G_PY2, G_PY3, G_N };

struct Geo {
    float cx, cy, limx, limy, c, s, area, rad;
    float px[4], py[4];
};

struct PolyLds {
    float x[kMaxPoly][kPolyThreads];
    float y[kMaxPoly][kPolyThreads];
    float key[kMaxPoly][kPolyThreads];
};

__device__ __forceinline__ Geo make_geo(const float* __restrict__ b) {
    Geo g;
    const float x = b[0], y = b[1], dx = b[3], dy = b[4], ang = b[6];
    // iou3d_cpu.cpp:134-140 half extents and the axis-aligned corners
    const float hx = dx / 2, hy = dy / 2;
    const float x1 = x - hx, y1 = y - hy, x2 = x + hx, y2 = y + hy;
    // iou3d_cpu.cpp:158-159; cos(-a)==cos(a), sin(-a)==-sin(a) covers :80 as well
    const double ad = (double)ang;
    g.c = (float)cos(ad);
    g.s = (float)sin(ad);
    g.cx = x;
    g.cy = y;
    // iou3d_cpu.cpp:85  box[3] / 2 + MARGIN
    g.limx = dx / 2 + 1e-2f;
    g.limy = dy / 2 + 1e-2f;
    g.area = dx * dy;  // iou3d_cpu.cpp:225
    const float rx[4] = {x1, x2, x2, x1};
    const float ry[4] = {y1, y1, y2, y2};
#pragma unroll
    for (int k = 0; k < 4; k++) {
        // iou3d_cpu.cpp:119-123 rotate_around_center
        g.px[k] = (rx[k] - x) * g.c + (ry[k] - y) * (-g.s) + x;
        g.py[k] = (rx[k] - x) * g.s + (ry[k] - y) * g.c + y;
    }
    // conservative radius: half diagonal + in-box margin + slack for fp32 rounding of far-away coordinates
    g.rad = sqrtf(hx * hx + hy * hy) * 1.001f + 0.02f + 1e-5f * (fabsf(x) + fabsf(y) + fabsf(hx) + fabsf(hy));
    return g;
}

template <int W>
__device__ __forceinline__ void store_geo(float (*g)[W], int i, const Geo& v) {
    g[G_CX][i] = v.cx; g[G_CY][i] = v.cy; g[G_LIMX][i] = v.limx; g[G_LIMY][i] = v.limy;
    g[G_COS][i] = v.c; g[G_SIN][i] = v.s; g[G_AREA][i] = v.area; g[G_RAD][i] = v.rad;
#pragma unroll
    for (int k = 0; k < 4; k++) { g[G_PX0 + k][i] = v.px[k]; g[G_PY0 + k][i] = v.py[k]; }
}

template <int W>
__device__ __forceinline__ Geo load_geo(const float (*g)[W], int i) {
    Geo v;
    v.cx = g[G_CX][i]; v.cy = g[G_CY][i]; v.limx = g[G_LIMX][i]; v.limy = g[G_LIMY][i];
    v.c = g[G_COS][i]; v.s = g[G_SIN][i]; v.area = g[G_AREA][i]; v.rad = g[G_RAD][i];
#pragma unroll
    for (int k = 0; k < 4; k++) { v.px[k] = g[G_PX0 + k][i]; v.py[k] = g[G_PY0 + k][i]; }
    return v;
}

// iou3d_cpu.cpp:63-65
__device__ __forceinline__ float cross3(float p1x, float p1y, float p2x, float p2y, float p0x, float p0y) {
    return (p1x - p0x) * (p2y - p0y) - (p2x - p0x) * (p1y - p0y);
}

// iou3d_cpu.cpp:30-36 (ternary min/max, not fminf/fmaxf)
__device__ __forceinline__ float rmin(float a, float b) { return a > b ? b : a; }
__device__ __forceinline__ float rmax(float a, float b) { return a > b ? a : b; }

// iou3d_cpu.cpp:88-117
__device__ __forceinline__ bool seg_isect(float p1x, float p1y, float p0x, float p0y, float q1x, float q1y, float q0x,
                                          float q0y, float& ax, float& ay) {
    // :67-73 check_rect_cross(p0, p1, q0, q1)
    const bool rc = rmin(p0x, p1x) <= rmax(q0x, q1x) && rmin(q0x, q1x) <= rmax(p0x, p1x) &&
                    rmin(p0y, p1y) <= rmax(q0y, q1y) && rmin(q0y, q1y) <= rmax(p0y, p1y);
    if (!rc) return false;
    const float s1 = cross3(q0x, q0y, p1x, p1y, p0x, p0y);
    const float s2 = cross3(p1x, p1y, q1x, q1y, p0x, p0y);
    const float s3 = cross3(p0x, p0y, q1x, q1y, q0x, q0y);
    const float s4 = cross3(q1x, q1y, p1x, p1y, q0x, q0y);
    if (!(s1 * s2 > 0 && s3 * s4 > 0)) return false;
    const float s5 = cross3(q1x, q1y, p1x, p1y, p0x, p0y);
    if (fabsf(s5 - s1) > kEps) {
        ax = (s5 * q0x - s1 * q1x) / (s5 - s1);
        ay = (s5 * q0y - s1 * q1y) / (s5 - s1);
    } else {
        const float a0 = p0y - p1y, b0 = p1x - p0x, c0 = p0x * p1y - p1x * p0y;
        const float a1 = q0y - q1y, b1 = q1x - q0x, c1 = q0x * q1y - q1x * q0y;
        const float D = a0 * b1 - a1 * b0;
        ax = (b0 * c1 - b1 * c0) / D;
        ay = (a1 * c0 - a0 * c1) / D;
    }
    return true;
}

// iou3d_cpu.cpp:75-86 with cos(-h), sin(-h) folded: angle_cos = c, angle_sin = -s
__device__ __forceinline__ bool in_box(const Geo& box, float px, float py) {
    const float ac = box.c, as = -box.s;
    const float rx = (px - box.cx) * ac + (py - box.cy) * (-as);
    const float ry = (px - box.cx) * as + (py - box.cy) * ac;
    return fabsf(rx) < box.limx && fabsf(ry) < box.limy;
}

// iou3d_cpu.cpp:128-220.  A = row box ("box_a"), B = column box ("box_b").
__device__ float box_overlap_dev(const Geo& A, const Geo& B, PolyLds* __restrict__ P, int tid) {
    // exact early-out: disjoint bounding circles => no edge crossing and no corner inside the other box
    // (margin included in rad) => cnt == 0 => the reference returns fabs(0)/2.
    {
        const float ddx = A.cx - B.cx, ddy = A.cy - B.cy;
        const float rr = A.rad + B.rad;
        if (ddx * ddx + ddy * ddy > rr * rr) return 0.f;
    }
    int cnt = 0;
    float sx = 0.f, sy = 0.f;  // poly_center accumulator, :170-181
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int i1 = (i + 1) & 3;  // corners[4] = corners[0]
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int j1 = (j + 1) & 3;
            float hx, hy;
            if (seg_isect(A.px[i1], A.py[i1], A.px[i], A.py[i], B.px[j1], B.py[j1], B.px[j], B.py[j], hx, hy)) {
                if (cnt < kMaxPoly) { P->x[cnt][tid] = hx; P->y[cnt][tid] = hy; }
                sx = sx + hx;
                sy = sy + hy;
                cnt++;
            }
        }
    }
    // :184-195 corners of one box inside the other, interleaved b_k then a_k
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (in_box(A, B.px[k], B.py[k])) {
            sx = sx + B.px[k];
            sy = sy + B.py[k];
            if (cnt < kMaxPoly) { P->x[cnt][tid] = B.px[k]; P->y[cnt][tid] = B.py[k]; }
            cnt++;
        }
        if (in_box(B, A.px[k], A.py[k])) {
            sx = sx + A.px[k];
            sy = sy + A.py[k];
            if (cnt < kMaxPoly) { P->x[cnt][tid] = A.px[k]; P->y[cnt][tid] = A.py[k]; }
            cnt++;
        }
    }
    // cnt < 3: the shoelace fan below is empty or degenerate (cross with a zero vector) => 0
    if (cnt < 3) return 0.f;
    const float pcx = sx / cnt, pcy = sy / cnt;  // :197-198
    if (cnt > kMaxPoly) cnt = kMaxPoly;          // unreachable for convex quads (<= 8 crossings + 8 corners)

    // polar angle of every vertex once; point_cmp (:125-127) compares exactly these values
    for (int k = 0; k < cnt; k++) P->key[k][tid] = atan2f(P->y[k][tid] - pcy, P->x[k][tid] - pcx);

    // :199-209 bubble sort, swap when key[i] > key[i+1]
    for (int j = 0; j < cnt - 1; j++) {
        float kl = P->key[0][tid], xl = P->x[0][tid], yl = P->y[0][tid];
        for (int i = 0; i < cnt - j - 1; i++) {
            const float kr = P->key[i + 1][tid], xr = P->x[i + 1][tid], yr = P->y[i + 1][tid];
            if (kl > kr) {  // swap: right element moves to slot i, left one keeps bubbling
                P->key[i][tid] = kr; P->x[i][tid] = xr; P->y[i][tid] = yr;
            } else {
                P->key[i][tid] = kl; P->x[i][tid] = xl; P->y[i][tid] = yl;
                kl = kr; xl = xr; yl = yr;
            }
        }
        const int last = cnt - j - 1;
        P->key[last][tid] = kl; P->x[last][tid] = xl; P->y[last][tid] = yl;
    }

    // :211-217 shoelace fan about vertex 0
    const float x0 = P->x[0][tid], y0 = P->y[0][tid];
    float area = 0.f;
    float ux = P->x[0][tid] - x0, uy = P->y[0][tid] - y0;
    for (int k = 0; k < cnt - 1; k++) {
        const float vx = P->x[k + 1][tid] - x0, vy = P->y[k + 1][tid] - y0;
        area += ux * vy - uy * vx;
        ux = vx; uy = vy;
    }
    return fabsf(area) / 2.0f;
}

// iou3d_cpu.cpp:222-229
__device__ __forceinline__ float iou_from_overlap(const Geo& A, const Geo& B, float ov) {
    return ov / fmaxf(A.area + B.area - ov, kEps);
}

}  // namespace liso_rbev

#endif  // LISO_RBEV_GEOM_H
