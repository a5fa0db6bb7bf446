// Host twin of the rotated-BEV pair geometry (iou3d_nms/src/iou3d_cpu.cpp:59-229), for the explicitly-CPU entry points of the
// library: liso_iou3d_iou_bev_cpu_f32 (iou3d_nms.hip) and liso_det_val_pairs_cpu_f32 (det_val.hip).  Not a fallback for any device
// path.  The including files are compiled with -ffp-contract=off (Makefile); the pragma keeps this true for any other includer.
#ifndef LISO_RBEV_GEOM_HOST_H
#define LISO_RBEV_GEOM_HOST_H

#include <math.h>

#pragma clang fp contract(off)

namespace liso_rbev_host {

constexpr float kEps = 1e-8f;  // iou3d_cpu.cpp:38

struct HPt { float x, y; };

inline float h_cross3(HPt p1, HPt p2, HPt p0) { return (p1.x - p0.x) * (p2.y - p0.y) - (p2.x - p0.x) * (p1.y - p0.y); }
inline float h_min(float a, float b) { return a > b ? b : a; }
inline float h_max(float a, float b) { return a > b ? a : b; }

inline bool h_isect(HPt p1, HPt p0, HPt q1, HPt q0, HPt& ans) {
    if (!(h_min(p0.x, p1.x) <= h_max(q0.x, q1.x) && h_min(q0.x, q1.x) <= h_max(p0.x, p1.x) &&
          h_min(p0.y, p1.y) <= h_max(q0.y, q1.y) && h_min(q0.y, q1.y) <= h_max(p0.y, p1.y)))
        return false;
    const float s1 = h_cross3(q0, p1, p0), s2 = h_cross3(p1, q1, p0), s3 = h_cross3(p0, q1, q0), s4 = h_cross3(q1, p1, q0);
    if (!(s1 * s2 > 0 && s3 * s4 > 0)) return false;
    const float s5 = h_cross3(q1, p1, p0);
    if (fabsf(s5 - s1) > kEps) {
        ans.x = (s5 * q0.x - s1 * q1.x) / (s5 - s1);
        ans.y = (s5 * q0.y - s1 * q1.y) / (s5 - s1);
    } else {
        const float a0 = p0.y - p1.y, b0 = p1.x - p0.x, c0 = p0.x * p1.y - p1.x * p0.y;
        const float a1 = q0.y - q1.y, b1 = q1.x - q0.x, c1 = q0.x * q1.y - q1.x * q0.y;
        const float D = a0 * b1 - a1 * b0;
        ans.x = (b0 * c1 - b1 * c0) / D;
        ans.y = (a1 * c0 - a0 * c1) / D;
    }
    return true;
}

inline bool h_in_box(const float* box, HPt p) {
    const float c = cosf(-box[6]), s = sinf(-box[6]);
    const float rx = (p.x - box[0]) * c + (p.y - box[1]) * (-s);
    const float ry = (p.x - box[0]) * s + (p.y - box[1]) * c;
    return fabsf(rx) < box[3] / 2 + 1e-2f && fabsf(ry) < box[4] / 2 + 1e-2f;
}

inline void h_corners(const float* box, HPt out[5]) {
    const float hx = box[3] / 2, hy = box[4] / 2, c = cosf(box[6]), s = sinf(box[6]);
    const float xs[4] = {box[0] - hx, box[0] + hx, box[0] + hx, box[0] - hx};
    const float ys[4] = {box[1] - hy, box[1] - hy, box[1] + hy, box[1] + hy};
    for (int k = 0; k < 4; k++) {
        out[k].x = (xs[k] - box[0]) * c + (ys[k] - box[1]) * (-s) + box[0];
        out[k].y = (xs[k] - box[0]) * s + (ys[k] - box[1]) * c + box[1];
    }
    out[4] = out[0];
}

// area of the intersection polygon of A and B (iou3d_cpu.cpp:128-220)
inline float h_overlap_bev(const float* A, const float* B) {
    HPt ca[5], cb[5], poly[24];
    float key[24];
    h_corners(A, ca);
    h_corners(B, cb);
    int cnt = 0;
    float sx = 0.f, sy = 0.f;
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) {
            HPt h;
            if (h_isect(ca[i + 1], ca[i], cb[j + 1], cb[j], h)) { poly[cnt++] = h; sx = sx + h.x; sy = sy + h.y; }
        }
    for (int k = 0; k < 4; k++) {
        if (h_in_box(A, cb[k])) { sx = sx + cb[k].x; sy = sy + cb[k].y; poly[cnt++] = cb[k]; }
        if (h_in_box(B, ca[k])) { sx = sx + ca[k].x; sy = sy + ca[k].y; poly[cnt++] = ca[k]; }
    }
    float ov = 0.f;
    if (cnt >= 3) {
        const float pcx = sx / cnt, pcy = sy / cnt;
        for (int k = 0; k < cnt; k++) key[k] = atan2f(poly[k].y - pcy, poly[k].x - pcx);
        for (int j = 0; j < cnt - 1; j++)
            for (int i = 0; i < cnt - j - 1; i++)
                if (key[i] > key[i + 1]) {
                    const HPt t = poly[i]; poly[i] = poly[i + 1]; poly[i + 1] = t;
                    const float tk = key[i]; key[i] = key[i + 1]; key[i + 1] = tk;
                }
        float area = 0.f;
        for (int k = 0; k < cnt - 1; k++)
            area += (poly[k].x - poly[0].x) * (poly[k + 1].y - poly[0].y) - (poly[k].y - poly[0].y) * (poly[k + 1].x - poly[0].x);
        ov = fabsf(area) / 2.0f;
    }
    return ov;
}

// iou3d_cpu.cpp:222-229
inline float h_iou_from_overlap(const float* A, const float* B, float ov) {
    return ov / fmaxf(A[3] * A[4] + B[3] * B[4] - ov, kEps);
}

inline float h_iou_bev(const float* A, const float* B) { return h_iou_from_overlap(A, B, h_overlap_bev(A, B)); }

}  // namespace liso_rbev_host

#endif  // LISO_RBEV_GEOM_HOST_H
