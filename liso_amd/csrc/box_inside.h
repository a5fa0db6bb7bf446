// The points-in-boxes inside test shared by box_points.hip and frame_prep.hip: the box's inverse pose as an LDS row, the fp32
// circle that rejects most (point, box) pairs, and the two arithmetics of the exact test (include/liso_tracking.h: precision).
//
// Like dev_common.h this header carries no floating-point setting.  The fp32 product of `inside<1>` is written operation by
// operation (explicit fmaf) and gives the same bits under every contraction mode.  The fp64 sums of `make_box_row` and of
// `inside<0>` follow the translation unit's mode: between a file built with and one built without -ffp-contract=off they can
// differ in the last fp64 bit, which the rounding to fp32 before the comparison hides except on an exact tie.
#ifndef LISO_BOX_INSIDE_H
#define LISO_BOX_INSIDE_H

#include <hip/hip_runtime.h>
#include <math.h>

namespace liso_box {
namespace {  // (one private copy per translation unit)

// One box in LDS, 64 B: rows x and y of inv(sensor_T_box) = [Rz(yaw)^T | -Rz^T pos] are (c, s, 0, m03) and (-s, c, 0, m13),
// row z is (0, 0, 1, tz); the zero entries are not stored (adding 0 * z changes nothing for finite z; non-finite points
// are excluded before the test).
struct BoxRow {
    double c, s, m03, m13, tz;
    float hx, hy, hz;  // 0.5 * bloat * dims
    float pad;
};
struct PreRow {
    float x, y, r2;  // conservative circle around the box footprint: fp32 reject before the exact test
    int count;
};

// box = x, y, z, dx, dy, dz, yaw -> its LDS row and circle (count 0)
__device__ __forceinline__ void make_box_row(const float* box, float dims_bloat, BoxRow& r, PreRow& p) {
    // Shape.get_poses: sensor_T_box = [Rz(yaw) | pos] in fp64 (shape_utils.py:271-319)
    const double x = box[0], y = box[1], z = box[2], yaw = box[6];
    const double cs = cos(yaw), sn = sin(yaw);
    r.c = cs; r.s = sn; r.m03 = -(cs * x + sn * y); r.m13 = sn * x - cs * y; r.tz = -z;
    r.hx = 0.5f * (dims_bloat * box[3]); r.hy = 0.5f * (dims_bloat * box[4]); r.hz = 0.5f * (dims_bloat * box[5]);
    r.pad = 0.f;
    // inside => bx^2 + by^2 < hx^2 + hy^2; the margin covers the fp32 rounding of the squared distance at |xy| <= 1e4 m
    const float r2 = r.hx * r.hx + r.hy * r.hy;
    p.x = box[0]; p.y = box[1];
    p.r2 = r2 * 1.001f + 0.05f;  // NaN boxes: every comparison against it is false -> never inside
    p.count = 0;
}

template <int PREC>
__device__ __forceinline__ bool inside(const BoxRow& r, float px, float py, float pz) {
    float bx, by, bz;
    if (PREC == 0) {  // fp64 product, rounded to fp32 (torch_dataset_commons.py:1914-1918)
        const double dx = px, dy = py, dz = pz;
        bx = (float)(r.c * dx + r.s * dy + r.m03);
        by = (float)(r.c * dy - r.s * dx + r.m13);
        bz = (float)(dz + r.tz);
    } else {          // inverse rounded to fp32, fp32 product (shape_utils.py:514-518)
        const float c = (float)r.c, s = (float)r.s;
        bx = fmaf(s, py, c * px) + (float)r.m03;
        by = fmaf(c, py, -s * px) + (float)r.m13;
        bz = pz + (float)r.tz;
    }
    return fabsf(bx) < r.hx && fabsf(by) < r.hy && fabsf(bz) < r.hz;
}

}  // namespace
}  // namespace liso_box
#endif
