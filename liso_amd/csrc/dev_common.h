// The small helpers every data-path translation unit needs, in one place: the launch check, the workspace carver, the clamping
// and rounding rules that the golden fixtures pin bit for bit, the fp64 affine algebra and the fp64 wave shuffle.  A kernel file
// includes this header and names what it uses (`using liso_dev::to_i32;`) instead of copying it.
//
// The header carries no floating-point setting: no #pragma, no contraction switch.  Every function here is compiled with the
// flags the Makefile gives the translation unit that includes it (FLAGS_<name>), and that is what keeps the files built with
// -ffp-contract=off evaluating these expressions operation by operation.
#ifndef LISO_DEV_COMMON_H
#define LISO_DEV_COMMON_H

#include <hip/hip_runtime.h>
#include <limits.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/liso_iou3d.h"  // LISO_OK, LISO_ELAUNCH

namespace liso_dev {
namespace {  // (one private copy per translation unit)

// ---- host ---------------------------------------------------------------------------------------------------------------------
inline int check_launch() { return hipGetLastError() == hipSuccess ? LISO_OK : LISO_ELAUNCH; }

inline size_t up256(size_t v) { return (v + 255) / 256 * 256; }

// Lays tables one behind the other into a workspace, each starting on a 256-byte boundary.  `bytes` is read after the last take;
// with a null base nothing is usable and the carver only measures.
struct Carver {
    void* base;
    size_t bytes = 0;
    template <typename T>
    T* take(size_t count) {
        char* p = (char*)base + bytes;
        bytes += up256(count * sizeof(T));
        return (T*)p;
    }
};

// the n-byte buffers at a and b do not overlap
inline bool distinct(const void* a, const void* b, size_t n) { return (const char*)a + n <= (const char*)b || (const char*)b + n <= (const char*)a; }

// ---- device -------------------------------------------------------------------------------------------------------------------
// rows of cloud b: the whole padded length without counts, else the count clamped to [0, N]
__device__ __forceinline__ int cloud_rows(const int32_t* counts, int b, int N) {
    if (!counts) return N;
    const int n = counts[b];
    return n < 0 ? 0 : (n > N ? N : n);
}

// numpy's astype(int32) of a float64: truncation, INT_MIN for NaN and for values outside int32
__device__ __forceinline__ int to_i32(double v) { return (v > -2147483649.0 && v < 2147483648.0) ? (int)v : INT_MIN; }

// C = A * B for 4x4 row-major, each entry ((a0*b0 + a1*b1) + a2*b2) + a3*b3
__device__ void mat4_mul(const double* A, const double* B, double* C) {
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c)
            C[4 * r + c] = ((A[4 * r] * B[c] + A[4 * r + 1] * B[4 + c]) + A[4 * r + 2] * B[8 + c]) + A[4 * r + 3] * B[12 + c];
}

// inverse of an affine matrix [A t; 0 0 0 1]: adjugate(A) / det(A), -A^-1 t
__device__ void affine_inv(const double* M, double* R) {
    const double a = M[0], b = M[1], c = M[2], d = M[4], e = M[5], f = M[6], g = M[8], h = M[9], k = M[10];
    const double c00 = e * k - f * h, c01 = c * h - b * k, c02 = b * f - c * e;
    const double c10 = f * g - d * k, c11 = a * k - c * g, c12 = c * d - a * f;
    const double c20 = d * h - e * g, c21 = b * g - a * h, c22 = a * e - b * d;
    const double det = (a * c00 + b * c10) + c * c20;
    const double inv[9] = {c00 / det, c01 / det, c02 / det, c10 / det, c11 / det, c12 / det, c20 / det, c21 / det, c22 / det};
    const double tx = M[3], ty = M[7], tz = M[11];
    for (int r = 0; r < 3; ++r) {
        R[4 * r] = inv[3 * r], R[4 * r + 1] = inv[3 * r + 1], R[4 * r + 2] = inv[3 * r + 2];
        R[4 * r + 3] = -((inv[3 * r] * tx + inv[3 * r + 1] * ty) + inv[3 * r + 2] * tz);
    }
    R[12] = 0.0, R[13] = 0.0, R[14] = 0.0, R[15] = 1.0;
}

// __shfl_xor of a double as its two 32-bit halves
__device__ __forceinline__ double shfl_xor_f64(double v, int m) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __shfl_xor(lo, m);
    hi = __shfl_xor(hi, m);
    return __hiloint2double(hi, lo);
}

}  // namespace
}  // namespace liso_dev
#endif
