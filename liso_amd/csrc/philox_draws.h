// Counter-based random draws for the data-path kernels: Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3",
// SC'11), the uniform conversions, and a sine / cosine of 2 pi (u - 1/2) stated operation by operation.  Everything here is restated
// in numpy by liso_amd/datasets/batch_augmentation.py (`philox4x32`, `draw_uniform`, `sincos_turn`) and must stay bit-equal to it:
// compile the including file with -ffp-contract=off.
//
// THE PACKING (the one place it is written down).  One draw = one Philox block:
//     key     = (seed & 0xffffffff, seed >> 32)                                   the 64-bit seed of the state tensor
//     counter = (element, (purpose << 27) | (object << 20) | (sample_id & 0xfffff), calls & 0xffffffff, calls >> 32)
//   element   32 bits: the index inside the purpose (attempt, axis, snippet row j, 3 j + component)
//   purpose   5 bits (Purpose below), object 7 bits (the slot 0..63; 0 for per-sample draws), sample id: its low 20 bits
//   calls     the 64-bit call number of the state tensor
// so a draw is a pure function of (seed, calls, sample id, object, purpose, element) and of nothing else -- not of the batch size,
// the launch geometry, another sample or another object.
//     uniform double  u = (((uint64)out[0] << 32 | out[1]) >> 11) * 2^-53      in [0, 1)
//     uniform integer in [0, n) = min((int64)(u * n), n - 1)                      (fp64 product; the min never binds for n < 2^52)
//     32-bit key      = out[0]
#ifndef LISO_PHILOX_DRAWS_H
#define LISO_PHILOX_DRAWS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace liso_draws {

enum Purpose : uint32_t {
    kCount = 0,     // number of objects of the sample
    kLocation = 1,  // element = attempt: index among the free cells
    kJitter = 2,    // element = axis (0 = x, 1 = y)
    kSnippet = 3,
    kHeight = 4,
    kHeading = 5,
    kFlip = 6,      // element = axis
    kScale = 7,     // element = axis (0, 1, 2)
    kKeep = 8,      // point drop-out: share of points kept
    kNth = 9,       // ray-drop: every nth row
    kStart = 10,    // ray-drop: first row
    kKey = 11,      // element = snippet row j: sort key of the drop-out subset
    kFlow = 12,     // element = 3 j + component
};

struct Stream {  // what is fixed for one (call, sample)
    uint32_t k0, k1, c2, c3, sample;
};

__host__ __device__ inline Stream make_stream(int64_t seed, int64_t calls, int64_t sample_id) {
    Stream s;
    s.k0 = (uint32_t)((uint64_t)seed & 0xffffffffull);
    s.k1 = (uint32_t)((uint64_t)seed >> 32);
    s.c2 = (uint32_t)((uint64_t)calls & 0xffffffffull);
    s.c3 = (uint32_t)((uint64_t)calls >> 32);
    s.sample = (uint32_t)((uint64_t)sample_id & 0xfffffull);
    return s;
}

__host__ __device__ inline void philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
    uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0, c1 = n1, c2 = n2, c3 = n3;
        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    }
    out[0] = c0, out[1] = c1, out[2] = c2, out[3] = c3;
}

__host__ __device__ inline void block(const Stream& s, uint32_t purpose, uint32_t object, uint32_t element, uint32_t out[4]) {
    const uint32_t ctr[4] = {element, (purpose << 27) | (object << 20) | s.sample, s.c2, s.c3};
    const uint32_t key[2] = {s.k0, s.k1};
    philox4x32_10(ctr, key, out);
}

__host__ __device__ inline double uniform(const Stream& s, uint32_t purpose, uint32_t object, uint32_t element) {
    uint32_t o[4];
    block(s, purpose, object, element, o);
    return (double)((((uint64_t)o[0] << 32) | o[1]) >> 11) * 0x1.0p-53;
}

__host__ __device__ inline uint32_t key32(const Stream& s, uint32_t purpose, uint32_t object, uint32_t element) {
    uint32_t o[4];
    block(s, purpose, object, element, o);
    return o[0];
}

// floor(u * n) for n >= 1, as an index
__host__ __device__ inline int64_t below(double u, int64_t n) {
    const int64_t v = (int64_t)(u * (double)n);
    return v < n - 1 ? v : n - 1;
}

// sin and cos of theta = 2 pi (u - 1/2), u in [0, 1).  With phi = 2 pi u = (pi / 4) (q + r), q = floor(8 u) the octant and
// r = 8 u - q the remainder (both exact: 8 u is a scaling by a power of two, the difference of two doubles that close is exact):
//     t = (pi / 4) r in [0, pi / 4)
//     S = t (1 + t2 (s3 + t2 (s5 + ... + t2 s17))),  C = 1 + t2 (c2 + t2 (c4 + ... + t2 c16)),  t2 = t t,  s_n = +-1 / n!, c_n = +-1 / n!
//     (every coefficient is the fp64 quotient 1 / n!, n! exact below 2^53; truncation below 1e-19)
//     odd q: the angle inside the quadrant is pi / 4 + t:  (S, C) <- (h (C + S), h (C - S)),  h = sqrt(1 / 2) rounded
//     quadrant q >> 1 rotates by a multiple of pi / 2 (swaps and signs), and theta = phi - pi negates both.
// At an octant border r = 0, so t = 0, S = 0 and C = 1: the results there are exactly 0, +-1 or +-h.
__host__ __device__ inline void sincos_turn(double u, double* sin_theta, double* cos_theta) {
    const double u8 = 8.0 * u;
    const int q = (int)u8;
    const double r = u8 - (double)q;
    const double t = 0.78539816339744830962 * r;
    const double t2 = t * t;
    double p = -1.0 / 355687428096000.0;         // -1 / 17!
    p = 1.0 / 1307674368000.0 + t2 * p;          // +1 / 15!
    p = -1.0 / 6227020800.0 + t2 * p;            // -1 / 13!
    p = 1.0 / 39916800.0 + t2 * p;               // +1 / 11!
    p = -1.0 / 362880.0 + t2 * p;                // -1 / 9!
    p = 1.0 / 5040.0 + t2 * p;                   // +1 / 7!
    p = -1.0 / 120.0 + t2 * p;                   // -1 / 5!
    p = 1.0 / 6.0 + t2 * p;                      // +1 / 3!  (sign folded below)
    double S = t * (1.0 - t2 * p);
    double c = 1.0 / 20922789888000.0;           // +1 / 16!
    c = -1.0 / 87178291200.0 + t2 * c;           // -1 / 14!
    c = 1.0 / 479001600.0 + t2 * c;              // +1 / 12!
    c = -1.0 / 3628800.0 + t2 * c;               // -1 / 10!
    c = 1.0 / 40320.0 + t2 * c;                  // +1 / 8!
    c = -1.0 / 720.0 + t2 * c;                   // -1 / 6!
    c = 1.0 / 24.0 + t2 * c;                     // +1 / 4!
    c = -0.5 + t2 * c;                           // -1 / 2!
    double C = 1.0 + t2 * c;
    if (q & 1) {
        const double h = 0.70710678118654752440;
        const double s1 = h * (C + S), c1 = h * (C - S);
        S = s1, C = c1;
    }
    double sp, cp;  // of phi
    switch ((q >> 1) & 3) {
        case 0: sp = S, cp = C; break;
        case 1: sp = C, cp = -S; break;
        case 2: sp = -S, cp = -C; break;
        default: sp = -C, cp = S; break;
    }
    *sin_theta = -sp;
    *cos_theta = -cp;
}

}  // namespace liso_draws
#endif
