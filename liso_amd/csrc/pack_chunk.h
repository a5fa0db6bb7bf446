// One 16-byte chunk of a convolution's packed filter panel (include/liso_conv.h: "Packed weights"), shared by the kernels that write
// panels: the pack launches of conv_mfma.hip (from the fp32 master weights in global memory) and the AdamW pass of optim.hip that
// writes the panels of the filters it has just updated (from LDS).  One copy of the rounding, the hi / lo split and the chunk's
// address, so that a panel holds the same bytes whichever kernel wrote it.
#ifndef LISO_PACK_CHUNK_H
#define LISO_PACK_CHUNK_H

#include <hip/hip_runtime.h>

#include "../../include/liso_conv.h"
#include "elem16.h"

namespace liso_pack {

__device__ __forceinline__ unsigned pack_bf16(float a, float b) {
    const __bf16 x = (__bf16)a, y = (__bf16)b;
    return (unsigned)__builtin_bit_cast(unsigned short, x) | ((unsigned)__builtin_bit_cast(unsigned short, y) << 16);
}
__device__ __forceinline__ float round_bf16(float v) { return (float)(__bf16)v; }

// panel formats: 16-bit planes of bf16 (BF16, F32X3 hi / lo), exact fp32, one fp16 plane
constexpr int kPackBf16 = 0, kPackF32 = 1, kPackF16 = 2;
__host__ __device__ inline int pack_format(int mode) { return mode == LISO_CONV_F32 ? kPackF32 : mode == LISO_CONV_F16 ? kPackF16 : kPackBf16; }
__host__ __device__ inline int pack_planes(int mode) { return mode == LISO_CONV_F32X3 ? 2 : 1; }
// values along k in one chunk: 8 x 16 bit, 4 x fp32
__host__ __device__ inline int pack_chunk_k(int fmt) { return fmt == kPackF32 ? 4 : 8; }

// 16-B chunks of the packed weights: 16-bit planes x taps x Kp/8 x Np; exact fp32 (one plane of 4-float groups): taps x Kp/4 x Np
__host__ __device__ inline long pack_chunks(int planes, int taps, int Kp, int Np, int fmt) {
    return fmt == kPackF32 ? (long)taps * (Kp / 4) * Np : (long)planes * taps * (Kp / 8) * Np;
}

// chunk (plane, tap, kc, n) of the panel `dst` = the values val(k, n, tap) for the chunk's 8 (fp32: 4) consecutive k; `val` returns 0
// for padding
template <typename F>
__device__ __forceinline__ void pack_chunk_at(F&& val, int fmt, int plane, int tap, int kc, int n, int taps, int Kp, int Np,
                                              unsigned short* __restrict__ dst) {
    if (fmt == kPackF32) {  // [tap][Kp / 4][Np][4] fp32, unrounded
        const long q = ((long)tap * (Kp / 4) + kc) * Np + n;
        float f[4];
#pragma unroll
        for (int e = 0; e < 4; e++) f[e] = val(kc * 4 + e, n, tap);
        *reinterpret_cast<float4*>(dst + q * 8) = make_float4(f[0], f[1], f[2], f[3]);
        return;
    }
    const long q = (((long)plane * taps + tap) * (Kp / 8) + kc) * Np + n;
    unsigned w[4];
#pragma unroll
    for (int e = 0; e < 4; e++) {
        float f[2];
#pragma unroll
        for (int z = 0; z < 2; z++) {
            const float v = val(kc * 8 + 2 * e + z, n, tap);
            if (fmt == kPackF16) {
                f[z] = v;
            } else {
                const float hi = round_bf16(v);
                f[z] = plane == 0 ? hi : (v - hi);
            }
        }
        w[e] = fmt == kPackF16 ? liso_e16::F16::pack(f[0], f[1]) : pack_bf16(f[0], f[1]);
    }
    *reinterpret_cast<uint4*>(dst + q * 8) = make_uint4(w[0], w[1], w[2], w[3]);
}

}  // namespace liso_pack

#endif  // LISO_PACK_CHUNK_H
