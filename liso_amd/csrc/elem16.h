// The two 16-bit storage types of the detector path (include/liso_conv.h: LISO_CONV_BF16 / LISO_CONV_F16), as one set of device
// operations the kernels are templated on, so that each kernel exists once and its fp16 instantiation differs from the bf16 one only in
// these few lines:
//   pack(a, b)  two fp32 values rounded to nearest even, packed low / high into one dword
//   lo(w), hi(w) the fp32 value of the low / high half of a packed dword
//   round(v)    v rounded to the element type and widened back
//   mfma(a, b, c) v_mfma_f32_32x32x16_{bf16,f16} on 8 packed elements per operand (fp32 accumulation).  The A / B lane maps and the
//               C / D layout of the two forms are the same on gfx950, so tiles, LDS images and epilogues carry over unchanged.
// fp32 -> fp16 is a plain conversion (v_cvt_f16_f32 / v_cvt_pk_f16_f32, round to nearest even, overflow to +-inf); never the
// round-toward-zero v_cvt_pkrtz_f16_f32.
#ifndef LISO_ELEM16_H
#define LISO_ELEM16_H
#include <hip/hip_runtime.h>

#include "../../include/liso_conv.h"

namespace liso_e16 {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

struct Bf16 {
    static __device__ __forceinline__ unsigned pack(float a, float b) {
        const __bf16 x = (__bf16)a, y = (__bf16)b;
        return (unsigned)__builtin_bit_cast(unsigned short, x) | ((unsigned)__builtin_bit_cast(unsigned short, y) << 16);
    }
    static __device__ __forceinline__ float lo(unsigned w) { return __uint_as_float(w << 16); }
    static __device__ __forceinline__ float hi(unsigned w) { return __uint_as_float(w & 0xffff0000u); }
    static __device__ __forceinline__ float round(float v) { return (float)(__bf16)v; }
    static __device__ __forceinline__ f32x16 mfma(const uint4& a, const uint4& b, f32x16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    }
    static __device__ __forceinline__ f32x16 mfma(const bf16x8& a, const bf16x8& b, f32x16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
    }
};

struct F16 {
    static __device__ __forceinline__ unsigned pack(float a, float b) {
        const _Float16 x = (_Float16)a, y = (_Float16)b;
        return (unsigned)__builtin_bit_cast(unsigned short, x) | ((unsigned)__builtin_bit_cast(unsigned short, y) << 16);
    }
    static __device__ __forceinline__ float lo(unsigned w) { return (float)__builtin_bit_cast(_Float16, (unsigned short)(w & 0xffffu)); }
    static __device__ __forceinline__ float hi(unsigned w) { return (float)__builtin_bit_cast(_Float16, (unsigned short)(w >> 16)); }
    static __device__ __forceinline__ float round(float v) { return (float)(_Float16)v; }
    static __device__ __forceinline__ f32x16 mfma(const uint4& a, const uint4& b, f32x16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
    }
    // (fragments assembled as bf16 vectors -- the transposing LDS reads of the weight-gradient kernels -- are 16-bit patterns only)
    static __device__ __forceinline__ f32x16 mfma(const bf16x8& a, const bf16x8& b, f32x16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
    }
};

// the 16-bit element of a convolution mode: fp16 for LISO_CONV_F16, bf16 otherwise (bf16 tensors, and the hi / lo planes of F32X3)
template <int MODE>
struct Elem {
    using T = Bf16;
};
template <>
struct Elem<LISO_CONV_F16> {
    using T = F16;
};

}  // namespace liso_e16
#endif  // LISO_ELEM16_H
