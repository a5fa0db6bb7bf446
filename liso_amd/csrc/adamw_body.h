// The per-element AdamW update shared by every update kernel of optim.hip (the flat pass, the loss-scaled pass and the pass that also
// writes the convolutions' packed filter panels): one copy, so that every kernel rounds an element the same way.
// Arithmetic and operation order: include/liso_optim.h.
#ifndef LISO_ADAMW_BODY_H
#define LISO_ADAMW_BODY_H

#include <hip/hip_runtime.h>
#include <math.h>

namespace liso_adamw {

struct AdamwScalars {
    float decay;      // 1 - lr * weight_decay
    float w1;         // 1 - beta1
    float beta2, w2;  // beta2, 1 - beta2
    float bc2_sqrt;   // sqrt(1 - beta2^step)
    float eps;
    float step_size;  // lr / (1 - beta1^step)
    float gscale;     // factor on the gradient (1 / world size behind a SUM all-reduce; 1 = none, bit-identical to no factor)
};

__device__ __forceinline__ void adamw_one(float& p, float g, float& m, float& v, const AdamwScalars& s) {
    g = g * s.gscale;
    p = p * s.decay;
    m = fmaf(s.w1, g - m, m);
    v = fmaf(s.w2, g * g, v * s.beta2);
    const float denom = sqrtf(v) / s.bc2_sqrt + s.eps;
    p = fmaf(-s.step_size, m / denom, p);
}

}  // namespace liso_adamw

#endif  // LISO_ADAMW_BODY_H
