// div_rn: the one arithmetic-contract expression that device code outside ssimu2_kernels.h needs -- the YUV
// front end's colour matrix (ssimu2_yuv.hip) divides with it as the SSIM term does.  It depends on nothing but its
// arguments, so it can live apart from the kernels and c_k: one definition, included by both.
#pragma once

#include <hip/hip_runtime.h>

namespace ssimu2 {

// Correctly rounded a / b for operands that need no exponent scaling (here b is in
// [9e-4, 4], |a| < 4): v_rcp_f32 seed, one Newton step on the reciprocal, two fused
// residual corrections of the quotient -- the sequence hipcc emits for `a / b` minus
// v_div_scale / v_div_fixup, which only act on out-of-range exponents.  Same bits as the
// IEEE division the CPU checker performs.
__device__ __forceinline__ float div_rn(float a, float b) {
    float r = __builtin_amdgcn_rcpf(b);
    const float e0 = fmaf(-b, r, 1.0f);
    r = fmaf(e0, r, r);
    float q = a * r;
    const float e1 = fmaf(-b, q, a);
    q = fmaf(e1, r, q);
    const float e2 = fmaf(-b, q, a);
    return fmaf(e2, r, q);
}

}  // namespace ssimu2
