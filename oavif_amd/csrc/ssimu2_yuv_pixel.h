// The per-pixel arithmetic of the YUV front ends, each half written once (include/ssimu2_hip_yuv.h is the definition;
// DESIGN.md sections 14 and 16): a sample -> its normalised float, and (Y, Cb, Cr) -> three codes.  ssimu2_yuv.hip
// (4:4:4 and 4:0:0) runs one after the other; ssimu2_chroma.hip (4:2:2 and 4:2:0) blends the normalised chroma samples
// in between.  Device functions only: no kernel and no __constant__ lives here.
#pragma once

#include "ssimu2_div_rn.h"
#include "ssimu2_host.h"

namespace ssimu2 {

using ssimu2h::YuvK;  // the constants of one conversion, formed on the host (yuv_constants)

// First half: the sample `s` of a plane (one above k's max_code is read as it) -> (s - bias) / range, the division
// correctly rounded (div_rn: the divisors are 219..4095, the quotients within +-1.3 -- no operand needs exponent
// scaling).
__device__ __forceinline__ float yuv_unorm(uint32_t s, uint32_t max_code, float bias, float range) {
    return div_rn((float)min(s, max_code) - bias, range);
}

__device__ __forceinline__ uint32_t yuv_code(float c, float top) {
    return (uint32_t)(0.5f + fminf(fmaxf(c, 0.0f), 1.0f) * top);
}

// Second half: the colour matrix.  Every operation rounded once (-ffp-contract=off), the division by kg (0.587..0.7152)
// correctly rounded.
__device__ __forceinline__ void yuv_codes(float Y, float Cb, float Cr, const YuvK& k, uint32_t* code) {
    const float R = Y + k.r_cr * Cr;
    const float B = Y + k.b_cb * Cb;
    const float G = Y - div_rn(2.0f * (k.g_cr * Cr + k.g_cb * Cb), k.kg);
    code[0] = yuv_code(R, k.top);
    code[1] = yuv_code(G, k.top);
    code[2] = yuv_code(B, k.top);
}

}  // namespace ssimu2
