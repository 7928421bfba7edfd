// The per-pixel arithmetic of the YUV front ends, each half written once (include/ssimu2_hip_yuv.h is the definition;
// DESIGN.md sections 14 and 16): a sample -> its normalised float, and (Y, Cb, Cr) -> three codes.  ssimu2_yuv.hip
// (4:4:4 and 4:0:0) runs one after the other; ssimu2_chroma.hip (4:2:2 and 4:2:0) blends the normalised chroma samples
// in between (chroma_blend); ssimu2_yuva.hip does either and composites the codes over a background.  Device functions
// only: no kernel and no __constant__ lives here.
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

// Between the halves, subsampled chroma only (include/ssimu2_hip_chroma.h's bilinear C(i, j)): the blend of the
// normalised sample `a` the pixel lies in, its column neighbour `b`, its row neighbour `c` and the diagonal one `d`,
// every product and sum rounded once, in the header's order.
__device__ __forceinline__ float chroma_blend(float a, float b, float c, float d) {
    return ((a * 0.5625f + b * 0.1875f) + c * 0.1875f) + d * 0.0625f;
}

// Sample `c` of a plane row of S-byte samples (2-byte aligned for S = 2).
template <int S>
__device__ __forceinline__ uint32_t sample_at(const uint8_t* row, uint32_t c) {
    if (S == 1) return row[c];
    uint16_t one;
    __builtin_memcpy(&one, row + 2u * c, 2);
    return one;
}

// N (2 or 4) adjacent samples of a plane row from `p` on, in one load of 2 bytes, one dword or two.
template <int S, int N>
__device__ __forceinline__ void samples_at(const uint8_t* p, uint32_t* out) {
    if constexpr (S * N == 2) {
        uint16_t two;
        __builtin_memcpy(&two, p, 2);
        out[0] = two & 0xFFu;
        out[1] = two >> 8;
    } else {
        uint32_t v[S * N / 4];
#pragma unroll
        for (int k = 0; k < S * N / 4; ++k) __builtin_memcpy(&v[k], p + 4 * k, 4);
#pragma unroll
        for (int i = 0; i < N; ++i)
            out[i] = S == 1 ? (v[0] >> (8 * i)) & 0xFFu : (v[i >> 1] >> (16 * (i & 1))) & 0xFFFFu;
    }
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
