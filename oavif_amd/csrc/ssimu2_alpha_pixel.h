// The per-sample arithmetic of the front ends that composite over a background, each expression written once
// (include/ssimu2_hip_ext.h and include/ssimu2_hip_yuva.h are the definitions; DESIGN.md sections 13, 17 and 20):
// ssimu2_ext.hip and ssimu2_yuva.hip composite one frame per launch, ssimu2_abatch.hip the frames of a batch.  Device
// functions and the host's forming of their constants only: no kernel and no __constant__ lives here.
#pragma once

#include <stdint.h>

#include <hip/hip_runtime.h>

namespace ssimu2 {

// The composite code of an RGBA8 sample: alpha `a`, colour `c`, background `b`, all 0..255; n <= 255 * 255.
__device__ __forceinline__ uint32_t composite_code(uint32_t a, uint32_t c, uint32_t b) { return a * c + (255u - a) * b; }

// The launch constants of one composite of YUV planes with an alpha plane (formed on the host: yuva_constants).
struct YuvaK {
    uint32_t b[3];   // the background's 8-bit samples
    uint32_t ma, mc; // 2^depth - 1, 2^rgb_depth - 1
    uint32_t den;    // ma * mc: odd, below 2^28
    uint64_t m;      // floor(2^64 / den)
};

// How n's division by den is taken.  DIV_NONE: depth 8 and rgb_depth 8, where n = a c + (255 - a) b exactly and nothing
// is divided.  DIV_MULHI: q = umul64hi(x, floor(2^64 / den)) is floor(x / den) or one below it -- x M / 2^64 lies
// below x / den by less than x / 2^64 < 2^-20 --, so one comparison of the remainder corrects it.  DIV_PLAIN: the
// compiler's 64-bit division, kept for the measurement of DESIGN.md section 17 (OAVIF_YUVA_DIVISION=plain).
enum { DIV_NONE = 0, DIV_MULHI = 1, DIV_PLAIN = 2 };

// The rule: nothing is divided at depth 8 with rgb_depth 8, else the multiply-high form.
inline int yuva_division(uint32_t depth, uint32_t rgb_depth) { return depth == 8 && rgb_depth == 8 ? DIV_NONE : DIV_MULHI; }

// The composite code n of include/ssimu2_hip_yuva.h: alpha `a` (already at most ma), colour code `c`, background `b`.
template <int DIV>
__device__ __forceinline__ uint32_t yuva_code(uint32_t a, uint32_t c, uint32_t b, const YuvaK& k) {
    if (DIV == DIV_NONE) return a * c + (255u - a) * b;
    const uint64_t num = (uint64_t)(a * c) * 255u + (uint64_t)((k.ma - a) * b) * k.mc;  // a c < 2^28, (ma - a) b < 2^20
    const uint64_t x = 255u * num + (k.den - 1u) / 2u;                                  // < 2^44
    if (DIV == DIV_PLAIN) return (uint32_t)(x / k.den);
    uint64_t q = __umul64hi(x, k.m);
    if (x - q * k.den >= k.den) ++q;
    return (uint32_t)q;
}

// The header's integers for one call.
inline YuvaK yuva_constants(uint32_t depth, uint32_t rgb_depth, uint32_t bg) {
    YuvaK k;
    k.b[0] = (bg >> 16) & 0xFFu, k.b[1] = (bg >> 8) & 0xFFu, k.b[2] = bg & 0xFFu;
    k.ma = (1u << depth) - 1u;
    k.mc = (1u << rgb_depth) - 1u;
    k.den = k.ma * k.mc;
    k.m = ~(uint64_t)0 / k.den;  // den is odd and above 1, so it does not divide 2^64: floor((2^64 - 1) / den) is floor(2^64 / den)
    return k;
}

}  // namespace ssimu2
