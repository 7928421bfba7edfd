// Device code of the MI355X (gfx950) SSIMULACRA2 scorer: every kernel and the constant block c_k that ssimu2_hip.hip
// launches and uploads.  Included by ssimu2_hip.hip and by no other unit of a library (a second copy is a link clash and
// a second c_k); the front ends' kernels are in their own units, and what they share with these is ssimu2_div_rn.h.
//
// Kernels (wave64; VALU + LDS work, no MFMA: stencil and pointwise arithmetic):
//   k_pyramid_bands : linear-light 2x2 box pyramid, all five levels in one launch from one read
//                  of the u8 sRGB frames (through the LUT)
//   k_march      : ONE launch for all scales: per workgroup, a strip of 128 output columns of
//                  one scale is marched top to bottom: sRGB LUT -> opsin -> cbrt -> positive
//                  XYB (converter waves, LDS ring of (ref, dist) pair rows), horizontal 9-tap of
//                  {x, y, xx, yy, xy} in registers, vertical 9-tap from a 9-row register
//                  window, SSIM + edge-difference maps, fp64 partial sums
//   k_finalize   : fixed-order fp64 reduction of the partials, 108 averages, weighted sum,
//                  polynomial, score
//   k_march_map, k_map_compose : the per-pixel error map (ssimu2_error_map_*): densities of every
//                  scale, then their sum at full resolution
//   k_pyramid_bands16, k_pyramid_bands_xyb16, k_march_lin, k_march_refblur_lin : 16-bit input
//                  (ssimu2_*_rgb16 / _strided16)
//   k_pyramid_bands_xyb16_batch : the 16-bit conversion of a whole batch (ssimu2_hbatch_*)
//
// Arithmetic contract: this translation unit is compiled with -ffp-contract=off;
// every fused multiply-add is an explicit fmaf().  The sequence of IEEE operations per pixel
// is fixed and is the one the CPU checker evaluates, because the SSIM map cancels hard in
// fp32 (a 1-ulp difference upstream moves the score by ~1e-3).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ssimu2_hip.h"
#include "ssimu2_div_rn.h"  // div_rn: correctly rounded division (shared with ssimu2_yuv.hip)

namespace ssimu2 {

constexpr int kNumScales = SSIMU2_NUM_SCALES;
constexpr int kStats = SSIMU2_STATS_PER_SCALE;

// ---- constants of the published algorithm (DESIGN.md "Algorithm") -----------------------------
constexpr float kC2 = 0.0009f;
constexpr float kM00 = 0.30f, kM01 = 0.622f, kM02 = 0.078f;
constexpr float kM10 = 0.23f, kM11 = 0.692f, kM12 = 0.078f;
constexpr float kM20 = 0.24342268924547819f, kM21 = 0.20476744424496821f,
                kM22 = 0.55180986650955360f;
constexpr float kOpsinBias = 0.0037930732552754493f;

struct DevConst {
    float lut[256];     // 8-bit sRGB -> linear, fp32(rounded from fp64)
    float taps[5];      // FIR taps |d| = 0..4 of the sigma-1.5 recursive Gaussian
    float cbrt_bias;    // cbrt_repro<true>(kOpsinBias)
    float rg_n2[3];     // the recursion itself (ssimu2_recursive.h): input gains of the three sections
    float rg_d1[3];     // ... and their feedback coefficients -2 cos(omega_k)
    double weights[108];
};
__constant__ DevConst c_k;

// ---- device helpers ---------------------------------------------------------------------------

// Cube root from IEEE mul/fma only (arguments are in [0, 2)): bit-trick seed for y = x^(-1/3), one third-order step
// y (1 + e/3 + 2e^2/9 + 14e^3/81) with e = 1 - x y^3, c = x y^2, one residual-corrected Newton
// step on c.  17 operations, max error 0.76 ulp.  The one definition: the kernels run it, and the host forms
// c_k.cbrt_bias with it (this file is built with -ffp-contract=off, the host's fmaf is the correctly rounded fma).
// GUARD: 0 for x <= 0, for inputs that were clamped to >= 0; without it x must be positive.
template <bool GUARD>
__host__ __device__ __forceinline__ float cbrt_repro(float x) {
    uint32_t i = __builtin_bit_cast(uint32_t, x);
#ifdef __HIP_DEVICE_COMPILE__
    // i / 3 as one multiply-high: floor(i * 0x55555556 / 2^32) == i / 3 for every i < 2^31
    // (checked exhaustively), and the bits of a float below 2.0 are below 2^30
    i = __umulhi(i, 0x55555556u);
#else
    i = i / 3u;
#endif
    i = 0x54A21D2Au - i;
    float y = __builtin_bit_cast(float, i);
    float t = x * y;
    t = t * y;
    t = t * y;
    const float e = 1.0f - t;
    float p = fmaf(e, 14.0f / 81.0f, 2.0f / 9.0f);
    p = fmaf(p, e, 1.0f / 3.0f);
    p = p * e;
    y = fmaf(y, p, y);
    const float y2 = y * y;
    float c = x * y2;
    const float r = fmaf(c * c, c, -x);
    c = fmaf(r, y2 * (-1.0f / 3.0f), c);
    return GUARD ? (x > 0.0f ? c : 0.0f) : c;  // branch-free guard
}

// Linear RGB -> positive XYB as two halves (the marching converters issue the sRGB LUT reads of their next row
// between them): the opsin mix, then clamp, cube roots and the XYB sums.
__device__ __forceinline__ void opsin_mix(float r, float g, float b, float (&lms)[3]) {
    lms[0] = fmaf(kM00, r, fmaf(kM01, g, fmaf(kM02, b, kOpsinBias)));
    lms[1] = fmaf(kM10, r, fmaf(kM11, g, fmaf(kM12, b, kOpsinBias)));
    lms[2] = fmaf(kM20, r, fmaf(kM21, g, fmaf(kM22, b, kOpsinBias)));
}
// CLAMP: the published clamp of the mixed values to >= 0 and the guarded cube root.  The marching kernels go without:
// all they ever see is non-negative linear input (LUT entries and their 2x2 averages are >= 0, so every opsin sum is
// >= the bias), for which clamp and guard can never act -- the same values.
template <bool CLAMP>
__device__ __forceinline__ void mixed_to_xyb(const float (&lms)[3], float (&v)[3]) {
    float l = lms[0], m = lms[1], s = lms[2];
    if (CLAMP) {
        l = fmaxf(l, 0.0f);
        m = fmaxf(m, 0.0f);
        s = fmaxf(s, 0.0f);
    }
    const float cb = c_k.cbrt_bias;
    l = cbrt_repro<CLAMP>(l) - cb;
    m = cbrt_repro<CLAMP>(m) - cb;
    s = cbrt_repro<CLAMP>(s) - cb;
    const float x = 0.5f * (l - m), y = 0.5f * (l + m);
    v[2] = (s - y) + 0.55f;
    v[0] = fmaf(x, 14.0f, 0.42f);
    v[1] = y + 0.01f;
}
__device__ __forceinline__ void linear_to_xyb(float r, float g, float b, float& X, float& Y, float& B) {
    float lms[3], v[3];
    opsin_mix(r, g, b, lms);
    mixed_to_xyb<true>(lms, v);
    B = v[2];
    X = v[0];
    Y = v[1];
}

// symmetric 9-tap in the contract's operation order: one mul, four FMAs.
__device__ __forceinline__ float fir9(float c, float s1, float s2, float s3, float s4, float w0,
                                      float w1, float w2, float w3, float w4) {
    float acc = w0 * c;
    acc = fmaf(w1, s1, acc);
    acc = fmaf(w2, s2, acc);
    acc = fmaf(w3, s3, acc);
    acc = fmaf(w4, s4, acc);
    return acc;
}

// ---- the per-pixel terms ----------------------------------------------------------------------
// What the score sums and the error map weighs, of one pixel of one channel: every kernel that forms them -- FIR or
// recursive blur, score or map -- calls these three, so score and map cannot drift apart (the CPU checker mirrors them).
// The SSIM term from the five blurred values.
__device__ __forceinline__ float ssim_term(float mu1, float mu2, float s11, float s22, float s12) {
    const float mu11 = mu1 * mu1, mu22 = mu2 * mu2, mu12 = mu1 * mu2;
    const float dm = mu1 - mu2;
    const float num_m = fmaf(-dm, dm, 1.0f);
    const float num_s = fmaf(2.0f, s12 - mu12, kC2);
    const float denom_s = ((s11 - mu11) + (s22 - mu22)) + kC2;
    const float d = 1.0f - div_rn(num_m * num_s, denom_s);
    return fmaxf(d, 0.0f);
}
// The edge-difference quotient (1+ea)/(1+eb) - 1, written without its cancellation, from the two blurred values and
// the two frames' pixels.  RN: the correctly rounded quotient, the reference's bits (the recursive modes, whose map is
// held to the checker bit for bit).  Otherwise one reciprocal times the difference (<= 1.5 ulp, the FIR kernels): the
// checker evaluates the FIR map in fp64, so div_rn's rounding bought no agreement there.
template <bool RN>
__device__ __forceinline__ float edge_quotient(float mu1, float mu2, float r1, float r2) {
    const float ea = fabsf(r2 - mu2), eb = fabsf(r1 - mu1);
    return RN ? div_rn(ea - eb, 1.0f + eb) : (ea - eb) * __builtin_amdgcn_rcpf(1.0f + eb);
}
// The six terms d, d^4, art, art^4, det, det^4 in statistic order, handed to put(k, term) one by one: a score adds
// them to its sums, a map collects them for map_density.
template <typename Put>
__device__ __forceinline__ void six_terms(float d, float e, Put put) {
    const float art = fmaxf(e, 0.0f), det = fmaxf(-e, 0.0f);
    const float d2 = d * d, a2 = art * art, t2 = det * det;
    put(0, d);
    put(1, d2 * d2);
    put(2, art);
    put(3, a2 * a2);
    put(4, det);
    put(5, t2 * t2);
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// ---- linear-light pyramid, all five levels from the 8-bit frame in one pass -----------------------
// A BAND is 256 x 32 pixels of the 8-bit frame (aligned to 256 / 32, so every 2x2 source block
// of every level, clamped or not, lies inside it: 32 = 2^5) and is worked on by 512 threads, one
// 4 x 4 pixel block each:
//   level 1 (2 x 2 per thread) and level 2 (1 per thread) in registers -- per thread four rows of
//     12 contiguous bytes = three dword loads each, twelve loads in flight; a wave covers 768
//     contiguous bytes of each of its rows;
//   levels 3, 4, 5 (32 x 4, 16 x 2, 8 x 1 per band) through three small LDS tiles.
// out(ox,oy) = (((p00 + p01) + p10) + p11) * 0.25 with coordinates clamped to the last row /
// column of the level above (the published Downsample(in, 2, 2); the CPU checker's
// or_downsample2), level by level: the same operations in the same order as round 1's
// three-levels-per-launch kernel, whose planes these reproduce bit for bit.
struct PyrBandArgs {
    const uint8_t* in[2];  // frames (tight RGB8)
    float* out[2][5];      // per frame: planes [3][h_l][w_l] of levels 1..5 (entries >= nlevels unused)
    float* xyb0[2];        // XYB variant only: positive-XYB planes [3][h_0][w_0] of the frame itself
    int w[6], h[6];        // level dimensions, [0] = the 8-bit frame
    int opitch[6];         // floats per row of the OUTPUT planes of each level (= w[] for the linear pyramid; the
                           // recursive modes pad their rows to 128 floats, ssimu2_recursive.h "Row pitch")
    int nlevels;           // levels to produce: 1..5; 0 = nothing to do
    int bands_x, bands_y, nframes;
    unsigned* zero4;       // XYB variant: four words zeroed here, the job cursor of the recursive pass that follows (RgPlan::q)
};

// High-bit-depth front end (ssimu2_*_rgb16 / _strided16): the frames are
// host-endian uint16_t RGB (CH = 3) or RGBA (CH = 4, alpha ignored) rows `pitch` bytes apart, and a
// sample s becomes tab[min(s, maxv)], the 2^d-entry table of its frame's depth d (device memory:
// 256 KB at d = 16, too big for __constant__ or beside the kernels' LDS).  The FIR modes also get the
// frame's scale-0 linear planes [3][h][w] (lin0), which the marching kernels read as they read the
// planes of the smaller scales.
struct PyrHbdArgs {
    const uint8_t* in[2];  // first byte of each frame's rows
    uint32_t pitch[2];     // bytes per row
    const float* tab[2];   // sRGB -> linear table of each frame's depth, maxv + 1 entries
    uint32_t maxv[2];      // 2^d - 1: larger samples are clamped to it
    float* lin0[2];        // FIR: scale-0 linear planes of each frame (null in the XYB variant)
};

constexpr int PYR_THREADS = 512;                      // (256-thread bands of 128 pixels measured the same)
constexpr int PYR_TX = PYR_THREADS / 8;               // threads across a band (8 thread rows of 4 pixel rows)
constexpr int PYR_BAND_W = 4 * PYR_TX, PYR_BAND_H = 32;
constexpr int PYR_BAND_LDS_FLOATS = 3 * 8 * PYR_TX + 3 * 4 * (PYR_TX / 2) + 3 * 2 * (PYR_TX / 4);  // levels 2, 3, 4 tiles

__device__ __forceinline__ float box4(float p00, float p01, float p10, float p11) {
    float sum = p00;
    sum += p01;
    sum += p10;
    sum += p11;
    return sum * 0.25f;
}

// Addresses of the pyramid kernels: a WAVE-UNIFORM pointer (a row of a plane or of a frame, formed on the scalar
// unit) plus a per-lane 32-bit BYTE offset -- global_load / global_store v_off, s[base:base+1], no 64-bit VALU
// arithmetic.  The empty asm gives every access an offset register of its own (one v_mov_b32; march_load does the
// same for its cursor): with one offset shared by the planes of a row the compiler adds it to the row pointer
// first and carries the sum through per-lane 64-bit additions.
template <typename T>
__device__ __forceinline__ T* pyr_at(T* row, uint32_t at) {
    asm volatile("" : "+v"(at));
    return (T*)((const char*)row + at);
}

// XYB variant (the recursive blur modes, which read nothing but XYB planes): the positive-XYB
// value of a linear-light pixel goes out instead of the pixel; the linear values stay in
// registers / LDS for the next level.  linear_to_xyb is what k_rg_xyb applies to the same values.
__device__ __forceinline__ void pyr_store_xyb(float* row, size_t n, uint32_t at, const float (&lin)[3]) {
    float X, Y, B;
    linear_to_xyb(lin[0], lin[1], lin[2], X, Y, B);
    *pyr_at(row, at) = X;
    *pyr_at(row + n, at) = Y;
    *pyr_at(row + 2 * n, at) = B;
}

// One level from an LDS tile of the level above: `src` is [3][sh][sw] (tile origin = global
// (2*ox0, 2*oy0) of the level above, whose size is wa x ha), outputs ox0+lx, oy0+ly.
template <bool XYB>
__device__ __forceinline__ void pyr_lds_level(const float* src, int sw, int sh, int wa, int ha, float* dst_tile,
                                              int dw_tile, int dh_tile, float* out, int wo, int ho, int po, int ox0,
                                              int oy0, int lx, int ly) {
    const int ox = ox0 + lx, oy = oy0 + ly;
    float v[3] = {0.f, 0.f, 0.f};
    if (ox < wo && oy < ho) {
        const int xa = 2 * lx, xb = min(2 * ox + 1, wa - 1) - 2 * ox0;
        const int ya = 2 * ly, yb = min(2 * oy + 1, ha - 1) - 2 * oy0;
        const size_t n = (size_t)po * ho;
        float* origin = out + (size_t)oy0 * po + ox0;              // the tile's first output: the same for every lane
        const uint32_t at = 4u * (uint32_t)(ly * po + lx);         // ly < 4: a few rows of bytes, far inside 32 bits
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float* p = src + c * sw * sh;
            v[c] = box4(p[ya * sw + xa], p[ya * sw + xb], p[yb * sw + xa], p[yb * sw + xb]);
            if (!XYB) *pyr_at(origin + c * n, at) = v[c];
        }
        if (XYB) pyr_store_xyb(origin, n, at, v);
    }
    if (dst_tile) {
#pragma unroll
        for (int c = 0; c < 3; ++c) dst_tile[(c * dh_tile + ly) * dw_tile + lx] = v[c];
    }
}

// Linear values of one thread's 4 x 4 block of a 16-bit frame: per row 2 * CH contiguous dwords
// (24 / 32 bytes, unaligned dword loads), all four rows in flight before the table gathers; at the
// frame border clamped coordinates, one 16-bit load per sample.
// BATCH (k_pyramid_bands_xyb16_batch): the frame lies `in_off` bytes behind hb.in[f] -- item i of a batch.
template <int CH, bool BATCH = false>
__device__ __forceinline__ void pyr_load16(const PyrHbdArgs& hb, int f, int w0, int h0, int X0, int Y0, bool inside,
                                           float (&lin)[4][4][3], size_t in_off = 0) {
    const uint8_t* base = hb.in[f];
    if constexpr (BATCH) base += in_off;
    const uint32_t pitch = hb.pitch[f], maxv = hb.maxv[f];
    const float* tab = hb.tab[f];
    uint32_t s[4][4][3];
    if (inside) {
        uint32_t raw[4][2 * CH];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint8_t* p = base + (size_t)(Y0 + j) * pitch + (size_t)X0 * (2 * CH);
#pragma unroll
            for (int k = 0; k < 2 * CH; ++k) __builtin_memcpy(&raw[j][k], p + 4 * k, 4);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int e = CH * i + c;  // 16-bit element of the row's run
                    s[j][i][c] = (raw[j][e >> 1] >> (16 * (e & 1))) & 0xFFFFu;
                }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint8_t* row = base + (size_t)min(Y0 + j, h0 - 1) * pitch;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const uint16_t* p = (const uint16_t*)(row + (size_t)min(X0 + i, w0 - 1) * (2 * CH));
#pragma unroll
                for (int c = 0; c < 3; ++c) s[j][i][c] = p[c];
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int c = 0; c < 3; ++c) lin[j][i][c] = tab[min(s[j][i][c], maxv)];
}

// `lut`: 256 floats of LDS that receive the sRGB table here; `lds`: PYR_BAND_LDS_FLOATS floats of scratch; 512
// threads, all of which must call (barriers inside).  `band` < bands_x * bands_y * nframes.
// CH16 = 0: 8-bit frames through the LDS table `lut`; 3 / 4: 16-bit RGB / RGBA frames of `hb`.
// BATCH (k_pyramid_bands_batch): `in_off` (bytes) / `out_off` (floats) are added to the frame's input and to each of
// its output levels -- item i of a batch.
// Addresses: a wave is one thread row (PYR_TX = 64 lanes), so the thread row, every pixel row and every output row
// are the same for all its lanes.  Each row's address is formed once, on the scalar unit, from the band's first
// column; a lane adds a 32-bit byte offset inside the band (< 256 pixels * 16 bytes).
template <bool XYB, int CH16 = 0, bool BATCH = false>
__device__ __forceinline__ void pyramid_band(const PyrBandArgs& a, int band, float* lut, float* lds,
                                             const PyrHbdArgs* hb = nullptr, size_t in_off = 0, size_t out_off = 0) {
    const int t = threadIdx.x;
    const int per_frame = a.bands_x * a.bands_y;
    const int f = band / per_frame;
    const int r = band - f * per_frame;
    const int by = r / a.bands_x, bx = r - by * a.bands_x;
    const int w0 = a.w[0], h0 = a.h[0], w1 = a.w[1], h1 = a.h[1];
    constexpr int TX = PYR_TX;
    static_assert(TX == 64, "one thread row per wave: ty below is read from lane 0");
    float* s2 = lds;                       // [3][8][TX]
    float* s3 = s2 + 3 * 8 * TX;           // [3][4][TX/2]
    float* s4 = s3 + 3 * 4 * (TX / 2);     // [3][2][TX/4]
    const int tx = t % TX, ty = __builtin_amdgcn_readfirstlane(t / TX);
    const int XB = bx * PYR_BAND_W;        // the band's first column
    const int X0 = XB + 4 * tx, Y0 = by * PYR_BAND_H + 4 * ty;
    const bool work = X0 < w0 && Y0 < h0;
    const bool inside = X0 + 3 < w0 && Y0 + 3 < h0;
    uint32_t raw[4][3];  // CH16 = 0: this thread's four rows of 12 bytes
    if constexpr (CH16 == 0) {
        // The table entry and the frame bytes are requested together, before the table is stored and the barrier
        // passed: one memory latency, not two in a row.
        const float entry = c_k.lut[t & 255];
        if (work) {
            const uint8_t* base = a.in[f];
            if constexpr (BATCH) base += in_off;
            if (inside) {  // four rows of 12 contiguous bytes
                // X0 + 3 < w0 and Y0 + j <= Y0 + 3 < h0: bytes 3 * ((Y0 + j) * w0 + X0) + 0..11 are pixels X0..X0+3
                // of row Y0 + j, the last of them at most byte 3 * w0 * h0 - 1, the frame's last.
                const uint8_t* row0 = base + ((size_t)Y0 * w0 + XB) * 3;
                const uint32_t at = 12u * tx;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint8_t* p = pyr_at(row0 + (size_t)j * w0 * 3, at);
#pragma unroll
                    for (int k = 0; k < 3; ++k) __builtin_memcpy(&raw[j][k], p + 4 * k, 4);
                }
            } else {  // frame border: clamped coordinates (row <= h0 - 1, column <= w0 - 1), byte by byte
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint8_t* row = base + ((size_t)min(Y0 + j, h0 - 1) * w0 + XB) * 3;
                    uint8_t b[12];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const uint8_t* p = pyr_at(row, 3u * (uint32_t)(min(X0 + i, w0 - 1) - XB));
                        b[3 * i] = p[0];
                        b[3 * i + 1] = p[1];
                        b[3 * i + 2] = p[2];
                    }
#pragma unroll
                    for (int k = 0; k < 3; ++k)
                        raw[j][k] = (uint32_t)b[4 * k] | ((uint32_t)b[4 * k + 1] << 8) | ((uint32_t)b[4 * k + 2] << 16) |
                                    ((uint32_t)b[4 * k + 3] << 24);
                }
            }
        }
        if (t < 256) lut[t] = entry;
        __syncthreads();
    }
    // ---- levels 1 and 2 in registers
    float v2[3] = {0.f, 0.f, 0.f};  // this thread's level-2 output
    if (work) {
        float lin16[4][4][3];  // CH16: linear values of this thread's 4 x 4 pixels
        if constexpr (CH16 != 0) pyr_load16<CH16, BATCH>(*hb, f, w0, h0, X0, Y0, inside, lin16, in_off);
        // byte 3*i + c of a row = channel c of pixel i
#define PYR_LIN(j, i, c) \
    (CH16 ? lin16[j][i][c] : lut[(raw[j][(3 * (i) + (c)) >> 2] >> (8 * ((3 * (i) + (c)) & 3))) & 255u])
        float l1[2][2][3];  // [row][col][channel] of this thread's 2 x 2 level-1 outputs
        const int p1 = a.opitch[1];
        const size_t n1 = (size_t)p1 * h1;
        float* o1 = a.out[f][0];
        if constexpr (BATCH) o1 += out_off;
        const int ox1 = X0 >> 1, oy1 = Y0 >> 1;
        // the two floats of a row go out as one 8-byte store where every such pair is 8-byte aligned: plane, pitch
        // (hence plane size) and the lane's offset 8 * tx all even in floats
        const bool pairs = !XYB && (p1 & 1) == 0 && ((uintptr_t)o1 & 7) == 0;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    l1[j][i][c] = box4(PYR_LIN(2 * j, 2 * i, c), PYR_LIN(2 * j, 2 * i + 1, c),
                                       PYR_LIN(2 * j + 1, 2 * i, c), PYR_LIN(2 * j + 1, 2 * i + 1, c));
            if (oy1 + j < h1 && (!XYB || a.nlevels >= 1)) {
                float* row = o1 + (size_t)(oy1 + j) * p1 + (XB >> 1);
                const uint32_t at = 8u * tx;
                if (XYB) {
#pragma unroll
                    for (int i = 0; i < 2; ++i)
                        if (ox1 + i < w1) pyr_store_xyb(row, n1, at + 4 * i, l1[j][i]);
                } else if (pairs && ox1 + 1 < w1) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) *(float2*)pyr_at(row + c * n1, at) = make_float2(l1[j][0][c], l1[j][1][c]);
                } else {
#pragma unroll
                    for (int i = 0; i < 2; ++i)
                        if (ox1 + i < w1) {
#pragma unroll
                            for (int c = 0; c < 3; ++c) *pyr_at(row + c * n1, at + 4 * i) = l1[j][i][c];
                        }
                }
            }
        }
        if constexpr (CH16 != 0 && !XYB) {  // FIR: the frame's scale-0 linear planes, a row of four pixels at a time
            const size_t n0 = (size_t)w0 * h0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float* row = hb->lin0[f] + (size_t)(Y0 + j) * w0 + XB;
                const uint32_t at = 16u * tx;
                if (inside) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const float px[4] = {lin16[j][0][c], lin16[j][1][c], lin16[j][2][c], lin16[j][3][c]};
                        __builtin_memcpy(pyr_at(row + c * n0, at), px, 16);
                    }
                } else if (Y0 + j < h0) {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (X0 + i < w0) {
#pragma unroll
                            for (int c = 0; c < 3; ++c) *pyr_at(row + c * n0, at + 4 * i) = lin16[j][i][c];
                        }
                }
            }
        }
        if (XYB) {  // the frame's own XYB planes: this thread's 4 x 4 pixels, a row of four at a time
            const int p0 = a.opitch[0];
            const size_t n0 = (size_t)p0 * h0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float px[3][4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    linear_to_xyb(PYR_LIN(j, i, 0), PYR_LIN(j, i, 1), PYR_LIN(j, i, 2), px[0][i], px[1][i], px[2][i]);
                }
                float* row = a.xyb0[f] + (size_t)(Y0 + j) * p0 + XB;
                if constexpr (BATCH) row += out_off;
                const uint32_t at = 16u * tx;
                if (inside) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) __builtin_memcpy(pyr_at(row + c * n0, at), px[c], 16);
                } else if (Y0 + j < h0) {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (X0 + i < w0) {
#pragma unroll
                            for (int c = 0; c < 3; ++c) *pyr_at(row + c * n0, at + 4 * i) = px[c][i];
                        }
                }
            }
        }
#undef PYR_LIN
        const int w2 = a.w[2], h2 = a.h[2];
        const int ox = X0 >> 2, oy = Y0 >> 2;  // = 64 bx + tx, 8 by + ty
        if (a.nlevels >= 2 && ox < w2 && oy < h2) {
            // the level-1 column / row 2*ox+1, 2*oy+1 may not exist: the published clamp repeats the last one
            const int ib = min(2 * ox + 1, w1 - 1) - 2 * ox, jb = min(2 * oy + 1, h1 - 1) - 2 * oy;
            const int p2 = a.opitch[2];
            const size_t n2 = (size_t)p2 * h2;
            float* row = a.out[f][1] + (size_t)oy * p2 + (XB >> 2);
            if constexpr (BATCH) row += out_off;
            const uint32_t at = 4u * tx;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float p01 = ib ? l1[0][1][c] : l1[0][0][c];
                const float p10 = jb ? l1[1][0][c] : l1[0][0][c];
                const float p11 = jb ? (ib ? l1[1][1][c] : l1[1][0][c]) : (ib ? l1[0][1][c] : l1[0][0][c]);
                v2[c] = box4(l1[0][0][c], p01, p10, p11);
                if (!XYB) *pyr_at(row + c * n2, at) = v2[c];
            }
            if (XYB) pyr_store_xyb(row, n2, at, v2);
        }
    }
    if (a.nlevels < 2) return;
    // a thread outside the frame (no `work`) has X0 / 4 >= w[2] or Y0 / 4 >= h[2] and stores 0, as one whose level-2
    // output does not exist always did
#pragma unroll
    for (int c = 0; c < 3; ++c) s2[(c * 8 + ty) * TX + tx] = v2[c];
    if (a.nlevels < 3) return;
    __syncthreads();
    if (t < 4 * (TX / 2))
        pyr_lds_level<XYB>(s2, TX, 8, a.w[2], a.h[2], s3, TX / 2, 4, BATCH ? a.out[f][2] + out_off : a.out[f][2], a.w[3], a.h[3], a.opitch[3], bx * (TX / 2), by * 4,
                      t % (TX / 2), t / (TX / 2));
    if (a.nlevels < 4) return;
    __syncthreads();
    if (t < 2 * (TX / 4))
        pyr_lds_level<XYB>(s3, TX / 2, 4, a.w[3], a.h[3], s4, TX / 4, 2, BATCH ? a.out[f][3] + out_off : a.out[f][3], a.w[4], a.h[4], a.opitch[4], bx * (TX / 4), by * 2,
                      t % (TX / 4), t / (TX / 4));
    if (a.nlevels < 5) return;
    __syncthreads();
    if (t < TX / 8)
        pyr_lds_level<XYB>(s4, TX / 4, 2, a.w[4], a.h[4], nullptr, 0, 0, BATCH ? a.out[f][4] + out_off : a.out[f][4], a.w[5], a.h[5], a.opitch[5], bx * (TX / 8), by, t, 0);
}

// The pair score's pyramid runs beside the other context's marching kernel, in the slot a marching workgroup has left
// ("Two scores in flight"): it holds that slot for as long as it lives.  Its few instructions
// would wait their turn behind the marching waves that saturate the SIMD's issue; at a higher issue priority they go
// first and the slot is back sooner.
__device__ __forceinline__ void pyr_issue_first() { __builtin_amdgcn_s_setprio(3); }

__global__ __launch_bounds__(PYR_THREADS) void k_pyramid_bands(PyrBandArgs a) {
    __shared__ float s_lut[256];
    __shared__ float s_tiles[PYR_BAND_LDS_FLOATS];
    pyr_issue_first();
    pyramid_band<false>(a, (int)blockIdx.x, s_lut, s_tiles);
}

// The band pyramid of a BATCH (ssimu2_score_batch_*): `a` describes item 0 -- a.nframes (2: reference and distorted,
// 1: distorted only) frames of one size -- and item i's frames and levels lie i * stride further on.  Grid:
// [item][frame][band]; per frame the arithmetic of k_pyramid_bands, so an item's planes do not depend on the batch.
struct PyrBatchArgs {
    PyrBandArgs a;
    size_t in_stride;   // bytes between the 8-bit frames of consecutive items
    size_t out_stride;  // floats between their linear pyramids
};
__global__ __launch_bounds__(PYR_THREADS) void k_pyramid_bands_batch(PyrBatchArgs b) {
    __shared__ float s_lut[256];
    __shared__ float s_tiles[PYR_BAND_LDS_FLOATS];
    pyr_issue_first();
    const int per_item = b.a.bands_x * b.a.bands_y * b.a.nframes;
    const int item = (int)blockIdx.x / per_item;
    pyramid_band<false, 0, true>(b.a, (int)blockIdx.x - item * per_item, s_lut, s_tiles, nullptr, (size_t)item * b.in_stride,
                        (size_t)item * b.out_stride);
}

// The same bands with positive-XYB planes of every level -- the frame's own included -- as the
// output instead of the linear-light levels: the one conversion launch of the recursive blur modes.
__global__ __launch_bounds__(PYR_THREADS) void k_pyramid_bands_xyb(PyrBandArgs a) {
    __shared__ float s_lut[256];
    __shared__ float s_tiles[PYR_BAND_LDS_FLOATS];
    if (blockIdx.x == 0 && threadIdx.x < 4 && a.zero4) a.zero4[threadIdx.x] = 0u;  // k_rg_v starts after this launch has ended
    pyramid_band<true>(a, (int)blockIdx.x, s_lut, s_tiles);
}

// The batch of the recursive modes (ssimu2_rbatch_*): PyrBatchArgs as k_pyramid_bands_batch takes them, out_stride
// the floats between two items' plane sets (every level and the frames' own XYB planes lie in one set per item).
__global__ __launch_bounds__(PYR_THREADS) void k_pyramid_bands_xyb_batch(PyrBatchArgs b) {
    __shared__ float s_lut[256];
    __shared__ float s_tiles[PYR_BAND_LDS_FLOATS];
    if (blockIdx.x == 0 && threadIdx.x < 4 && b.a.zero4) b.a.zero4[threadIdx.x] = 0u;  // k_rg_v_batch starts after this launch has ended
    const int per_item = b.a.bands_x * b.a.bands_y * b.a.nframes;
    const int item = (int)blockIdx.x / per_item;
    pyramid_band<true, 0, true>(b.a, (int)blockIdx.x - item * per_item, s_lut, s_tiles, nullptr, (size_t)item * b.in_stride,
                                (size_t)item * b.out_stride);
}

// The 16-bit counterparts (CH = 3: tight or padded RGB rows; 4: RGBA rows, alpha dropped here).
// FIR: levels 1..5 as k_pyramid_bands and the frame's scale-0 linear planes.
template <int CH>
__global__ __launch_bounds__(PYR_THREADS) void k_pyramid_bands16(PyrBandArgs a, PyrHbdArgs hb) {
    __shared__ float s_tiles[PYR_BAND_LDS_FLOATS];
    pyramid_band<false, CH>(a, (int)blockIdx.x, nullptr, s_tiles, &hb);
}

// Recursive modes: XYB planes of every level, as k_pyramid_bands_xyb.
template <int CH>
__global__ __launch_bounds__(PYR_THREADS) void k_pyramid_bands_xyb16(PyrBandArgs a, PyrHbdArgs hb) {
    __shared__ float s_tiles[PYR_BAND_LDS_FLOATS];
    if (blockIdx.x == 0 && threadIdx.x < 4 && a.zero4) a.zero4[threadIdx.x] = 0u;  // k_rg_v starts after this launch has ended
    __syncthreads();
    pyramid_band<true, CH>(a, (int)blockIdx.x, nullptr, s_tiles, &hb);
}

// The 16-bit batch of the recursive modes (ssimu2_hbatch_*): `b` as k_pyramid_bands_xyb_batch
// takes it, in_stride the bytes between the 16-bit frames of consecutive items, and `hb` describes item 0's frames --
// one pitch, table and top code for the whole batch.  Grid: [item][frame][band]; per frame the arithmetic of
// k_pyramid_bands_xyb16, so an item's planes do not depend on the batch.
template <int CH>
__global__ __launch_bounds__(PYR_THREADS) void k_pyramid_bands_xyb16_batch(PyrBatchArgs b, PyrHbdArgs hb) {
    __shared__ float s_tiles[PYR_BAND_LDS_FLOATS];
    if (blockIdx.x == 0 && threadIdx.x < 4 && b.a.zero4) b.a.zero4[threadIdx.x] = 0u;  // k_rg_v_batch starts after this launch has ended
    __syncthreads();
    const int per_item = b.a.bands_x * b.a.bands_y * b.a.nframes;
    const int item = (int)blockIdx.x / per_item;
    pyramid_band<true, CH, true>(b.a, (int)blockIdx.x - item * per_item, nullptr, s_tiles, &hb, (size_t)item * b.in_stride,
                                 (size_t)item * b.out_stride);
}

// ---- fused per-scale kernel, marching form, all scales in one launch ----------------------------
// One workgroup (8 waves) owns a strip of MW output columns (MarchGeo below) of ONE scale and marches down
// `seg` output rows, one image row per step.
//   waves 0-1 (converters): lane = one staged column (of MW + 8; the wide geometry's last eight: halo pass), both frames.  Each
//     step they convert one input row (sRGB LUT at scale 0 -> opsin -> cbrt -> positive XYB)
//     into an LDS ring of raw rows, one barrier group ahead of the blur waves; their global
//     loads run one more group ahead, so HBM latency is off the critical path.  At scale 0 a
//     lane fetches its pixel with ONE dword load (the three bytes of the pixel plus one of the
//     next), the wave's loads covering a contiguous 193-byte run of the row.
//   waves 2-7 (blur + maps): two waves per XYB channel, lane = one output column.  Each step
//     a lane reads its 9-wide window of (x, y) = (ref, dist) pairs from the ring, forms the
//     products, does the horizontal 9-tap of the five planes {x, y, xx, yy, xy} in
//     registers and pushes the results into a 9-row register window, from which the
//     vertical 9-tap and the SSIM / edge-difference maps of the row four steps back are
//     evaluated and accumulated.  The row loop is unrolled nine times so the window is
//     addressed with compile-time indices (no register moves).
//     LDS latency is taken off the critical path without extra registers: the five inner
//     window pairs of the NEXT row are requested right after the horizontal pass of this row
//     (when the tap registers are dead) and land under the vertical pass and the maps; the
//     four outer pairs are requested at the top of the step and land under the partial sums
//     of the inner ones.
// One output pixel per lane keeps the window at 45 registers, and the two roles run separate
// loops (own register allocation): <= 80 VGPRs, 3 workgroups = 24 waves per CU.  A lone wave
// issues a VALU op only every ~4 cycles, so occupancy is what fills the SIMDs.
// The workgroup synchronises once per GROUP rows; in the blur waves the barrier sits between
// the horizontal pass of the group's last row and the prefetch for the next group's first.
// HBM traffic: each input pixel is read once per strip (+8/MW horizontal, +8/seg vertical
// halo); only 18 partial sums per workgroup are written.
// Scales are laid out largest first in the grid, so the short workgroups of the small scales
// fill the tail of the big ones instead of running as five latency-bound launches.
constexpr int RAD = 4;
constexpr int RING = 16;       // raw-row ring depth (power of two >= 13: rows t-4 .. t+8)
constexpr int AHEAD = 3;       // rows the converters run ahead of the blur waves (1 group)
constexpr int GROUP = 3;       // rows per barrier interval (divides the 9-phase unroll)
constexpr int MARCH_THREADS = 512;
constexpr int CONV_WAVES = 2;  // each converter lane handles one staged column of BOTH frames

// One ring element: the positive-XYB value of one channel of one staged pixel in both frames,
// .x = reference, .y = distorted.  Keeping the pair together makes every tap of the blur
// waves one naturally aligned ds_read_b64 (256 B/clk/CU; the planar layout needed
// ds_read2_b32, 128 B/clk/CU) and every converter store one ds_write_b64.
typedef float f2 __attribute__((ext_vector_type(2)));

// Strip geometry of a marching kernel (a template parameter of the marching body: each entry point names its own).
//   MarchNarrow  120 output columns, 128 staged: one staged column per converter lane; lanes 60..63 of every blur wave
//                idle.  The kernels that write planes (k_ref_blur, the map kernels).
//   MarchWide    128 output columns, 136 staged: every blur-wave lane owns a column.  The converter lanes stage columns
//                0..127 as before; the 8 columns behind them are converted six rows at a time, once per pair of barrier
//                groups (march_convert_rows, "halo pass").  Every kernel whose partial sums k_finalize reads: the fp64
//                part of a sum is grouped by wave and tile, so those kernels share one geometry and a pair score, a
//                pass against the cached reference, a batch item and a 16-bit score of the same pixels keep equal bits.
template <int W>
struct MarchGeo {
    static constexpr int MW = W;              // output columns per strip
    static constexpr int MRW = W + 2 * RAD;   // staged columns (4 px halo each side)
    static constexpr int MHALF = W / 2;       // output columns per blur wave
    static constexpr int HALO = MRW - 128;    // staged columns behind the 128 converter lanes
    static constexpr int RING_ROW = 3 * MRW;  // f2 elements per ring row: [channel][column]
    static_assert(MHALF <= 64 && (HALO == 0 || HALO == 8), "two blur waves per channel, 128 converter lanes");
};
typedef MarchGeo<120> MarchNarrow;
typedef MarchGeo<128> MarchWide;

struct MarchPlan {
    int nscales;
    int blk_end[kNumScales];   // exclusive end of each scale's block range in the grid
    int w[kNumScales], h[kNumScales], seg[kNumScales], nstrips[kNumScales], nblocks[kNumScales];
    const void* ref[kNumScales];   // scale 0: u8 interleaved; others: fp32 planes
    const void* dist[kNumScales];
    const float* ref_xyb[kNumScales];  // cached positive-XYB planes of the reference, or null
    // blur(ref*ref) planes [3][h][w] of the scale: read by MARCH_REFBLUR (cached once per
    // search), written by MARCH_EMIT
    float* ref_s11[kNumScales];
    double* part[kNumScales];      // [18][nblocks] partial sums of the scale
};

// Kernel modes of the marching body (one __global__ entry each, so every mode has its own
// register allocation and the pair-score kernel is untouched by the others):
//   MARCH_PAIR     both frames blurred in flight (any pair; what `value` measures)
//   MARCH_REFBLUR  s11 = blur(ref*ref), which depends on the reference alone, comes from planes
//                  cached once per search (tq.zig:37 passes the same e.rgb on every pass); the blur
//                  waves keep four planes instead of five.  Same operations on the same operands,
//                  so the score's bits do not move.  mu1 = blur(ref) depends on the reference
//                  alone too, but caching it as well makes the kernel HBM-bound and slower
//                  (measured): one cached plane is the balance point.
//   MARCH_EMIT     writes that plane (run once by ssimu2_set_reference)
//   MARCH_MAP      both frames as MARCH_PAIR, but each lane writes its pixel's error-map density
//                  (map_density) into the [3][h][w] plane the plan passes in
//                  ref_s11 instead of accumulating sums (ssimu2_error_map_*)
enum { MARCH_PAIR = 0, MARCH_REFBLUR = 1, MARCH_EMIT = 2, MARCH_MAP = 3 };

// Per-lane cursor of a blur wave over the cached / emitted reference blur planes of its channel:
// the pixel of this lane's column in the next output row, plus a prefetch queue (the values are
// loaded RB_AHEAD steps before the step that consumes them; HBM latency under load is several
// row steps).
constexpr int RB_AHEAD = 6;  // round 4: 4 / 6 / 8 = 0.1621 / 0.1597 / 0.1636 ms per cached 4K pass (profiles/r04_refblur_ab.log)
struct MarchRefBlur {
    float* s11;
    int pitch;       // elements per row
    int rows_left;   // rows of this segment not loaded yet
    bool active;     // lane owns an output column (lanes >= MarchNarrow::MHALF of a blur wave only shadow lane 0)
    float ps11[9];  // slot = phase of the consuming step; RB_AHEAD of them are live
};

// Error-map coefficients, [scale][18] in the statistic order of the averages (w, or w / a^3 for an L4
// statistic); ssimu2_hip.hip computes them from the 108 averages of the score before the map pass.
struct MapCoef {
    float c[kNumScales][kStats];
};

// The six per-pixel terms whose plane means / L4 norms are the averages, and the channel's
// density from them: sum of mc[k] * term[k] in term order (the error map's definition).
__device__ __forceinline__ float map_density(const float (&t)[6], const float (&mc)[6]) {
    float v = mc[0] * t[0];
#pragma unroll
    for (int k = 1; k < 6; ++k) v = fmaf(mc[k], t[k], v);
    return v;
}
// Where term k of channel c sits among a scale's 18 statistics, as k_finalize reads them: 0..5 ssim (c*2 + n),
// 6..17 edge (c*4 + j).
__device__ __forceinline__ int term_stat(int c, int k) { return k < 2 ? c * 2 + k : 6 + c * 4 + (k - 2); }

// ---- converter waves ------------------------------------------------------------------------------
// Per-lane read cursor of a converter lane over one frame: address of this lane's
// (column-clamped) pixel in the next row to load, advanced by one row pitch per load.
//   u8 frames (scale 0): ONE unaligned dword load per pixel -- R | G << 8 | B << 16 | the next
//     pixel's R << 24 -- so a wave's loads cover one contiguous 193-byte run of the row.  The
//     lane of the image's last column reads one byte earlier and shifts (`shift` = 8), so no
//     load ever reaches behind the frame's last byte.
//   fp32 planes (scales >= 1, cached reference XYB): three dword loads, `plane` elements apart.
struct MarchCursor {
    const uint8_t* base;  // uniform: first byte of the frame / of the first plane
    uint32_t off;         // per lane: byte offset of this lane's pixel inside a row
    size_t plane;         // bytes between planes (fp32 sources)
    int pitch;            // bytes per row
    uint32_t shift;       // u8 only
};

template <bool U8>
__device__ __forceinline__ MarchCursor march_cursor(const void* base, int w, int h, int gxc) {
    MarchCursor c;
    c.plane = (size_t)w * h * 4;
    c.pitch = U8 ? w * 3 : w * 4;
    const bool last_col = U8 && gxc == w - 1;
    c.shift = last_col ? 8u : 0u;
    c.base = (const uint8_t*)base;
    c.off = (uint32_t)gxc * (U8 ? 3u : 4u) - (last_col ? 1u : 0u);
    return c;
}

// Load this lane's pixel of image row `row` (uniform; clamped into the image by the caller, so
// the load is unconditional: every row issues the same number of loads and the compiler's
// s_waitcnt vmcnt(N) can count them -- a conditional load made it fall back to vmcnt(0), which
// shortened the prefetch distance to one row).
// Addressing: the row's address is uniform (scalar arithmetic) and the lane's 32-bit offset is added by
// the load itself (global_load_dword v, v_off, s[base:base+1]): no VALU for the address.  The compiler
// only selects that form when it sees the offset's zero extension in the load's own basic block; the
// offset is loop-invariant, so without the empty asm it would hoist the extension out of the loop and
// form every address with a 64-bit VALU add (v_lshl_add_u64 / v_mad_u64_u32).  The asm rewrites the
// cursor's own offset (not a copy), so the register carried round the loop is its output: no v_mov.
template <bool U8>
__device__ __forceinline__ void march_load(uint32_t (&raw)[3], MarchCursor& c, int row) {
    const uint8_t* p = c.base + (size_t)(uint32_t)row * (uint32_t)c.pitch;
    asm volatile("" : "+v"(c.off));
    const uint32_t off = c.off;
    if (U8) {
        uint32_t d;
        __builtin_memcpy(&d, p + off, 4);
        raw[0] = d;
    } else {
        raw[0] = *(const uint32_t*)(p + off);
        raw[1] = *(const uint32_t*)((p + c.plane) + off);
        raw[2] = *(const uint32_t*)((p + 2 * c.plane) + off);
    }
}

// One copy of the table: four interleaved copies were no faster (profiles/r03_lut_ab.log; a
// ds_read_b32 serves 32 lanes from 32 banks whichever copy a lane reads).
__device__ __forceinline__ void march_lut(const float* lut, uint32_t d, uint32_t shift, float (&lin)[3]) {
    d >>= shift;
    lin[0] = lut[d & 255u];
    lin[1] = lut[(d >> 8) & 255u];
    lin[2] = lut[(d >> 16) & 255u];
}

// The converter role of one workgroup: rows 0 .. steps-1 of the segment into the ring, GROUP
// rows per barrier interval, global loads GROUP rows ahead of their use.
//   U8    the frames are 8-bit sRGB (scale 0); otherwise fp32 linear-light planes
//   MODE  MARCH_PAIR: both frames converted.  MARCH_REFBLUR: frame 0 is the cached positive-XYB
//         planes of the reference (no arithmetic).  MARCH_EMIT: the same, and frame 1 is not needed.
// Per row and lane: [LUT values of this row, requested one row earlier] -> opsin mix of both
// frames -> request the LUT values of the next row -> cube roots, XYB, one ds_write_b64 per
// channel.  The LUT reads therefore land under ~100 arithmetic instructions.
// LIN0: instantiated for the kernels of march_body<MODE, true> (same code; an instantiation of their own leaves the
// code generated for the 8-bit kernels as it was).
// G::HALO (MarchWide): the halo pass.  Staged columns 128..135 have no converter lane of their own; wave f converts
// them for frame f alone, six rows at a time: lane L takes row L >> 3 of the six and column 128 + (L & 7) and writes
// the frame's 4-byte half of the ring element (lanes 48..63 repeat lanes 40..47: the same value to the same
// address, so nothing is masked).  The pass for rows 3g .. 3g+5 runs at the head of even group g, so rows 3g+3 ..
// 3g+5 of those columns are written one group early, into slots that held rows <= 3g-11 while the oldest row the
// blur waves still read is 3g-8: the ring depth holds.  Its loads go out one pass (six rows) ahead, unconditional
// and in the SGPR-base form like the others; clamping rows into the image and the zero padding sit behind uniform
// branches that only the first and last segment and the image's last strips take.
template <typename G, bool U8, int MODE, bool LIN0 = false, bool BATCH = false>
__device__ __forceinline__ void march_convert_rows(f2 (*ring)[3][G::MRW], const float* lut,
                                                   const MarchPlan& plan, int sc, int w, int h, int x0,
                                                   int y0, int steps, int ngroups, int col, size_t off0 = 0,
                                                   size_t off1 = 0) {
    // BATCH: off0 / off1 are the uniform byte offsets of this workgroup's item from plan.ref[sc] / plan.dist[sc]
    // (the cached reference planes are shared by every item).
    constexpr bool CACHED = MODE == MARCH_REFBLUR || MODE == MARCH_EMIT;
    constexpr bool TWO = MODE != MARCH_EMIT;
    constexpr bool LUT0 = U8 && !CACHED;  // frame 0 goes through the sRGB LUT
    const int gx = x0 - RAD + col;
    const bool col_ok = gx >= 0 && gx < w;
    const bool all_cols = x0 - RAD >= 0 && x0 - RAD + G::MRW <= w;  // uniform: no lane outside the image
    const int gxc = min(max(gx, 0), w - 1);  // clamped: the value is discarded when gx is outside
    MarchCursor c0 = CACHED ? march_cursor<false>(plan.ref_xyb[sc], w, h, gxc)
                            : march_cursor<U8>(plan.ref[sc], w, h, gxc);
    MarchCursor c1 = march_cursor<U8>(plan.dist[sc], w, h, gxc);
    if constexpr (BATCH) {
        if (!CACHED) c0.base += off0;
        c1.base += off1;
    }
    int load_row = y0 - RAD;  // image row of the next load
    // raw[f][j]: loaded, not yet converted row of frame f.  The queue is QD = 2 * GROUP rows deep
    // (the LUT reads of a row are requested one row before it is converted, so its pixels must
    // have landed by then: 4.5 rows = several microseconds of flight, enough for an HBM miss
    // under load); slot j is refilled every QD rows, the loop body is unrolled QD times, so the
    // queue rotates without register moves.
    constexpr int NG = 2;  // groups in flight (1, 3 and 4 measured the same: what mattered was the counted wait)
    constexpr int QD = NG * GROUP;
    uint32_t raw0[QD][3], raw1[QD][3];
    float lin0[3] = {0.f, 0.f, 0.f}, lin1[3] = {0.f, 0.f, 0.f};  // LUT values of the next row to convert
    // A row outside the image (only in the halo of the image's first and last segments) loads the
    // nearest image row instead and is converted like any other; its values are then replaced by
    // the blur's zero padding together with the columns outside the image.  So the row body is
    // straight-line code: no per-row branch around the loads or the arithmetic.
#define MARCH_LOAD(J)                                                      \
    {                                                                      \
        const int lrow_ = min(max(load_row, 0), h - 1); /* uniform */      \
        if (CACHED) march_load<false>(raw0[J], c0, lrow_);                 \
        else march_load<U8>(raw0[J], c0, lrow_);                           \
        if (TWO) march_load<U8>(raw1[J], c1, lrow_);                       \
        ++load_row;                                                        \
    }
#define MARCH_LUT(J)                                                             \
    if (U8) {                                                                    \
        if (LUT0) march_lut(lut, raw0[J][0], c0.shift, lin0);                    \
        if (TWO) march_lut(lut, raw1[J][0], c1.shift, lin1);                     \
    }
#define MARCH_PUT(J, R)                                                                        \
    {                                                                                          \
        /* is ring row R inside the image?  (uniform, from scalars: keeps the test on the */   \
        /* scalar unit instead of a flag carried in a vector register) */                      \
        const bool rok_ = (unsigned)(y0 - RAD + (R)) < (unsigned)h;                            \
        float a_[3] = {0.f, 0.f, 0.f}, b_[3] = {0.f, 0.f, 0.f};                                \
        float m0_[3], m1_[3];                                                                  \
        if (!CACHED) {                                                                         \
            if (U8) opsin_mix(lin0[0], lin0[1], lin0[2], m0_);                                 \
            else opsin_mix(__uint_as_float(raw0[J][0]), __uint_as_float(raw0[J][1]),           \
                           __uint_as_float(raw0[J][2]), m0_);                                  \
        }                                                                                      \
        if (TWO) {                                                                             \
            if (U8) opsin_mix(lin1[0], lin1[1], lin1[2], m1_);                                 \
            else opsin_mix(__uint_as_float(raw1[J][0]), __uint_as_float(raw1[J][1]),           \
                           __uint_as_float(raw1[J][2]), m1_);                                  \
        }                                                                                      \
        if (U8) {                                                                              \
            __builtin_amdgcn_sched_barrier(0);                                                 \
            MARCH_LUT((J + 1) % QD)                                                            \
            __builtin_amdgcn_sched_barrier(0);                                                 \
        }                                                                                      \
        if (CACHED) {                                                                          \
            _Pragma("unroll") for (int c_ = 0; c_ < 3; ++c_) a_[c_] = __uint_as_float(raw0[J][c_]); \
        } else {                                                                               \
            mixed_to_xyb<false>(m0_, a_);                                                      \
        }                                                                                      \
        if (TWO) mixed_to_xyb<false>(m1_, b_);                                                 \
        if (!(all_cols && rok_)) { /* uniform; the asm keeps it a branch, not 12 selects */    \
            asm volatile("; zero padding");                                                    \
            const bool keep_ = col_ok && rok_;                                                 \
            _Pragma("unroll") for (int c_ = 0; c_ < 3; ++c_) {                                 \
                a_[c_] = keep_ ? a_[c_] : 0.0f;                                                \
                b_[c_] = keep_ ? b_[c_] : 0.0f;                                                \
            }                                                                                  \
        }                                                                                      \
        _Pragma("unroll") for (int c_ = 0; c_ < 3; ++c_)                                       \
            ring[(R) & (RING - 1)][c_][col] = f2{a_[c_], b_[c_]};                              \
    }
    // ---- halo pass (G::HALO): this wave's frame, staged columns 128 .. 135, QD rows per pass
    constexpr bool HALO = G::HALO > 0;
    static_assert(!HALO || (TWO && QD * G::HALO <= 64), "halo pass: one wave per frame, one lane per row and column");
    constexpr int HN = U8 && !CACHED ? 1 : 3;  // dwords of a halo pixel: one of a u8 frame, three of fp32 planes
    const int hf = HALO ? __builtin_amdgcn_readfirstlane(col >> 6) : 0;  // this wave and its frame
    const bool hcopy = CACHED && hf == 0;                                // cached XYB planes: no arithmetic
    const bool hu8 = U8 && !hcopy;                                       // this wave's frame goes through the LUT
    const int hrow = min((col & 63) >> 3, QD - 1), hcol = 128 + (col & 7);
    const bool hcol_ok = x0 - RAD + hcol < w;
    MarchCursor hc = hf ? c1 : c0;  // base, pitch, plane of the frame; the lane's offset is set below
    uint32_t hoff = 0;              // row `hrow` of a pass, column `hcol`: loop-invariant
    size_t hplane = 0;              // bytes between the three loads (a u8 pixel among fp32 ones: loaded three times)
    uint32_t hnext[HN] = {};        // the next pass's pixel
    if constexpr (HALO) {
        const int hgxc = min(x0 - RAD + hcol, w - 1);
        const MarchCursor at = hu8 ? march_cursor<true>(nullptr, w, h, hgxc) : march_cursor<false>(nullptr, w, h, hgxc);
        hc.off = at.off;
        hc.shift = at.shift;
        hoff = (uint32_t)hrow * (uint32_t)hc.pitch + hc.off;
        hplane = hu8 ? 0 : hc.plane;
    }
    // pixels of pass b (ring rows QD b .. QD b + QD - 1) into q
    const auto halo_load = [&](uint32_t (&q)[HN], int b) {
        const int r0 = y0 - RAD + QD * b;  // image row of the pass's first row (uniform)
        int rbase = r0;
        uint32_t off = hoff;
        if (r0 < 0 || r0 + QD > h) {  // uniform; the asm keeps it a branch
            asm volatile("; halo rows clamped into the image");
            rbase = min(max(r0, 0), h - 1);
            off = (uint32_t)(min(max(r0 + hrow, 0), h - 1) - rbase) * (uint32_t)hc.pitch;
            asm volatile("" : "+v"(off));  // a 32-bit product and a 32-bit sum, not one 64-bit multiply-add
            off += hc.off;
        }
        const uint8_t* p = hc.base + (size_t)(uint32_t)rbase * (uint32_t)hc.pitch;
        asm volatile("" : "+v"(off));  // as in march_load: the zero extension stays with the loads
        __builtin_memcpy(&q[0], p + off, 4);
        if constexpr (HN == 3) {
            __builtin_memcpy(&q[1], (p + hplane) + off, 4);
            __builtin_memcpy(&q[2], (p + 2 * hplane) + off, 4);
        }
    };
    // ... converted and stored: this frame's half of the ring elements
    const auto halo_put = [&](const uint32_t (&q)[HN], int b) {
        float v[3];
        if (hcopy) {
#pragma unroll
            for (int k = 0; k < 3; ++k) v[k] = __uint_as_float(q[k % HN]);
        } else {
            float lin[3], m[3];
            if (hu8) {
                march_lut(lut, q[0], hc.shift, lin);
            } else {
#pragma unroll
                for (int k = 0; k < 3; ++k) lin[k] = __uint_as_float(q[k % HN]);
            }
            opsin_mix(lin[0], lin[1], lin[2], m);
            mixed_to_xyb<false>(m, v);
        }
        const int r0 = y0 - RAD + QD * b;
        if (!(all_cols && r0 >= 0 && r0 + QD <= h)) {  // uniform; the asm keeps it a branch
            asm volatile("; halo zero padding");
            const bool keep = hcol_ok && (unsigned)(r0 + hrow) < (unsigned)h;
#pragma unroll
            for (int k = 0; k < 3; ++k) v[k] = keep ? v[k] : 0.0f;
        }
        float* dst = (float*)&ring[(QD * b + hrow) & (RING - 1)][0][hcol] + hf;
#pragma unroll
        for (int k = 0; k < 3; ++k) dst[k * 2 * G::MRW] = v[k];
    };
#define MARCH_HALO(G_)                                        \
    if constexpr (HALO) {                                     \
        uint32_t hcur_[HN];                                   \
        _Pragma("unroll") for (int k_ = 0; k_ < HN; ++k_) hcur_[k_] = hnext[k_]; \
        halo_load(hnext, ((G_) >> 1) + 1);                    \
        halo_put(hcur_, (G_) >> 1);                           \
    }
    // first of all loads, as in the loop a pass's load precedes the QD rows' own: the wait before its use then counts
    // the same loads behind it on both ways into the loop
    if constexpr (HALO) halo_load(hnext, 0);
#pragma unroll
    for (int j = 0; j < QD; ++j) MARCH_LOAD(j)  // rows 0 .. QD-1
    MARCH_LUT(0)
    // group g produces ring rows 3g .. 3g+2 (the blur waves consume them in their group g, one
    // barrier later) and loads rows 3g+6 .. 3g+8; ngroups + 1 barriers in all, the last group
    // only joins the barrier.  A partial last group converts up to two rows behind the segment
    // into ring slots nobody reads any more.
#define MARCH_GROUP(G, J0)                                   \
    if ((G) * GROUP < steps) {                               \
        if ((J0) == 0) MARCH_HALO(G) /* even groups */       \
        MARCH_PUT(J0 + 0, (G) * GROUP + 0)                   \
        MARCH_LOAD(J0 + 0)                                   \
        MARCH_PUT(J0 + 1, (G) * GROUP + 1)                   \
        MARCH_LOAD(J0 + 1)                                   \
        MARCH_PUT(J0 + 2, (G) * GROUP + 2)                   \
        MARCH_LOAD(J0 + 2)                                   \
    }
    static_assert(GROUP == 3, "MARCH_GROUP is written for three rows per barrier interval");
#pragma unroll 1
    for (int g = 0; g <= ngroups; g += 2) {
        MARCH_GROUP(g, 0)
        __syncthreads();
        if (g + 1 <= ngroups) {
            MARCH_GROUP(g + 1, GROUP)
            __syncthreads();
        }
    }
#undef MARCH_GROUP
#undef MARCH_HALO
#undef MARCH_LOAD
#undef MARCH_LUT
#undef MARCH_PUT
}

// Positive-XYB planes of one frame at one scale (run once per search for the reference, whose
// pixels are the same on every pass: tq.zig:37 passes the same e.rgb, main.zig:86).
__global__ __launch_bounds__(256) void k_ref_xyb(const void* __restrict__ in, bool u8, int w, int h,
                                                 float* __restrict__ out) {
    const size_t n = (size_t)w * h;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float r, g, b;
    if (u8) {
        const uint8_t* p = (const uint8_t*)in + i * 3;
        r = c_k.lut[p[0]];
        g = c_k.lut[p[1]];
        b = c_k.lut[p[2]];
    } else {
        const float* p = (const float*)in + i;
        r = p[0];
        g = p[n];
        b = p[2 * n];
    }
    float X, Y, B;
    linear_to_xyb(r, g, b, X, Y, B);
    out[i] = X;
    out[n + i] = Y;
    out[2 * n + i] = B;
}

// One (ref, dist) pair as it sits in the ring, fetched with one ds_read_b64 and split into its
// two 32-bit halves (sub-registers: no instruction).  Kept as a 64-bit integer rather than a
// float vector so that the compiler does not pair up the x / y arithmetic into v_pk_*_f32,
// which ties values to even-aligned register pairs the 80-VGPR budget has no room for.
struct MarchPair {
    unsigned long long u;
    __device__ __forceinline__ float x() const { return __uint_as_float((uint32_t)u); }
    __device__ __forceinline__ float y() const { return __uint_as_float((uint32_t)(u >> 32)); }
};
// volatile: one ds_read_b64 per tap.  The compiler would otherwise fuse neighbouring taps into
// ds_read2_b64, which the LDS serves at half the rate of two ds_read_b64 (measured: +3 %).
typedef __attribute__((address_space(3))) volatile unsigned long long lds_vu64;

template <typename G>
__device__ __forceinline__ const lds_vu64* march_row(const lds_vu64* rp, int t) {
    return rp + (t & (RING - 1)) * G::RING_ROW;
}

// Horizontal pass of ring row t into window slot P: the lane's 9-wide window of (x, y) pairs
// (staged columns o .. o+8, centre o+4), nine ds_read_b64.
// plain planes: pair sums of the taps; product planes: the products are formed inside the
// pair sums as fma(a-, b-, a+ * b+) -- one rounding and one operation fewer than two
// products and an add (arithmetic contract, mirrored by the CPU checker)
template <int P, int MODE, typename G>
__device__ __forceinline__ void march_h(const lds_vu64* rp, float (&win)[5][9], int t, float w0,
                                        float w1, float w2, float w3, float w4) {
    const lds_vu64* row = march_row<G>(rp, t);
    MarchPair v[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) v[q].u = row[q];
#define H9(f) \
    fir9(v[4].f(), v[3].f() + v[5].f(), v[2].f() + v[6].f(), v[1].f() + v[7].f(), v[0].f() + v[8].f(), \
         w0, w1, w2, w3, w4)
#define H9P(a, b)                                                                                      \
    fir9(v[4].a() * v[4].b(), fmaf(v[3].a(), v[3].b(), v[5].a() * v[5].b()),                           \
         fmaf(v[2].a(), v[2].b(), v[6].a() * v[6].b()), fmaf(v[1].a(), v[1].b(), v[7].a() * v[7].b()), \
         fmaf(v[0].a(), v[0].b(), v[8].a() * v[8].b()), w0, w1, w2, w3, w4)
    win[0][P] = H9(x);
    if (MODE != MARCH_REFBLUR) win[2][P] = H9P(x, x);
    if (MODE != MARCH_EMIT) {
        win[1][P] = H9(y);
        win[3][P] = H9P(y, y);
        win[4][P] = H9P(x, y);
    }
#undef H9
#undef H9P
}

// Second half of step t: vertical pass and maps of output row t - 4 (window slot of row t - j
// is (P - j) mod 9).  `edge`: the strip reaches past the image's right edge, so lanes whose
// column is outside (`!ok`) must not contribute (uniform; interior strips skip the selects).
template <int P, int MODE, typename G>
__device__ __forceinline__ void march_v(const lds_vu64* rp, float (&win)[5][9], float (&acc)[6], int t,
                                        bool ok, bool edge, float w0, float w1, float w2, float w3,
                                        float w4, MarchRefBlur& rb, const float (&mc)[6]) {
    float c_s11 = 0.f;
    if (MODE == MARCH_REFBLUR) {
        // consume the value loaded RB_AHEAD steps ago, then load the row RB_AHEAD steps ahead
        c_s11 = rb.ps11[P];
        if (t >= 8 - RB_AHEAD && rb.rows_left > 0) {  // uniform: that output row exists
            rb.ps11[(P + RB_AHEAD) % 9] = ok ? *rb.s11 : 0.0f;
            rb.s11 += rb.pitch;
            --rb.rows_left;
        }
    }
    if (t < 8) return;  // window not full yet (uniform across the workgroup)
    float v[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        if (MODE == MARCH_REFBLUR && k == 2) continue;
        if (MODE == MARCH_EMIT && k != 2) continue;
        const float* q = win[k];
        v[k] = fir9(q[(P + 5) % 9], q[(P + 4) % 9] + q[(P + 6) % 9],
                    q[(P + 3) % 9] + q[(P + 7) % 9], q[(P + 2) % 9] + q[(P + 8) % 9],
                    q[(P + 1) % 9] + q[P], w0, w1, w2, w3, w4);
    }
    if (MODE == MARCH_EMIT) {  // the reference's blur(ref*ref) plane, one row per step
        if (ok && rb.active) *rb.s11 = v[2];
        rb.s11 += rb.pitch;
        return;
    }
    MarchPair ctr;
    ctr.u = march_row<G>(rp, t - 4)[RAD];  // centre pixel of the output row
    const float r1 = ctr.x(), r2 = ctr.y();
    const float mu1 = v[0], mu2 = v[1];
    const float s11 = MODE == MARCH_REFBLUR ? c_s11 : v[2], s22 = v[3], s12 = v[4];
    float d = ssim_term(mu1, mu2, s11, s22, s12);
    float e = edge_quotient<false>(mu1, mu2, r1, r2);
    if (edge) {  // uniform; the asm keeps it a branch
        asm volatile("; right image edge");
        d = ok ? d : 0.0f;  // column inside the image?
        e = ok ? e : 0.0f;
    }
    if (MODE == MARCH_MAP) {  // this channel's density, one row per step
        float tm[6];
        six_terms(d, e, [&](int k, float term) { tm[k] = term; });
        if (ok && rb.active) *rb.s11 = map_density(tm, mc);
        rb.s11 += rb.pitch;
        return;
    }
    six_terms(d, e, [&](int k, float term) { acc[k] += term; });
}

// XCD-aware tile order.  Workgroups are dealt to the eight XCDs round-robin by blockIdx (each XCD has its own
// 4 MiB L2), while neighbouring strips of one segment share their 8 halo columns and -- strips being 120 columns,
// not a multiple of a 128-byte line -- the cache lines their edges straddle.  With tile = blockIdx those neighbours
// sit on DIFFERENT XCDs and every XCD fetches its own copy.  So each XCD takes a contiguous run of tiles instead
// (profiles/r04_xcd_order_ab.log: 21 % fewer fetched bytes): among the workgroups [first, end) of a scale, the ones
// with blockIdx % 8 == x take the x-th run, in blockIdx order.  A bijection on [0, end - first); which workgroup
// computes a tile does not enter the tile's arithmetic, and the partial sums are stored under the TILE index: scores
// keep their bits.
__device__ __forceinline__ int march_tile_of_block(int b, int first, int end) {
    // cnt(n, r) = how many k in [0, n) have k % 8 == r
    const int x = b & 7;
    int before = 0;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int n_r = (end + 7 - r) / 8 - (first + 7 - r) / 8;  // workgroups of this scale on XCD phase r
        before += r < x ? n_r : 0;
    }
    return before + (b >> 3) - ((first + 7 - x) >> 3);  // + its rank among those of phase x
}

// Where a workgroup of a BATCH launch works (march_batch_body): its scale and tile come from the batch grid instead
// of blockIdx.x, and its item's frames and partial sums lie at uniform offsets from the plan's (item 0's) pointers.
struct MarchItem {
    int sc, tile;
    size_t off_ref, off_dist;  // bytes: the item's frame at scale `sc` from plan.ref[sc] / plan.dist[sc]
    size_t off_part;           // doubles: the item's partial sums from plan.part[sc]
};

// LIN0: scale 0 is fp32 linear planes [3][h][w] like the smaller scales (the 16-bit front end's), not 8-bit frames.
// BATCH: `it` says where the workgroup works; otherwise blockIdx.x does and `it` is not read.
template <int MODE, typename G, bool LIN0 = false, bool BATCH = false>
__device__ __forceinline__ void march_body(const MarchPlan& plan, const MapCoef* coef = nullptr,
                                           const MarchItem* it = nullptr) {
    // [row slot][channel][column] of (ref, dist) pairs
    __shared__ __attribute__((aligned(16))) f2 s_ring[RING][3][G::MRW];
    __shared__ float s_lut[256];
    __shared__ double s_part[6][6];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

    // which scale / strip / segment is this workgroup?
    int sc = 0, first = 0;
#pragma unroll
    for (int s = 0; s < kNumScales - 1; ++s)
        if (!BATCH && s + 1 < plan.nscales && (int)blockIdx.x >= plan.blk_end[s]) {
            sc = s + 1;
            first = plan.blk_end[s];
        }
    if constexpr (BATCH) sc = it->sc;
    const int blk = BATCH ? it->tile : march_tile_of_block((int)blockIdx.x, first, plan.blk_end[sc]);
    const int w = plan.w[sc], h = plan.h[sc], seg_rows = plan.seg[sc];
    const int nstrips = plan.nstrips[sc];
    const int by = blk / nstrips, bx = blk - by * nstrips;
    const bool u8 = !LIN0 && sc == 0;
    const int x0 = bx * G::MW;
    const int y0 = by * seg_rows;
    const int rows_out = min(seg_rows, h - y0);
    const int steps = rows_out + 2 * RAD;  // input rows y0-4 .. y0+rows_out+3
    if (u8) {
        for (int i = tid; i < 256; i += MARCH_THREADS) s_lut[i] = c_k.lut[i];
    }
    __syncthreads();

    const float w0 = c_k.taps[0], w1 = c_k.taps[1], w2 = c_k.taps[2], w3 = c_k.taps[3],
                w4 = c_k.taps[4];
    const bool is_conv = wave < CONV_WAVES;
    // blur state (fp32 sums: at most seg <= 160 terms per lane before the fp64 reduce)
    float acc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const int hw = wave - CONV_WAVES;
    const int ch = hw >> 1;
    const bool hv_active = G::MHALF == 64 || lane < G::MHALF;  // MarchWide: every lane owns a column
    const int o = (hw & 1) * G::MHALF + (hv_active ? lane : 0);
    const bool ok = x0 + o < w;
    MarchRefBlur rb;
    rb.pitch = w;
    rb.rows_left = rows_out;
    rb.active = hv_active;
#pragma unroll
    for (int k = 0; k < 9; ++k) rb.ps11[k] = 0.f;
    // MARCH_MAP: coefficients of this channel's six terms (d, d^4, art, art^4, det, det^4)
    float mc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (MODE == MARCH_MAP) {
#pragma unroll
        for (int k = 0; k < 6; ++k) mc[k] = coef->c[sc][term_stat(max(ch, 0), k)];
    }
    {
        // this lane's pixel in output row y0 of its channel's planes (column clamped: lanes
        // outside the image never dereference it)
        const size_t at = ((size_t)max(ch, 0) * h + y0) * (size_t)w + (size_t)min(x0 + o, w - 1);
        rb.s11 = MODE == MARCH_PAIR ? nullptr : plan.ref_s11[sc] + at;
    }

    // Input row j (= image row y0-4+j) lives in ring slot j & (RING-1).  While the blur waves
    // consume rows 3I..3I+2 the converters fill rows 3I+AHEAD..3I+AHEAD+2.  The two roles run
    // separate loops with the same number of barriers (one per group of GROUP rows), so each
    // gets its own register allocation instead of carrying the other role's state.
    const int ngroups = (steps + GROUP - 1) / GROUP;
    if (is_conv) {
        // No issue-priority bump for the converter waves: s_setprio(1) once took 7 % off, but with the
        // 64-bit address arithmetic gone from their rows it makes k_march 4 % slower
        // (profiles/r07_march_ab.txt).  Waves 0-1 of the three workgroups of a CU already sit 2/2/1/1
        // on its SIMDs (profiles/r07_placement.txt), so which wave converts is left as it is.
        const int col = (wave << 6) + lane;  // staged column; this lane converts both frames
        if constexpr (BATCH) {
            if (u8) march_convert_rows<G, true, MODE, LIN0, true>(s_ring, s_lut, plan, sc, w, h, x0, y0, steps, ngroups, col, it->off_ref, it->off_dist);
            else march_convert_rows<G, false, MODE, LIN0, true>(s_ring, s_lut, plan, sc, w, h, x0, y0, steps, ngroups, col, it->off_ref, it->off_dist);
        } else {
            if (u8) march_convert_rows<G, true, MODE, LIN0>(s_ring, s_lut, plan, sc, w, h, x0, y0, steps, ngroups, col);
            else march_convert_rows<G, false, MODE, LIN0>(s_ring, s_lut, plan, sc, w, h, x0, y0, steps, ngroups, col);
        }
    } else {
        float win[5][9];
        const lds_vu64* rp = (const lds_vu64*)&s_ring[0][ch][o];  // staged columns o .. o+8, centre o+4
        const bool edge = x0 + G::MW > w;  // uniform: some lanes of this strip are outside the image
        __syncthreads();
        // step t: horizontal pass of ring row t; [barrier after the group's last row]; vertical
        // pass + maps of output row t - 4
#define MARCH_STEP(P)                                                                          \
    {                                                                                          \
        const int t = t0 + P;                                                                  \
        if (t < steps) march_h<P, MODE, G>(rp, win, t, w0, w1, w2, w3, w4);                       \
        if ((P % GROUP) == GROUP - 1 && t - (GROUP - 1) < steps) __syncthreads();              \
        if (t < steps) march_v<P, MODE, G>(rp, win, acc, t, ok, edge, w0, w1, w2, w3, w4, rb, mc);    \
    }
#pragma unroll 1
        for (int t0 = 0; t0 < steps; t0 += 9) {
            MARCH_STEP(0)
            MARCH_STEP(1)
            MARCH_STEP(2)
            MARCH_STEP(3)
            MARCH_STEP(4)
            MARCH_STEP(5)
            MARCH_STEP(6)
            MARCH_STEP(7)
            MARCH_STEP(8)
        }
#undef MARCH_STEP
    }

    if (MODE == MARCH_EMIT || MODE == MARCH_MAP) return;  // planes written, nothing to reduce
    // the two half-strip waves of a channel each publish their sums; combined in fixed order
    if (!is_conv) {
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const double v = wave_sum(hv_active ? (double)acc[k] : 0.0);
            if (lane == 0) s_part[hw][k] = v;
        }
    }
    __syncthreads();
    if (tid < kStats) {
        // tid = stat index: 0..5 ssim (c*2+n), 6..17 edge (c*4+k)
        const int c = tid < 6 ? tid >> 1 : (tid - 6) >> 2;
        const int k = tid < 6 ? (tid & 1) : 2 + ((tid - 6) & 3);
        if constexpr (BATCH)
            plan.part[sc][it->off_part + (size_t)tid * plan.nblocks[sc] + blk] = s_part[2 * c][k] + s_part[2 * c + 1][k];
        else
            plan.part[sc][(size_t)tid * plan.nblocks[sc] + blk] = s_part[2 * c][k] + s_part[2 * c + 1][k];
    }
}

// ---- batch form: N pairs of one size in ONE marching launch (ssimu2_score_batch_*) ----------------
// `item` is the MarchPlan of item 0 (geometry, and the pointers of its frames, pyramids and partial sums); item i's
// buffers lie i * stride further on.  The cached reference planes (ref_xyb, ref_s11) are one set for the whole batch.
struct MarchBatchPlan {
    MarchPlan item;
    int n_items;
    int blk_end[kNumScales];          // exclusive end of each scale's range in the batch grid: n_items * item.blk_end[s]
    size_t ref_stride0, dist_stride0;  // bytes between items' 8-bit frames (a reference shared by all items: 0)
    size_t ref_stride, dist_stride;    // bytes between items' linear pyramids (scales >= 1)
    size_t part_stride;                // doubles between items' partial sums
};

// Workgroup -> (scale, item, tile).  The grid is ordered largest scale first ACROSS all items, so the short workgroups
// of the small scales fill the tail of the whole batch, as they fill the tail of scale 0 in a single score.  Within
// a scale, march_tile_of_block deals each XCD (own L2) a contiguous run of the scale's n_items * nblocks virtual
// indices, and
//   ITEMS_FASTEST = false (pairs): index = item * nblocks + tile -- an XCD's run is neighbouring tiles of one item,
//       which share their halo columns and the cache lines their strip edges straddle, as in a single score;
//   ITEMS_FASTEST = true (cached reference): index = tile * n_items + item -- an XCD's run is the SAME tile of
//       consecutive items, which all read that tile of the reference's XYB and blur planes: fetched from HBM once
//       per XCD and batch instead of once per item (the reference is 24 of the 27 bytes per pixel such a pass reads).
// Which workgroup computes a tile does not enter its arithmetic and sums are stored under (item, tile): bits unmoved.
template <int MODE, bool ITEMS_FASTEST>
__device__ __forceinline__ void march_batch_body(const MarchBatchPlan& bp) {
    const int b = (int)blockIdx.x;
    int sc = 0, first = 0;
#pragma unroll
    for (int s = 0; s < kNumScales - 1; ++s)
        if (s + 1 < bp.item.nscales && b >= bp.blk_end[s]) {
            sc = s + 1;
            first = bp.blk_end[s];
        }
    const int v = march_tile_of_block(b, first, bp.blk_end[sc]);
    const int nb = bp.item.nblocks[sc];
    int item, tile;
    if (ITEMS_FASTEST) {
        tile = v / bp.n_items;
        item = v - tile * bp.n_items;
    } else {
        item = v / nb;
        tile = v - item * nb;
    }
    // blockIdx arithmetic over kernel arguments: uniform, but say so (the converters' loads take their base from SGPRs)
    item = __builtin_amdgcn_readfirstlane(item);
    tile = __builtin_amdgcn_readfirstlane(tile);
    MarchItem it;
    it.sc = sc;
    it.tile = tile;
    it.off_ref = (size_t)item * (sc == 0 ? bp.ref_stride0 : bp.ref_stride);
    it.off_dist = (size_t)item * (sc == 0 ? bp.dist_stride0 : bp.dist_stride);
    it.off_part = (size_t)item * bp.part_stride;
    march_body<MODE, MarchWide, false, true>(bp.item, nullptr, &it);
}

// launch bound: 3 workgroups of 8 waves per CU = 6 waves per SIMD (<= 80 VGPRs)
__global__ __launch_bounds__(MARCH_THREADS, 6) void k_march(MarchPlan plan) {
    march_body<MARCH_PAIR, MarchWide>(plan);
}

// the per-pass kernel of a search: reference XYB and blur(ref*ref) planes cached
__global__ __launch_bounds__(MARCH_THREADS, 6) void k_march_refblur(MarchPlan plan) {
    march_body<MARCH_REFBLUR, MarchWide>(plan);
}

// once per search: blur(ref*ref) of every scale into plan.ref_s11
__global__ __launch_bounds__(MARCH_THREADS, 6) void k_ref_blur(MarchPlan plan) {
    march_body<MARCH_EMIT, MarchNarrow>(plan);
}

// The same two kernels for 16-bit frames: scale 0 comes from the linear planes k_pyramid_bands16 wrote
// (ssimu2_score_rgb16, ssimu2_score_against_reference_rgb16 / _strided16).
__global__ __launch_bounds__(MARCH_THREADS, 6) void k_march_lin(MarchPlan plan) {
    march_body<MARCH_PAIR, MarchWide, true>(plan);
}

__global__ __launch_bounds__(MARCH_THREADS, 6) void k_march_refblur_lin(MarchPlan plan) {
    march_body<MARCH_REFBLUR, MarchWide, true>(plan);
}

// The batch forms of k_march and k_march_refblur: entries of their own (own register allocation; the single-score
// kernels above are not touched by them).
__global__ __launch_bounds__(MARCH_THREADS, 6) void k_march_batch(MarchBatchPlan bp) {
    march_batch_body<MARCH_PAIR, false>(bp);
}

__global__ __launch_bounds__(MARCH_THREADS, 6) void k_march_refblur_batch(MarchBatchPlan bp) {
    march_batch_body<MARCH_REFBLUR, true>(bp);
}

// error-map pass (ssimu2_error_map_*): per-pixel densities of every scale into plan.ref_s11.  Its own entry and
// register allocation; the score kernels above are not touched by it.
__global__ __launch_bounds__(MARCH_THREADS, 6) void k_march_map(MarchPlan plan, MapCoef coef) {
    march_body<MARCH_MAP, MarchNarrow>(plan, &coef);
}

// The same pass after a 16-bit score (include/ssimu2_hip_map.h): scale 0 comes from the linear planes of the two
// frames, as in k_march_lin.  An entry of its own; k_march_map's code is what it was.
__global__ __launch_bounds__(MARCH_THREADS, 6) void k_march_map_lin(MarchPlan plan, MapCoef coef) {
    march_body<MARCH_MAP, MarchNarrow, true>(plan, &coef);
}

// The full-resolution map: map(x, y) = sum over scales s (ascending) of
// (dens_s[X] + dens_s[Y]) + dens_s[B] at (x >> s, y >> s).  One thread per pixel, fixed order.
struct MapComposeArgs {
    const float* dens[kNumScales];  // [3][h_s][w_s] per scale
    int w[kNumScales], h[kNumScales];
    int nscales;
    float* out;                     // [h_0][w_0]
};
__global__ __launch_bounds__(256) void k_map_compose(MapComposeArgs a) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)a.w[0] * a.h[0]) return;
    const int y = (int)(i / (unsigned)a.w[0]), x = (int)(i - (size_t)y * a.w[0]);
    float v = 0.0f;
    for (int s = 0; s < a.nscales; ++s) {
        const size_t n = (size_t)a.w[s] * a.h[s];
        const float* p = a.dens[s] + (size_t)(y >> s) * a.w[s] + (x >> s);
        v += (p[0] + p[n]) + p[2 * n];
    }
    a.out[i] = v;
}

// ---- final reduction ------------------------------------------------------------------------------
struct FinalizeArgs {
    const double* part[kNumScales];
    int nblocks[kNumScales];
    double inv_pixels[kNumScales];
    int nscales;
};

// result layout: [0..107] averages [scale][18], [108] score, [109] nscales.  `result` is page-locked host memory: the
// kernel writes the 880 bytes over the bus itself (round 5: no device-side copy of them and no D2H copy command per
// score; -1.7 us per pair score, bits equal).
// 8 lanes per (scale, stat) item stride over the workgroup partials; lane-local sums, then a
// fixed-order 8-lane shuffle tree: deterministic, and 128 items run in parallel instead of 16.
// A launch of its own by measurement (round 5, profiles/r05_finalize_ab.log): folded into the last workgroup of the
// marching launch (an atomic done-counter behind a device-scope release) it made k_march 20 us SLOWER at 4K -- every
// one of its ~1000 workgroups pays an L2 write-back for the release -- and the recursive pass 2.5 us slower.
// One body for both entries.  BATCH: one workgroup per item of a batch, whose partial sums lie `part_stride` doubles
// per item behind fa.part[scale]; an item's result depends on its own sums alone.
template <bool BATCH>
__device__ __forceinline__ void finalize_body(const FinalizeArgs& fa, size_t part_stride, double* __restrict__ result) {
    __shared__ double s_avg[kNumScales * kStats];
    const int item = threadIdx.x >> 3, sub = threadIdx.x & 7;
    double v = 0.0;
    const int scale = item / kStats, stat = item - scale * kStats;
    const bool live = item < kNumScales * kStats && scale < fa.nscales;
    if (live) {
        // each lane sums runs of 8 consecutive partials: the 8 loads of a run are independent,
        // so the loop is 8x shorter than one dependent load + add per partial
        const double* p = fa.part[scale] + (size_t)stat * fa.nblocks[scale];
        if constexpr (BATCH) p += (size_t)blockIdx.x * part_stride;
        const int nb = fa.nblocks[scale];
        for (int b = sub * 8; b < nb; b += 64) {
            double t[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) t[k] = b + k < nb ? p[b + k] : 0.0;
            v += ((t[0] + t[1]) + (t[2] + t[3])) + ((t[4] + t[5]) + (t[6] + t[7]));
        }
    }
    v += __shfl_down(v, 4, 8);
    v += __shfl_down(v, 2, 8);
    v += __shfl_down(v, 1, 8);
    if (sub == 0 && item < kNumScales * kStats) {
        if (live) {
            v *= fa.inv_pixels[scale];
            if (stat & 1) v = sqrt(sqrt(v));  // odd stats are L4 norms
        }
        s_avg[item] = v;
    }
    __syncthreads();
    // published Score(): weights are consumed with a running index over (channel, scale present,
    // norm, {ssim, artifact, detail}); term j of that walk is evaluated by thread j and the
    // terms are summed with a fixed shuffle tree (two waves), then by thread 0.
    __shared__ double s_red[2];
    if (threadIdx.x < 128) {
        const int j = threadIdx.x;
        const int nterms = 3 * fa.nscales * 2 * 3;
        double term = 0.0;
        if (j < nterms) {
            const int k = j % 3, n = (j / 3) & 1, cs = j / 6;
            const int sc = cs % fa.nscales, c = cs / fa.nscales;
            const double* a = s_avg + sc * kStats;
            const double val = k == 0 ? a[c * 2 + n] : a[6 + c * 4 + n + (k == 2 ? 2 : 0)];
            term = c_k.weights[j] * fabs(val);
        }
        term = wave_sum(term);
        if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = term;
    }
    __syncthreads();
    // the averages leave as two full-wave stores of consecutive doubles (they cross PCIe: not 108 scattered ones)
    if (threadIdx.x < kNumScales * kStats) result[threadIdx.x] = s_avg[threadIdx.x];
    if (threadIdx.x == 0) {
        double ssim = s_red[0] + s_red[1];
        ssim = ssim * 0.9562382616834844;
        ssim = 2.326765642916932 * ssim - 0.020884521182843837 * ssim * ssim +
               6.248496625763138e-05 * ssim * ssim * ssim;
        if (ssim > 0.0) ssim = 100.0 - 10.0 * pow(ssim, 0.6276336467831387);
        else ssim = 100.0;
        result[108] = ssim;
        result[109] = (double)fa.nscales;
    }
}

__global__ __launch_bounds__(1024) void k_finalize(FinalizeArgs fa, double* __restrict__ result) {
    finalize_body<false>(fa, 0, result);
}

// Item i's 110 doubles go to results + 110 i of the context's page-locked batch mirror.
__global__ __launch_bounds__(1024) void k_finalize_batch(FinalizeArgs fa, size_t part_stride, double* __restrict__ results) {
    finalize_body<true>(fa, part_stride, results + (size_t)blockIdx.x * (kNumScales * kStats + 2));
}

// ---------------------------------------------------------------------------------------------
// Decoded-frame hand-off (io.zig:654-663): libavif's RGB / RGBA rows `pitch` bytes apart ->
// tight RGB8.  kFast: four RGBA pixels per lane, four dword loads and three dword stores
// (needs w % 4 == 0, pitch % 4 == 0 and dword-aligned buffers); otherwise one pixel per lane
// with byte accesses.  Pure byte movement, HBM-bound: (ch + 3) bytes per pixel.
// ---------------------------------------------------------------------------------------------
template <bool kFast>
__global__ __launch_bounds__(256) void k_unpack_rgb(const uint8_t* __restrict__ src, uint32_t pitch,
                                                    uint32_t ch, uint32_t w, uint32_t h,
                                                    uint8_t* __restrict__ dst) {
    const uint32_t y = blockIdx.y;
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (y >= h) return;
    if (kFast) {
        if (i * 4u >= w) return;
        const uint32_t* s = reinterpret_cast<const uint32_t*>(src + (size_t)y * pitch) + i * 4u;
        const uint32_t p0 = s[0], p1 = s[1], p2 = s[2], p3 = s[3];  // LE: R | G<<8 | B<<16 | A<<24
        uint32_t* d = reinterpret_cast<uint32_t*>(dst + ((size_t)y * w + i * 4u) * 3u);
        d[0] = (p0 & 0x00FFFFFFu) | (p1 << 24);
        d[1] = ((p1 >> 8) & 0x0000FFFFu) | (p2 << 16);
        d[2] = ((p2 >> 16) & 0x000000FFu) | (p3 << 8);
    } else {
        if (i >= w) return;
        const uint8_t* s = src + (size_t)y * pitch + (size_t)i * ch;
        uint8_t* d = dst + ((size_t)y * w + i) * 3u;
        d[0] = s[0];
        d[1] = s[1];
        d[2] = s[2];
    }
}

}  // namespace ssimu2
