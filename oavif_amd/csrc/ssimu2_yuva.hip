// YUV input with an alpha plane of the MI355X SSIMULACRA2 scorer: the entry points of include/ssimu2_hip_yuva.h
// (DESIGN.md section 17).
//
// A translation unit of its own over ssimu2_host.h, like the RGBA, YUV, map and chroma units: one kernel template, one
// Feed constructor, one check and six functions.  Its object is linked with the chroma library's objects into
// liboavif_hip_yuva.so; the other six libraries contain none of this, and their exports are what they were.
//
// A frame is chroma_feed's Feed (the one yuv_constants, the chroma planes at their own size) with one more plane behind
// the others, the alpha plane if there is one, whose unpacking is k_yuva_to_codes below: the colour codes of
// ssimu2_yuv_pixel.h composited over the background into the 65,026 codes the RGBA front end reads through its table T
// (Feed::top = 65025, the context's alpha_tab).  The three shapes of a call and the two of a map are the scorer's.
#include "../../include/ssimu2_hip_yuva.h"
#include "ssimu2_alpha_pixel.h"
#include "ssimu2_host.h"
#include "ssimu2_yuv_pixel.h"

#include <stdlib.h>
#include <string.h>

using namespace ssimu2h;

namespace ssimu2 {

// ---------------------------------------------------------------------------------------------
// Planes of S-byte samples -- Y and A of w x h, U and V as SUB says -- rows `pitch` bytes apart at any alignment
// (2-byte for S = 2) -> tight u16 composite codes over the background k.b.
//   SUB = 0: U and V of w x h (4:4:4);  SUB = 2: none (4:0:0, R = G = B = Y as in k_yuv_to_codes<S, true>);
//   SUB = 1: U and V of cw x ch, upsampled as include/ssimu2_hip_chroma.h defines it (V: 4:2:0, else 4:2:2;
//            BILINEAR or nearest), exactly as in k_yuv_chroma_to_codes.
// The lane shape is k_yuv_chroma_to_codes': four luma columns x0..x0+3 of the luma rows that share chroma row r (two
// for V, else one); the chroma samples those pixels need normalised once per plane (yuv_unorm) -- for SUB = 1 columns
// x0/2 - 1 .. x0/2 + 2 (bilinear) or x0/2, x0/2 + 1 (nearest) of rows r - 1 .. r + 1 (bilinear and V) or r, for SUB = 0
// the four pixels' own columns of row r --, every index clamped into the plane before its load, a lane none of whose
// indices is clamped taking a row's samples in one load (samples_at).  Luma and alpha go alike: per row one unaligned
// dword load (S = 1) or two (S = 2); a null alpha plane (uniform) costs no load, a = ma.  Six dword stores per row; the
// last w % 4 pixels of a row go sample by sample.  Chroma rows beyond gridDim.y are taken in further rounds.  No LDS,
// no scratch (every array index is a constant once unrolled).
// ---------------------------------------------------------------------------------------------
template <int S, int SUB, bool V, bool BILINEAR, int DIV>
__global__ __launch_bounds__(256) void k_yuva_to_codes(const uint8_t* __restrict__ py, const uint8_t* __restrict__ pu,
                                                       const uint8_t* __restrict__ pv, const uint8_t* __restrict__ pa,
                                                       uint32_t pitch_y, uint32_t pitch_u, uint32_t pitch_v, uint32_t pitch_a,
                                                       uint32_t w, uint32_t h, YuvK k, YuvaK ak, uint16_t* __restrict__ dst) {
    static_assert(SUB == 1 || (!V && !BILINEAR), "only subsampled chroma is upsampled");
    constexpr bool HALF = SUB == 1;                      // chroma columns are luma columns / 2
    constexpr int NR = (BILINEAR && V) ? 3 : 1;          // chroma rows a lane holds: r - 1, r, r + 1, or r alone
    constexpr int NC = SUB == 2 ? 1 : (HALF && !BILINEAR) ? 2 : 4;  // chroma columns it holds
    constexpr int QC = NR == 3 ? 1 : 0;                  // where row r is among them
    constexpr int LC = BILINEAR ? 1 : 0;                 // where column c0 is
    const uint32_t x0 = (blockIdx.x * 256u + threadIdx.x) * 4u;
    if (x0 >= w) return;
    const uint32_t cw = HALF ? (w + 1u) / 2u : w, ch = V ? (h + 1u) / 2u : h;
    const uint32_t c0 = HALF ? x0 >> 1 : x0;
    uint32_t col[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const uint32_t at = c0 + (uint32_t)c;  // LC columns to the right of the one meant
        col[c] = min(at >= (uint32_t)LC ? at - (uint32_t)LC : 0u, cw - 1u);
    }
    // all NC columns inside the plane (no index was clamped): they are adjacent, one load per row takes them
    const bool inner = c0 >= (uint32_t)LC && c0 + (uint32_t)(NC - 1 - LC) < cw;
    for (uint32_t r = blockIdx.y; r < ch; r += gridDim.y) {
        float cb[NR][NC], cr[NR][NC];
        if constexpr (SUB != 2) {
#pragma unroll
            for (int q = 0; q < NR; ++q) {
                const uint32_t row = NR == 3 ? (q == 0 ? (r ? r - 1u : 0u) : q == 1 ? r : min(r + 1u, ch - 1u)) : r;
                const uint8_t* const ru = pu + (size_t)row * pitch_u;
                const uint8_t* const rv = pv + (size_t)row * pitch_v;
                uint32_t su[NC], sv[NC];
                if (inner) {
                    samples_at<S, NC>(ru + (size_t)col[0] * S, su);
                    samples_at<S, NC>(rv + (size_t)col[0] * S, sv);
                } else {
#pragma unroll
                    for (int c = 0; c < NC; ++c) su[c] = sample_at<S>(ru, col[c]), sv[c] = sample_at<S>(rv, col[c]);
                }
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    cb[q][c] = yuv_unorm(su[c], k.max_code, k.bias_uv, k.range_uv);
                    cr[q][c] = yuv_unorm(sv[c], k.max_code, k.bias_uv, k.range_uv);
                }
            }
        }
#pragma unroll
        for (int jj = 0; jj < (V ? 2 : 1); ++jj) {
            const uint32_t j = V ? 2u * r + (uint32_t)jj : r;
            if (j >= h) continue;  // the last chroma row of an odd height has one luma row
            const int qn = NR == 3 ? 2 * jj : 0;  // the neighbour row: above an even luma row, below an odd one
            const uint8_t* const sy = py + (size_t)j * pitch_y + (size_t)x0 * S;
            const uint8_t* const sa = pa ? pa + (size_t)j * pitch_a + (size_t)x0 * S : nullptr;
            uint16_t* const d = dst + ((size_t)j * w + x0) * 3u;
            // pixel i of the lane's four, of luma sample y and alpha sample a -> its three composite codes
            auto pixel = [&](int i, uint32_t y, uint32_t a, uint32_t* code) {
                const float Y = yuv_unorm(y, k.max_code, k.bias_y, k.range_y);
                if (SUB == 2) {
                    code[0] = code[1] = code[2] = yuv_code(Y, k.top);
                } else {
                    const int lc = HALF ? LC + (i >> 1) : i, ln = BILINEAR ? ((i & 1) ? lc + 1 : lc - 1) : lc;
                    float Cb = cb[QC][lc], Cr = cr[QC][lc];
                    if (BILINEAR) {
                        Cb = chroma_blend(cb[QC][lc], cb[QC][ln], cb[qn][lc], cb[qn][ln]);
                        Cr = chroma_blend(cr[QC][lc], cr[QC][ln], cr[qn][lc], cr[qn][ln]);
                    }
                    yuv_codes(Y, Cb, Cr, k, code);
                }
                a = min(a, ak.ma);
#pragma unroll
                for (int c = 0; c < 3; ++c) code[c] = yuva_code<DIV>(a, code[c], ak.b[c], ak);
            };
            if (x0 + 4u <= w) {
                uint32_t smp[4], alpha[4] = {ak.ma, ak.ma, ak.ma, ak.ma};
                samples_at<S, 4>(sy, smp);
                if (sa) samples_at<S, 4>(sa, alpha);
                uint32_t n[12];
#pragma unroll
                for (int i = 0; i < 4; ++i) pixel(i, smp[i], alpha[i], n + 3 * i);
#pragma unroll
                for (int i = 0; i < 6; ++i) {
                    const uint32_t pair = n[2 * i] | (n[2 * i + 1] << 16);
                    __builtin_memcpy((uint8_t*)d + 4 * i, &pair, 4);
                }
            } else {
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    if (x0 + (uint32_t)i < w) {
                        uint32_t n[3];
                        pixel(i, sample_at<S>(sy, (uint32_t)i), sa ? sample_at<S>(sa, (uint32_t)i) : ak.ma, n);
#pragma unroll
                        for (int c = 0; c < 3; ++c) d[3 * i + c] = (uint16_t)n[c];
                    }
                }
            }
        }
    }
}

}  // namespace ssimu2

using namespace ssimu2;

// Argument checks of one frame for a w x h call (the ctx is not null): check_chroma's of the colour planes, then the
// alpha plane's.
int ssimu2h::check_yuva(ssimu2_ctx* c, const ssimu2_yuva_frame* f, uint32_t w, uint32_t rgb_depth, uint32_t upsampling) {
    const int rc = check_chroma(c, f ? &f->yuv : nullptr, w, rgb_depth, upsampling);
    if (rc) return rc;
    if (f->alpha_premultiplied) return c->fail(SSIMU2_ERR_UNSUPPORTED, "premultiplied alpha is not supported: alpha_premultiplied must be 0");
    if (!f->alpha) return SSIMU2_OK;
    const uint32_t sample = f->yuv.depth > 8 ? 2u : 1u;
    if ((uint64_t)f->alpha_row_bytes < (uint64_t)w * sample)
        return c->fail(SSIMU2_ERR_INVALID_ARG, "alpha_row_bytes smaller than one row of samples");
    if (sample == 2 && (((uintptr_t)f->alpha | f->alpha_row_bytes) & 1u))
        return c->fail(SSIMU2_ERR_INVALID_ARG, "16-bit alpha pointer or alpha_row_bytes not 2-byte aligned");
    return SSIMU2_OK;
}

// check_rgba's background rule.
int ssimu2h::check_background(ssimu2_ctx* c, uint32_t background_rgb) {
    if (background_rgb > 0xFFFFFFu) return c->fail(SSIMU2_ERR_INVALID_ARG, "background_rgb is 0xRRGGBB: the upper byte must be 0");
    return SSIMU2_OK;
}

// What an against-reference call answers to a reference that recorded no background.
int ssimu2h::no_background(ssimu2_ctx* c) {
    return c->fail(SSIMU2_ERR_INVALID_ARG,
                   "the reference was not set by ssimu2_set_reference_yuva or ssimu2_set_reference_rgba8: no background recorded");
}

namespace {

constexpr uint32_t kCompositeTop = 65025;  // 255 * 255, the largest composite code: SSIMU2_ALPHA_CODES - 1

// What the unpacking of a frame needs beyond the planes.  `chroma` comes first, as ChromaAux::yuv does.
struct YuvaAux {
    ChromaAux chroma;
    YuvaK k;
    int sub;  // k_yuva_to_codes' SUB
    int div;  // ... and DIV
    bool alpha;
};

// The planes in `stage` (plane_off, each with its own size; the alpha plane last) -> the tight u16 frame of composite
// codes `dst`.
void composite(ssimu2_ctx* c, const Feed& f, uint32_t w, uint32_t h, void* dst) {
    const YuvaAux& a = *(const YuvaAux*)f.aux;
    const uint8_t* const base = c->stage.as<uint8_t>();
    const bool colour = a.sub != 2;
    const uint8_t* const pu = colour ? base + plane_off(f, 1, w, h) : base;
    const uint8_t* const pv = colour ? base + plane_off(f, 2, w, h) : base;
    const uint8_t* const pa = a.alpha ? base + plane_off(f, f.nplanes - 1, w, h) : nullptr;
    const uint32_t rows = a.chroma.vertical ? (h + 1u) / 2u : h;
    const dim3 grid(((w + 3) / 4 + 255) / 256, rows < 65535u ? rows : 65535u);
    using Kernel = void (*)(const uint8_t*, const uint8_t*, const uint8_t*, const uint8_t*, uint32_t, uint32_t, uint32_t,
                            uint32_t, uint32_t, uint32_t, YuvK, YuvaK, uint16_t*);
    // [S - 1][DIV][shape]; shape: 4:4:4, 4:0:0, then 4:2:2 nearest / bilinear, 4:2:0 nearest / bilinear.  DIV_NONE needs
    // depth 8: one-byte samples
#define YUVA_SHAPES(S, DIV)                                                                                      \
    {k_yuva_to_codes<S, 0, false, false, DIV>, k_yuva_to_codes<S, 2, false, false, DIV>,                         \
     k_yuva_to_codes<S, 1, false, false, DIV>, k_yuva_to_codes<S, 1, false, true, DIV>,                          \
     k_yuva_to_codes<S, 1, true, false, DIV>,  k_yuva_to_codes<S, 1, true, true, DIV>}
    static const Kernel kernels[2][3][6] = {
        {YUVA_SHAPES(1, DIV_NONE), YUVA_SHAPES(1, DIV_MULHI), YUVA_SHAPES(1, DIV_PLAIN)},
        {{}, YUVA_SHAPES(2, DIV_MULHI), YUVA_SHAPES(2, DIV_PLAIN)}};
#undef YUVA_SHAPES
    const int shape = a.sub == 0 ? 0 : a.sub == 2 ? 1 : 2 + 2 * a.chroma.vertical + a.chroma.bilinear;
    const uint32_t last = f.nplanes - 1;
    launch(kernels[f.sample - 1][a.div][shape], grid, dim3(256), 0, c->stream, base, pu, pv, pa, f.plane[0].row_bytes,
           colour ? f.plane[1].row_bytes : 0u, colour ? f.plane[2].row_bytes : 0u, a.alpha ? f.plane[last].row_bytes : 0u, w,
           h, a.chroma.yuv.k, a.k, (uint16_t*)dst);
}

// One frame in host memory composited over `bg`, for a w x h call.  `aux` outlives the call.
Feed yuva_feed(const ssimu2_yuva_frame& f, uint32_t w, uint32_t h, uint32_t rgb_depth, uint32_t upsampling, uint32_t bg,
               YuvaAux* aux) {
    Feed feed = chroma_feed(f.yuv, w, h, rgb_depth, upsampling, &aux->chroma);
    aux->k = yuva_constants(f.yuv.depth, rgb_depth, bg);
    aux->sub = aux->chroma.yuv.mono ? 2 : (f.yuv.format == SSIMU2_YUV_444 ? 0 : 1);
    // OAVIF_YUVA_DIVISION = mulhi | plain forces one form of the division, for the measurement of DESIGN.md section 17 and
    // the test that all three give the same codes; unset, the rule is: none at 8 and 8, else mulhi
    const char* const how = getenv("OAVIF_YUVA_DIVISION");
    aux->div = yuva_division(f.yuv.depth, rgb_depth);
    if (how && !strcmp(how, "mulhi")) aux->div = DIV_MULHI;
    if (how && !strcmp(how, "plain")) aux->div = DIV_PLAIN;
    aux->alpha = f.alpha != nullptr;
    if (aux->alpha) feed.plane[feed.nplanes++] = {f.alpha, f.alpha_row_bytes};
    feed.top = kCompositeTop;
    feed.bg = (int64_t)bg;
    feed.unpack = composite;
    feed.aux = aux;
    return feed;
}

}  // namespace

extern "C" {

int ssimu2_composite_yuva(ssimu2_ctx* c, const ssimu2_yuva_frame* frame, uint32_t w, uint32_t h, uint32_t rgb_depth,
                          uint32_t chroma_upsampling, uint32_t background_rgb, uint16_t* out_codes) {
    REMOTE_REFUSE(c, "ssimu2_composite_yuva");
    int rc = check_args(c, frame, out_codes, w, h);
    if (rc || (rc = check_yuva(c, frame, w, rgb_depth, chroma_upsampling)) || (rc = check_background(c, background_rgb))) return rc;
    YuvaAux aux;
    return feed_codes(c, yuva_feed(*frame, w, h, rgb_depth, chroma_upsampling, background_rgb, &aux), w, h, out_codes,
                      "ssimu2_composite_yuva");
}

int ssimu2_score_yuva(ssimu2_ctx* c, const ssimu2_yuva_frame* ref_frame, const ssimu2_yuva_frame* dist_frame, uint32_t w,
                      uint32_t h, uint32_t rgb_depth, uint32_t chroma_upsampling, uint32_t background_rgb, double* out_score) {
    REMOTE_REFUSE(c, "ssimu2_score_yuva");
    const uint32_t up = chroma_upsampling, bg = background_rgb;
    int rc = check_args(c, ref_frame, dist_frame, w, h);
    if (rc || (rc = check_yuva(c, ref_frame, w, rgb_depth, up)) || (rc = check_yuva(c, dist_frame, w, rgb_depth, up)) ||
        (rc = check_background(c, bg)))
        return rc;
    if (!out_score) return c->fail(SSIMU2_ERR_INVALID_ARG, "null out_score");
    YuvaAux ra, da;
    return score_pair(c, yuva_feed(*ref_frame, w, h, rgb_depth, up, bg, &ra), yuva_feed(*dist_frame, w, h, rgb_depth, up, bg, &da),
                      w, h, out_score);
}

int ssimu2_set_reference_yuva(ssimu2_ctx* c, const ssimu2_yuva_frame* frame, uint32_t w, uint32_t h, uint32_t rgb_depth,
                              uint32_t chroma_upsampling, uint32_t background_rgb) {
    REMOTE_REFUSE(c, "ssimu2_set_reference_yuva");
    int rc = check_args(c, frame, frame, w, h);
    if (rc || (rc = check_yuva(c, frame, w, rgb_depth, chroma_upsampling)) || (rc = check_background(c, background_rgb))) return rc;
    YuvaAux aux;
    return feed_reference(c, yuva_feed(*frame, w, h, rgb_depth, chroma_upsampling, background_rgb, &aux), w, h);
}

int ssimu2_score_against_reference_yuva(ssimu2_ctx* c, const ssimu2_yuva_frame* frame, uint32_t rgb_depth,
                                        uint32_t chroma_upsampling, double* out_score) {
    REMOTE_REFUSE(c, "ssimu2_score_against_reference_yuva");
    int rc = check_against(c, frame && out_score);
    if (rc) return rc;
    if (c->ref.bg < 0) return no_background(c);
    if ((rc = check_yuva(c, frame, c->ref.w, rgb_depth, chroma_upsampling))) return rc;
    YuvaAux aux;
    return score_against(c, yuva_feed(*frame, c->ref.w, c->ref.h, rgb_depth, chroma_upsampling, (uint32_t)c->ref.bg, &aux),
                         out_score);
}

int ssimu2_error_map_yuva(ssimu2_ctx* c, const ssimu2_yuva_frame* ref_frame, const ssimu2_yuva_frame* dist_frame, uint32_t w,
                          uint32_t h, uint32_t rgb_depth, uint32_t chroma_upsampling, uint32_t background_rgb, float* out_map,
                          double* out_score) {
    REMOTE_REFUSE(c, "ssimu2_error_map_yuva");
    const uint32_t up = chroma_upsampling, bg = background_rgb;
    int rc = check_args(c, ref_frame, dist_frame, w, h);
    if (rc || (rc = check_yuva(c, ref_frame, w, rgb_depth, up)) || (rc = check_yuva(c, dist_frame, w, rgb_depth, up)) ||
        (rc = check_background(c, bg)))
        return rc;
    if (!out_score) return c->fail(SSIMU2_ERR_INVALID_ARG, "null out_score");
    if (!out_map) return c->fail(SSIMU2_ERR_INVALID_ARG, "null out_map");
    YuvaAux ra, da;
    return map_pair(c, yuva_feed(*ref_frame, w, h, rgb_depth, up, bg, &ra), yuva_feed(*dist_frame, w, h, rgb_depth, up, bg, &da),
                    w, h, out_map, out_score);
}

int ssimu2_error_map_against_reference_yuva(ssimu2_ctx* c, const ssimu2_yuva_frame* frame, uint32_t rgb_depth,
                                            uint32_t chroma_upsampling, float* out_map, double* out_score) {
    REMOTE_REFUSE(c, "ssimu2_error_map_against_reference_yuva");
    int rc = check_against(c, frame && out_score && out_map);
    if (rc) return rc;
    if (c->ref.bg < 0) return no_background(c);
    if ((rc = check_yuva(c, frame, c->ref.w, rgb_depth, chroma_upsampling))) return rc;
    YuvaAux aux;
    return map_against(c, yuva_feed(*frame, c->ref.w, c->ref.h, rgb_depth, chroma_upsampling, (uint32_t)c->ref.bg, &aux),
                       out_map, out_score);
}

}  // extern "C"
