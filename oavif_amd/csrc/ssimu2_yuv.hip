// YUV input of the MI355X SSIMULACRA2 scorer: the entry points of include/ssimu2_hip_yuv.h.
//
// A translation unit of its own: one kernel template, one Feed constructor, one check and four functions over
// ssimu2_host.h, the list of what a front end may use of the scorer.  Its object is linked with the extension library's
// objects into liboavif_hip_yuv.so; the other three libraries contain none of this, and their exports are what they were.
//
// A decoder's Y, U and V planes become a u16 frame of RGB codes of the caller's depth (k_yuv_to_codes: the colour matrix
// in fp32, operation for operation the header's definition) that the 16-bit front end reads through that depth's
// table: Src16{codes, w * 6, 3, table, 2^rgb_depth - 1}.  No pyramid, marching, recursive or finalize kernel knows about
// YUV.  To the host code a YUV frame is one more Feed, of three planes (yuv_feed below): the three shapes of a call --
// score_pair, feed_reference, score_against -- are the product's.
#include "../../include/ssimu2_hip_yuv.h"
#include "ssimu2_host.h"
#include "ssimu2_yuv_pixel.h"

using namespace ssimu2h;

namespace ssimu2 {

// YuvK, the constants of one conversion (formed on the host: yuv_constants), is ssimu2_host.h's; the two halves of the
// arithmetic -- yuv_unorm, yuv_codes -- are ssimu2_yuv_pixel.h's, shared with the subsampled formats' unit.

// One pixel: the samples y, u, v -> its three codes.  MONO: Cb = Cr = 0, which leaves R = G = B = Y in the same bits.
template <bool MONO>
__device__ __forceinline__ void yuv_pixel(uint32_t y, uint32_t u, uint32_t v, const YuvK& k, uint32_t* code) {
    const float Y = yuv_unorm(y, k.max_code, k.bias_y, k.range_y);
    if (MONO) {
        code[0] = code[1] = code[2] = yuv_code(Y, k.top);
        return;
    }
    yuv_codes(Y, yuv_unorm(u, k.max_code, k.bias_uv, k.range_uv), yuv_unorm(v, k.max_code, k.bias_uv, k.range_uv), k, code);
}

// ---------------------------------------------------------------------------------------------
// Planes of S-byte samples (S = 1: depth 8; S = 2: depth 10 and 12), rows `pitch` bytes apart at any alignment (2-byte
// for S = 2) -> tight u16 RGB codes.  Shaped like k_composite_rgba8: a lane takes four pixels of one row -- per plane
// one unaligned dword load (S = 1) or two (S = 2) -- and makes six dword stores (a row of codes starts 6 * w * y
// bytes in, 2-byte aligned only); the last w % 4 pixels of a row go sample by sample.  Rows beyond gridDim.y are taken
// in further rounds.  HBM-bound: 9 bytes per pixel for S = 1, 12 for S = 2 (7 and 8 for MONO).
// ---------------------------------------------------------------------------------------------
template <int S, bool MONO>
__global__ __launch_bounds__(256) void k_yuv_to_codes(const uint8_t* __restrict__ py, const uint8_t* __restrict__ pu,
                                                      const uint8_t* __restrict__ pv, uint32_t pitch_y,
                                                      uint32_t pitch_u, uint32_t pitch_v, uint32_t w, uint32_t h, YuvK k,
                                                      uint16_t* __restrict__ dst) {
    const uint32_t x0 = (blockIdx.x * 256u + threadIdx.x) * 4u;
    if (x0 >= w) return;
    for (uint32_t y = blockIdx.y; y < h; y += gridDim.y) {
        const uint8_t* s[3] = {py + (size_t)y * pitch_y + (size_t)x0 * S, MONO ? nullptr : pu + (size_t)y * pitch_u + (size_t)x0 * S,
                               MONO ? nullptr : pv + (size_t)y * pitch_v + (size_t)x0 * S};
        uint16_t* d = dst + ((size_t)y * w + x0) * 3u;
        if (x0 + 4u <= w) {
            uint32_t smp[3][4] = {};  // [plane][pixel]
#pragma unroll
            for (int p = 0; p < (MONO ? 1 : 3); ++p) {
                if (S == 1) {
                    uint32_t four;
                    __builtin_memcpy(&four, s[p], 4);
#pragma unroll
                    for (int i = 0; i < 4; ++i) smp[p][i] = (four >> (8 * i)) & 0xFFu;
                } else {
                    uint32_t two[2];
                    __builtin_memcpy(&two[0], s[p], 4);
                    __builtin_memcpy(&two[1], s[p] + 4, 4);
#pragma unroll
                    for (int i = 0; i < 4; ++i) smp[p][i] = (two[i >> 1] >> (16 * (i & 1))) & 0xFFFFu;
                }
            }
            uint32_t n[12];
#pragma unroll
            for (int i = 0; i < 4; ++i) yuv_pixel<MONO>(smp[0][i], smp[1][i], smp[2][i], k, n + 3 * i);
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                const uint32_t pair = n[2 * i] | (n[2 * i + 1] << 16);
                __builtin_memcpy((uint8_t*)d + 4 * i, &pair, 4);
            }
        } else {
            for (uint32_t i = 0; x0 + i < w; ++i) {
                uint32_t smp[3] = {};
#pragma unroll
                for (int p = 0; p < (MONO ? 1 : 3); ++p) {
                    if (S == 1) {
                        smp[p] = s[p][i];
                    } else {
                        uint16_t one;
                        __builtin_memcpy(&one, s[p] + 2 * i, 2);
                        smp[p] = one;
                    }
                }
                uint32_t n[3];
                yuv_pixel<MONO>(smp[0], smp[1], smp[2], k, n);
#pragma unroll
                for (int c = 0; c < 3; ++c) d[3 * i + c] = (uint16_t)n[c];
            }
        }
    }
}

}  // namespace ssimu2

using namespace ssimu2;

namespace {

// The header's constants, each operation in fp32 and rounded once (the host code is built with -ffp-contract=off too).
YuvK yuv_constants(const ssimu2_yuv_frame& f, uint32_t rgb_depth) {
    float kr = 0.299f, kb = 0.114f;  // 5, 6 and 2 (unspecified)
    if (f.matrix_coefficients == 1) kr = 0.2126f, kb = 0.0722f;
    if (f.matrix_coefficients == 9) kr = 0.2627f, kb = 0.0593f;
    const uint32_t m = (1u << f.depth) - 1u, scale = 1u << (f.depth - 8);
    YuvK k;
    k.bias_y = f.full_range ? 0.0f : (float)(16u * scale);
    k.range_y = f.full_range ? (float)m : (float)(219u * scale);
    k.bias_uv = (float)(1u << (f.depth - 1));
    k.range_uv = f.full_range ? (float)m : (float)(224u * scale);
    const float one_kr = 1.0f - kr, one_kb = 1.0f - kb;
    k.r_cr = 2.0f * one_kr;
    k.b_cb = 2.0f * one_kb;
    k.g_cr = kr * one_kr;
    k.g_cb = kb * one_kb;
    k.kg = one_kr - kb;
    k.top = (float)((1u << rgb_depth) - 1u);
    k.max_code = m;
    return k;
}

}  // namespace

// Argument checks of one frame for a w x h call (the ctx is not null).
int ssimu2h::check_yuv(ssimu2_ctx* c, const ssimu2_yuv_frame* f, uint32_t w, uint32_t rgb_depth) {
    if (!f) return c->fail(SSIMU2_ERR_INVALID_ARG, "null frame");
    if (f->depth != 8 && f->depth != 10 && f->depth != 12) return c->fail(SSIMU2_ERR_UNSUPPORTED, "depth must be 8, 10 or 12");
    if (rgb_depth < 8 || rgb_depth > 16) return c->fail(SSIMU2_ERR_UNSUPPORTED, "rgb_depth must be 8..16");
    if (f->format != SSIMU2_YUV_444 && f->format != SSIMU2_YUV_400)
        return c->fail(SSIMU2_ERR_UNSUPPORTED, "format must be 4:4:4 or 4:0:0: subsampled chroma is not converted");
    const uint32_t mc = f->matrix_coefficients;
    if (mc != 1 && mc != 2 && mc != 5 && mc != 6 && mc != 9)
        return c->fail(SSIMU2_ERR_UNSUPPORTED, "matrix_coefficients must be 1, 2, 5, 6 or 9 (identity and YCgCo are not converted)");
    if (f->full_range > 1) return c->fail(SSIMU2_ERR_INVALID_ARG, "full_range must be 0 or 1");
    const uint32_t sample = f->depth > 8 ? 2u : 1u;
    for (uint32_t p = 0; p < (f->format == SSIMU2_YUV_400 ? 1u : 3u); ++p) {
        if (!f->planes[p]) return c->fail(SSIMU2_ERR_INVALID_ARG, "null plane");
        if ((uint64_t)f->row_bytes[p] < (uint64_t)w * sample)
            return c->fail(SSIMU2_ERR_INVALID_ARG, "row_bytes smaller than one row of samples");
        if (sample == 2 && (((uintptr_t)f->planes[p] | f->row_bytes[p]) & 1u))
            return c->fail(SSIMU2_ERR_INVALID_ARG, "16-bit plane pointer or row_bytes not 2-byte aligned");
    }
    return SSIMU2_OK;
}

namespace {

// The planes in `stage` (plane_off) -> the tight u16 frame of codes `dst`.
void convert(ssimu2_ctx* c, const Feed& f, uint32_t w, uint32_t h, void* dst) {
    const YuvAux& a = *(const YuvAux*)f.aux;
    const uint8_t* const base = c->stage.as<uint8_t>();
    const uint8_t* p[3] = {base, base, base};
    for (uint32_t q = 1; q < f.nplanes; ++q) p[q] = base + plane_off(f, q, w, h);
    const uint32_t pitch[3] = {f.plane[0].row_bytes, f.plane[1].row_bytes, f.plane[2].row_bytes};
    const dim3 grid(((w + 3) / 4 + 255) / 256, h < 65535u ? h : 65535u);
    auto* const kernel = f.sample == 1 ? (a.mono ? k_yuv_to_codes<1, true> : k_yuv_to_codes<1, false>)
                                       : (a.mono ? k_yuv_to_codes<2, true> : k_yuv_to_codes<2, false>);
    launch(kernel, grid, dim3(256), 0, c->stream, p[0], p[1], p[2], pitch[0], pitch[1], pitch[2], w, h, a.k, (uint16_t*)dst);
}

}  // namespace

// One YUV frame in host memory: its planes go through the staging buffer as they are, the front end reads the codes
// through the table of depth rgb_depth.  `aux` outlives the call.
Feed ssimu2h::yuv_feed(const ssimu2_yuv_frame& f, uint32_t rgb_depth, YuvAux* aux) {
    *aux = {yuv_constants(f, rgb_depth), f.format == SSIMU2_YUV_400};
    Feed feed = staged1(f.planes[0], f.row_bytes[0], 1u, f.depth > 8 ? 2u : 1u, (1u << rgb_depth) - 1u, convert);
    if (!aux->mono) {
        feed.plane[1] = {f.planes[1], f.row_bytes[1]};
        feed.plane[2] = {f.planes[2], f.row_bytes[2]};
        feed.nplanes = 3;
    }
    feed.aux = aux;
    return feed;
}

extern "C" {

int ssimu2_convert_yuv(ssimu2_ctx* c, const ssimu2_yuv_frame* frame, uint32_t w, uint32_t h, uint32_t rgb_depth,
                       uint16_t* out_codes) {
    REMOTE_REFUSE(c, "ssimu2_convert_yuv");
    int rc = check_args(c, frame, out_codes, w, h);
    if (rc || (rc = check_yuv(c, frame, w, rgb_depth))) return rc;
    YuvAux aux;
    return feed_codes(c, yuv_feed(*frame, rgb_depth, &aux), w, h, out_codes, "ssimu2_convert_yuv");
}

int ssimu2_score_yuv(ssimu2_ctx* c, const ssimu2_yuv_frame* ref_frame, const ssimu2_yuv_frame* dist_frame, uint32_t w,
                     uint32_t h, uint32_t rgb_depth, double* out_score) {
    REMOTE_REFUSE(c, "ssimu2_score_yuv");
    int rc = check_args(c, ref_frame, dist_frame, w, h);
    if (rc || (rc = check_yuv(c, ref_frame, w, rgb_depth)) || (rc = check_yuv(c, dist_frame, w, rgb_depth))) return rc;
    if (!out_score) return c->fail(SSIMU2_ERR_INVALID_ARG, "null out_score");
    YuvAux ra, da;
    return score_pair(c, yuv_feed(*ref_frame, rgb_depth, &ra), yuv_feed(*dist_frame, rgb_depth, &da), w, h, out_score);
}

int ssimu2_set_reference_yuv(ssimu2_ctx* c, const ssimu2_yuv_frame* frame, uint32_t w, uint32_t h, uint32_t rgb_depth) {
    REMOTE_REFUSE(c, "ssimu2_set_reference_yuv");
    int rc = check_args(c, frame, frame, w, h);
    if (rc || (rc = check_yuv(c, frame, w, rgb_depth))) return rc;
    YuvAux aux;
    return feed_reference(c, yuv_feed(*frame, rgb_depth, &aux), w, h);
}

int ssimu2_score_against_reference_yuv(ssimu2_ctx* c, const ssimu2_yuv_frame* frame, uint32_t rgb_depth,
                                       double* out_score) {
    REMOTE_REFUSE(c, "ssimu2_score_against_reference_yuv");
    int rc = check_against(c, frame && out_score);
    if (rc || (rc = check_yuv(c, frame, c->ref.w, rgb_depth))) return rc;
    YuvAux aux;
    return score_against(c, yuv_feed(*frame, rgb_depth, &aux), out_score);
}

}  // extern "C"
