// Subsampled YUV input of the MI355X SSIMULACRA2 scorer: the entry points of include/ssimu2_hip_chroma.h (DESIGN.md
// section 16).
//
// A translation unit of its own over ssimu2_host.h, like the RGBA, YUV and map units: one kernel template, one Feed
// constructor, one check and six functions.  Its object is linked with the map library's objects into
// liboavif_hip_chroma.so (and liboavif_hip_yuva.so on top of it); the other five libraries contain none of this, and
// their exports are what they were.
//
// A 4:2:2 or 4:2:0 frame is a YUV Feed (yuv_feed: the one yuv_constants) whose planes 1 and 2 carry their own size
// (Plane::w, Plane::h), so that only cw x ch samples of each leave the caller's memory, and whose unpacking is
// k_yuv_chroma_to_codes below instead of k_yuv_to_codes.  A 4:4:4 or 4:0:0 frame is yuv_feed's Feed as it is.  The
// three shapes of a call and the two of a map are the scorer's.
#include "../../include/ssimu2_hip_chroma.h"
#include "ssimu2_host.h"
#include "ssimu2_yuv_pixel.h"

using namespace ssimu2h;

namespace ssimu2 {

// sample_at, samples_at (a plane row's samples in one load) and chroma_blend are ssimu2_yuv_pixel.h's, shared with the
// alpha unit.

// ---------------------------------------------------------------------------------------------
// Planes of S-byte samples -- Y of w x h, U and V of cw x ch (cw = (w + 1) / 2; V: ch = (h + 1) / 2, 4:2:0; else
// ch = h, 4:2:2), rows `pitch` bytes apart at any alignment (2-byte for S = 2) -> tight u16 RGB codes, the chroma
// upsampled as include/ssimu2_hip_chroma.h defines it.  A lane takes four luma columns x0..x0+3 of the luma rows that
// share chroma row r: two for V (2r, 2r + 1), else one -- 8 or 4 pixels.  It normalises the chroma samples those pixels
// blend once per plane (yuv_unorm): columns x0/2 - 1 .. x0/2 + 2 of rows r - 1, r, r + 1 for BILINEAR and V (4 x 3),
// of row r alone without V (4 x 1), columns x0/2 and x0/2 + 1 of row r for nearest (2 x 1).  Every neighbour index is
// clamped into the plane before its load, which is the header's ac / ar rule: nothing is read before a plane's first
// sample or beyond its last.  A lane none of whose column indices is clamped -- every lane but a row's first and last
// -- takes the adjacent samples of a row in one load (samples_at), the others sample by sample.  Luma goes as in k_yuv_to_codes: per row one unaligned dword load (S = 1) or two (S = 2)
// and six dword stores; the last w % 4 pixels of a row go sample by sample.  Chroma rows beyond gridDim.y are taken in
// further rounds.  No LDS, no scratch (every array index is a constant once unrolled).
// ---------------------------------------------------------------------------------------------
template <int S, bool V, bool BILINEAR>
__global__ __launch_bounds__(256) void k_yuv_chroma_to_codes(const uint8_t* __restrict__ py, const uint8_t* __restrict__ pu,
                                                             const uint8_t* __restrict__ pv, uint32_t pitch_y,
                                                             uint32_t pitch_u, uint32_t pitch_v, uint32_t w, uint32_t h,
                                                             YuvK k, uint16_t* __restrict__ dst) {
    constexpr int NR = (BILINEAR && V) ? 3 : 1;  // chroma rows a lane holds: r - 1, r, r + 1, or r alone
    constexpr int NC = BILINEAR ? 4 : 2;         // chroma columns: c0 - 1 .. c0 + 2, or c0, c0 + 1
    constexpr int QC = NR == 3 ? 1 : 0;          // where row r is among them
    constexpr int LC = BILINEAR ? 1 : 0;         // where column c0 is
    const uint32_t x0 = (blockIdx.x * 256u + threadIdx.x) * 4u;
    if (x0 >= w) return;
    const uint32_t cw = (w + 1u) / 2u, ch = V ? (h + 1u) / 2u : h;
    const uint32_t c0 = x0 >> 1;
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
#pragma unroll
        for (int jj = 0; jj < (V ? 2 : 1); ++jj) {
            const uint32_t j = V ? 2u * r + (uint32_t)jj : r;
            if (j >= h) continue;  // the last chroma row of an odd height has one luma row
            const int qn = NR == 3 ? 2 * jj : 0;  // the neighbour row: above an even luma row, below an odd one
            const uint8_t* const sy = py + (size_t)j * pitch_y + (size_t)x0 * S;
            uint16_t* const d = dst + ((size_t)j * w + x0) * 3u;
            // pixel i of the lane's four, of luma sample y -> its three codes
            auto pixel = [&](int i, uint32_t y, uint32_t* code) {
                const int lc = LC + (i >> 1), ln = BILINEAR ? ((i & 1) ? lc + 1 : lc - 1) : lc;
                float Cb = cb[QC][lc], Cr = cr[QC][lc];
                if (BILINEAR) {
                    Cb = chroma_blend(cb[QC][lc], cb[QC][ln], cb[qn][lc], cb[qn][ln]);
                    Cr = chroma_blend(cr[QC][lc], cr[QC][ln], cr[qn][lc], cr[qn][ln]);
                }
                yuv_codes(yuv_unorm(y, k.max_code, k.bias_y, k.range_y), Cb, Cr, k, code);
            };
            if (x0 + 4u <= w) {
                uint32_t smp[4];
                if (S == 1) {
                    uint32_t four;
                    __builtin_memcpy(&four, sy, 4);
#pragma unroll
                    for (int i = 0; i < 4; ++i) smp[i] = (four >> (8 * i)) & 0xFFu;
                } else {
                    uint32_t two[2];
                    __builtin_memcpy(&two[0], sy, 4);
                    __builtin_memcpy(&two[1], sy + 4, 4);
#pragma unroll
                    for (int i = 0; i < 4; ++i) smp[i] = (two[i >> 1] >> (16 * (i & 1))) & 0xFFFFu;
                }
                uint32_t n[12];
#pragma unroll
                for (int i = 0; i < 4; ++i) pixel(i, smp[i], n + 3 * i);
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
                        pixel(i, sample_at<S>(sy, (uint32_t)i), n);
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

namespace {

// ChromaAux, what the unpacking of a frame needs beyond the planes, is ssimu2_host.h's.

bool subsampled(uint32_t format) { return format == SSIMU2_YUV_422 || format == SSIMU2_YUV_420; }

}  // namespace

// Argument checks of one frame for a w x h call (the ctx is not null): check_yuv's, with formats 2 and 3 let through
// and their chroma planes held to cw samples per row.
int ssimu2h::check_chroma(ssimu2_ctx* c, const ssimu2_yuv_frame* f, uint32_t w, uint32_t rgb_depth, uint32_t upsampling) {
    if (upsampling > SSIMU2_CHROMA_NEAREST) return c->fail(SSIMU2_ERR_INVALID_ARG, "chroma_upsampling must be 0 (bilinear) or 1 (nearest)");
    if (!f || !subsampled(f->format)) {
        if (f && f->format != SSIMU2_YUV_444 && f->format != SSIMU2_YUV_400)
            return c->fail(SSIMU2_ERR_UNSUPPORTED, "format must be 4:4:4, 4:2:2, 4:2:0 or 4:0:0");
        return check_yuv(c, f, w, rgb_depth);
    }
    ssimu2_yuv_frame luma = *f;  // everything but the chroma planes is checked as a 4:0:0 frame's
    luma.format = SSIMU2_YUV_400;
    const int rc = check_yuv(c, &luma, w, rgb_depth);
    if (rc) return rc;
    const uint32_t sample = f->depth > 8 ? 2u : 1u, cw = (w + 1u) / 2u;
    for (uint32_t p = 1; p < 3; ++p) {
        if (!f->planes[p]) return c->fail(SSIMU2_ERR_INVALID_ARG, "null plane");
        if ((uint64_t)f->row_bytes[p] < (uint64_t)cw * sample)
            return c->fail(SSIMU2_ERR_INVALID_ARG, "chroma row_bytes smaller than one row of (w + 1) / 2 samples");
        if (sample == 2 && (((uintptr_t)f->planes[p] | f->row_bytes[p]) & 1u))
            return c->fail(SSIMU2_ERR_INVALID_ARG, "16-bit plane pointer or row_bytes not 2-byte aligned");
    }
    return SSIMU2_OK;
}

namespace {

// The planes in `stage` (plane_off, each with its own size) -> the tight u16 frame of codes `dst`.
void convert(ssimu2_ctx* c, const Feed& f, uint32_t w, uint32_t h, void* dst) {
    const ChromaAux& a = *(const ChromaAux*)f.aux;
    const uint8_t* const base = c->stage.as<uint8_t>();
    const uint8_t* const pu = base + plane_off(f, 1, w, h);
    const uint8_t* const pv = base + plane_off(f, 2, w, h);
    const uint32_t rows = a.vertical ? (h + 1u) / 2u : h;
    const dim3 grid(((w + 3) / 4 + 255) / 256, rows < 65535u ? rows : 65535u);
    using Kernel = void (*)(const uint8_t*, const uint8_t*, const uint8_t*, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t,
                            YuvK, uint16_t*);
    static const Kernel kernels[2][2][2] = {  // [S - 1][vertical][bilinear]
        {{k_yuv_chroma_to_codes<1, false, false>, k_yuv_chroma_to_codes<1, false, true>},
         {k_yuv_chroma_to_codes<1, true, false>, k_yuv_chroma_to_codes<1, true, true>}},
        {{k_yuv_chroma_to_codes<2, false, false>, k_yuv_chroma_to_codes<2, false, true>},
         {k_yuv_chroma_to_codes<2, true, false>, k_yuv_chroma_to_codes<2, true, true>}}};
    launch(kernels[f.sample - 1][a.vertical][a.bilinear], grid, dim3(256), 0, c->stream, base, pu, pv, f.plane[0].row_bytes,
           f.plane[1].row_bytes, f.plane[2].row_bytes, w, h, a.yuv.k, (uint16_t*)dst);
}

}  // namespace

// One frame of any of the four formats in host memory, for a w x h call.  `aux` outlives the call.
Feed ssimu2h::chroma_feed(const ssimu2_yuv_frame& f, uint32_t w, uint32_t h, uint32_t rgb_depth, uint32_t upsampling,
                          ChromaAux* aux) {
    aux->vertical = aux->bilinear = false;
    if (!subsampled(f.format)) return yuv_feed(f, rgb_depth, &aux->yuv);
    ssimu2_yuv_frame full = f;  // three planes and the constants, as of a 4:4:4 frame
    full.format = SSIMU2_YUV_444;
    Feed feed = yuv_feed(full, rgb_depth, &aux->yuv);
    aux->vertical = f.format == SSIMU2_YUV_420;
    aux->bilinear = upsampling == SSIMU2_CHROMA_BILINEAR;
    for (uint32_t p = 1; p < 3; ++p) {
        feed.plane[p].w = (w + 1u) / 2u;
        feed.plane[p].h = aux->vertical ? (h + 1u) / 2u : h;
    }
    feed.unpack = convert;
    feed.aux = aux;
    return feed;
}

extern "C" {

int ssimu2_convert_yuv_chroma(ssimu2_ctx* c, const ssimu2_yuv_frame* frame, uint32_t w, uint32_t h, uint32_t rgb_depth,
                              uint32_t chroma_upsampling, uint16_t* out_codes) {
    REMOTE_REFUSE(c, "ssimu2_convert_yuv_chroma");
    int rc = check_args(c, frame, out_codes, w, h);
    if (rc || (rc = check_chroma(c, frame, w, rgb_depth, chroma_upsampling))) return rc;
    ChromaAux aux;
    return feed_codes(c, chroma_feed(*frame, w, h, rgb_depth, chroma_upsampling, &aux), w, h, out_codes,
                      "ssimu2_convert_yuv_chroma");
}

int ssimu2_score_yuv_chroma(ssimu2_ctx* c, const ssimu2_yuv_frame* ref_frame, const ssimu2_yuv_frame* dist_frame,
                            uint32_t w, uint32_t h, uint32_t rgb_depth, uint32_t chroma_upsampling, double* out_score) {
    REMOTE_REFUSE(c, "ssimu2_score_yuv_chroma");
    const uint32_t up = chroma_upsampling;
    int rc = check_args(c, ref_frame, dist_frame, w, h);
    if (rc || (rc = check_chroma(c, ref_frame, w, rgb_depth, up)) || (rc = check_chroma(c, dist_frame, w, rgb_depth, up)))
        return rc;
    if (!out_score) return c->fail(SSIMU2_ERR_INVALID_ARG, "null out_score");
    ChromaAux ra, da;
    return score_pair(c, chroma_feed(*ref_frame, w, h, rgb_depth, up, &ra), chroma_feed(*dist_frame, w, h, rgb_depth, up, &da),
                      w, h, out_score);
}

int ssimu2_set_reference_yuv_chroma(ssimu2_ctx* c, const ssimu2_yuv_frame* frame, uint32_t w, uint32_t h,
                                    uint32_t rgb_depth, uint32_t chroma_upsampling) {
    REMOTE_REFUSE(c, "ssimu2_set_reference_yuv_chroma");
    int rc = check_args(c, frame, frame, w, h);
    if (rc || (rc = check_chroma(c, frame, w, rgb_depth, chroma_upsampling))) return rc;
    ChromaAux aux;
    return feed_reference(c, chroma_feed(*frame, w, h, rgb_depth, chroma_upsampling, &aux), w, h);
}

int ssimu2_score_against_reference_yuv_chroma(ssimu2_ctx* c, const ssimu2_yuv_frame* frame, uint32_t rgb_depth,
                                              uint32_t chroma_upsampling, double* out_score) {
    REMOTE_REFUSE(c, "ssimu2_score_against_reference_yuv_chroma");
    int rc = check_against(c, frame && out_score);
    if (rc || (rc = check_chroma(c, frame, c->ref.w, rgb_depth, chroma_upsampling))) return rc;
    ChromaAux aux;
    return score_against(c, chroma_feed(*frame, c->ref.w, c->ref.h, rgb_depth, chroma_upsampling, &aux), out_score);
}

int ssimu2_error_map_yuv_chroma(ssimu2_ctx* c, const ssimu2_yuv_frame* ref_frame, const ssimu2_yuv_frame* dist_frame,
                                uint32_t w, uint32_t h, uint32_t rgb_depth, uint32_t chroma_upsampling, float* out_map,
                                double* out_score) {
    REMOTE_REFUSE(c, "ssimu2_error_map_yuv_chroma");
    const uint32_t up = chroma_upsampling;
    int rc = check_args(c, ref_frame, dist_frame, w, h);
    if (rc || (rc = check_chroma(c, ref_frame, w, rgb_depth, up)) || (rc = check_chroma(c, dist_frame, w, rgb_depth, up)))
        return rc;
    if (!out_score) return c->fail(SSIMU2_ERR_INVALID_ARG, "null out_score");
    if (!out_map) return c->fail(SSIMU2_ERR_INVALID_ARG, "null out_map");
    ChromaAux ra, da;
    return map_pair(c, chroma_feed(*ref_frame, w, h, rgb_depth, up, &ra), chroma_feed(*dist_frame, w, h, rgb_depth, up, &da),
                    w, h, out_map, out_score);
}

int ssimu2_error_map_against_reference_yuv_chroma(ssimu2_ctx* c, const ssimu2_yuv_frame* frame, uint32_t rgb_depth,
                                                  uint32_t chroma_upsampling, float* out_map, double* out_score) {
    REMOTE_REFUSE(c, "ssimu2_error_map_against_reference_yuv_chroma");
    int rc = check_against(c, frame && out_score && out_map);
    if (rc || (rc = check_chroma(c, frame, c->ref.w, rgb_depth, chroma_upsampling))) return rc;
    ChromaAux aux;
    return map_against(c, chroma_feed(*frame, c->ref.w, c->ref.h, rgb_depth, chroma_upsampling, &aux), out_map, out_score);
}

}  // extern "C"
