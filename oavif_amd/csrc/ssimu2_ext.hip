// RGBA input of the MI355X SSIMULACRA2 scorer: the entry points of include/ssimu2_hip_ext.h.
//
// A translation unit of its own: one kernel, one Feed constructor, one check and five functions over ssimu2_host.h, the
// list of what a front end may use of the scorer.  Its object is linked with the product library's objects into
// liboavif_hip_ext.so (and liboavif_hip_yuv.so); liboavif_hip.so and liboavif_hip_instr.so contain none of this, and
// their exports are what they were.
//
// An RGBA frame becomes a u16 frame of exact integer codes n = a * c + (255 - a) * b (k_composite_rgba8) that the
// 16-bit front end reads through a table of its own: Src16{codes, w * 6, 3, T, 65025}.  No pyramid, marching,
// recursive or finalize kernel knows about alpha.  To the host code an RGBA frame is one more Feed (rgba8 below): the
// three shapes of a call -- score_pair, feed_reference, score_against -- are the product's.
#include "../../include/ssimu2_hip_ext.h"
#include "ssimu2_alpha_pixel.h"
#include "ssimu2_host.h"

using namespace ssimu2h;

namespace ssimu2 {

// ---------------------------------------------------------------------------------------------
// RGBA rows `pitch` bytes apart (any alignment) over the background `bg` = 0xRRGGBB -> tight u16 RGB codes.
// A lane takes four pixels of one row: four unaligned dword loads (16 bytes) and six dword stores (24 bytes: a row of
// codes starts 6 * w * y bytes in, 2-byte aligned only); the last w % 4 pixels of a row go sample by sample.  Rows
// beyond gridDim.y are taken in further rounds.  Pure integer arithmetic (n < 2^16), HBM-bound: 10 bytes per pixel.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_composite_rgba8(const uint8_t* __restrict__ src, uint32_t pitch, uint32_t w,
                                                         uint32_t h, uint32_t bg, uint16_t* __restrict__ dst) {
    const uint32_t x0 = (blockIdx.x * 256u + threadIdx.x) * 4u;
    if (x0 >= w) return;
    const uint32_t b[3] = {(bg >> 16) & 0xFFu, (bg >> 8) & 0xFFu, bg & 0xFFu};
    for (uint32_t y = blockIdx.y; y < h; y += gridDim.y) {
        const uint8_t* s = src + (size_t)y * pitch + (size_t)x0 * 4u;
        uint16_t* d = dst + ((size_t)y * w + x0) * 3u;
        if (x0 + 4u <= w) {
            uint32_t px[4];  // LE: R | G << 8 | B << 16 | A << 24
#pragma unroll
            for (int k = 0; k < 4; ++k) __builtin_memcpy(&px[k], s + 4 * k, 4);
            uint32_t n[12];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t a = px[k] >> 24;
#pragma unroll
                for (int c = 0; c < 3; ++c) n[3 * k + c] = composite_code(a, (px[k] >> (8 * c)) & 0xFFu, b[c]);
            }
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                const uint32_t pair = n[2 * k] | (n[2 * k + 1] << 16);
                __builtin_memcpy((uint8_t*)d + 4 * k, &pair, 4);
            }
        } else {
            for (uint32_t i = 0; x0 + i < w; ++i) {
                const uint32_t a = s[4 * i + 3];
#pragma unroll
                for (int c = 0; c < 3; ++c) d[3 * i + c] = (uint16_t)composite_code(a, s[4 * i + c], b[c]);
            }
        }
    }
}

}  // namespace ssimu2

using namespace ssimu2;

namespace {

constexpr uint32_t kAlphaTop = SSIMU2_ALPHA_CODES - 1;  // 65025 = 255 * 255, the largest code

}  // namespace

// Argument checks of the RGBA calls that name a frame size (the ctx may be null).
int ssimu2h::check_rgba(ssimu2_ctx* c, const void* a, const void* b, uint32_t row_bytes_a, uint32_t row_bytes_b,
                        uint32_t w, uint32_t h, uint32_t background_rgb) {
    int rc = check_args(c, a, b, w, h);
    if (rc) return rc;
    if ((uint64_t)row_bytes_a < (uint64_t)w * 4 || (uint64_t)row_bytes_b < (uint64_t)w * 4)
        return c->fail(SSIMU2_ERR_INVALID_ARG, "row_bytes smaller than one row of RGBA pixels");
    if (background_rgb > 0xFFFFFFu) return c->fail(SSIMU2_ERR_INVALID_ARG, "background_rgb is 0xRRGGBB: the upper byte must be 0");
    return SSIMU2_OK;
}

// What an against-reference RGBA call answers to a reference that recorded no background.
int ssimu2h::rgba_no_background(ssimu2_ctx* c) {
    return c->fail(SSIMU2_ERR_INVALID_ARG, "the reference was not set by ssimu2_set_reference_rgba8: no background recorded");
}

namespace {

// RGBA rows in `stage` composited over f.bg -> the tight u16 frame of codes `dst`.
void composite(ssimu2_ctx* c, const Feed& f, uint32_t w, uint32_t h, void* dst) {
    const uint32_t groups = (w + 3) / 4;
    launch(k_composite_rgba8, dim3((groups + 255) / 256, h < 65535u ? h : 65535u), dim3(256), 0, c->stream,
           c->stage.as<uint8_t>(), f.plane[0].row_bytes, w, h, (uint32_t)f.bg, (uint16_t*)dst);
}

}  // namespace

// One RGBA frame in host memory: its rows go through the staging buffer as they are, the front end reads the codes
// through the composite table T (entry n: the 8-bit table's expression at n / 65025; entry 255 u is the 8-bit entry u).
Feed ssimu2h::rgba8_feed(const uint8_t* pixels, uint32_t row_bytes, uint32_t bg) {
    return staged1(pixels, row_bytes, 4u, 1u, kAlphaTop, composite, (int64_t)bg);
}

extern "C" {

int ssimu2_alpha_table(float* out) { return copy_table(SSIMU2_ALPHA_CODES, kAlphaTop, out); }

int ssimu2_composite_rgba8(ssimu2_ctx* c, const uint8_t* pixels, uint32_t row_bytes, uint32_t w, uint32_t h,
                           uint32_t background_rgb, uint16_t* out_codes) {
    REMOTE_REFUSE(c, "ssimu2_composite_rgba8");
    const int rc = check_rgba(c, pixels, out_codes, row_bytes, row_bytes, w, h, background_rgb);
    if (rc) return rc;
    return feed_codes(c, rgba8_feed(pixels, row_bytes, background_rgb), w, h, out_codes, "ssimu2_composite_rgba8");
}

int ssimu2_score_rgba8(ssimu2_ctx* c, const uint8_t* ref, uint32_t ref_row_bytes, const uint8_t* dist,
                       uint32_t dist_row_bytes, uint32_t w, uint32_t h, uint32_t background_rgb, double* out_score) {
    REMOTE_REFUSE(c, "ssimu2_score_rgba8");
    const int rc = check_rgba(c, ref, dist, ref_row_bytes, dist_row_bytes, w, h, background_rgb);
    if (rc) return rc;
    if (!out_score) return c->fail(SSIMU2_ERR_INVALID_ARG, "null out_score");
    const uint32_t bg = background_rgb;
    return score_pair(c, rgba8_feed(ref, ref_row_bytes, bg), rgba8_feed(dist, dist_row_bytes, bg), w, h, out_score);
}

int ssimu2_set_reference_rgba8(ssimu2_ctx* c, const uint8_t* ref, uint32_t row_bytes, uint32_t w, uint32_t h,
                               uint32_t background_rgb) {
    REMOTE_REFUSE(c, "ssimu2_set_reference_rgba8");
    const int rc = check_rgba(c, ref, ref, row_bytes, row_bytes, w, h, background_rgb);
    return rc ? rc : feed_reference(c, rgba8_feed(ref, row_bytes, background_rgb), w, h);
}

int ssimu2_score_against_reference_rgba8(ssimu2_ctx* c, const uint8_t* pixels, uint32_t row_bytes, double* out_score) {
    REMOTE_REFUSE(c, "ssimu2_score_against_reference_rgba8");
    const int rc = check_against(c, pixels && out_score);
    if (rc) return rc;
    if (c->ref.bg < 0) return rgba_no_background(c);
    if ((uint64_t)row_bytes < (uint64_t)c->ref.w * 4)
        return c->fail(SSIMU2_ERR_INVALID_ARG, "row_bytes smaller than one row of RGBA pixels");
    return score_against(c, rgba8_feed(pixels, row_bytes, (uint32_t)c->ref.bg), out_score);
}

}  // extern "C"
