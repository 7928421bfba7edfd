/* YUV input with an alpha plane of the MI355X SSIMULACRA2 scorer: what a decoder leaves of a transparent AVIF -- Y, U
   and V planes plus an alpha plane -- converted, upsampled and composited over an opaque background on the device in one
   pass, then scored as ssimu2_hip_ext.h's RGBA frames are.

   These functions live in liboavif_hip_yuva.so, which is liboavif_hip_chroma.so -- the same objects, the same kernels,
   every function of ssimu2_hip.h, oavif_tq.h, ssimu2_hip_ext.h, ssimu2_hip_yuv.h, ssimu2_hip_map.h and
   ssimu2_hip_chroma.h -- plus the six below.  The other six libraries have none of them.

   Definition (the library's own, exact).  A frame is an ssimu2_yuv_frame of any of the four formats plus an alpha plane
   of w x h samples of the frame's own `depth`: the sample type of Y (one byte at depth 8, two above), rows
   alpha_row_bytes apart.  Alpha is straight (not premultiplied) and full range; with ma = 2^depth - 1 a sample above
   ma is read as ma, and a null alpha pointer means an opaque frame, a = ma everywhere (libavif's image without an
   alpha plane).  For each pixel and channel, c is the colour code of ssimu2_hip_yuv.h / ssimu2_hip_chroma.h at
   rgb_depth, bit for bit; mc = 2^rgb_depth - 1; b is the 8-bit background sample of the channel (background_rgb =
   0xRRGGBB, as in ssimu2_hip_ext.h).  Then, in unsigned integers:
       den = ma * mc                                  (always odd; < 2^28)
       num = a * c * 255 + (ma - a) * b * mc          (<= 255 * den)
       n   = (255 * num + (den - 1) / 2) / den        (floor; 0 <= n <= 65025; 255 * num < 2^44)
   n is the nearest of the 65,026 composite codes to 65025 * (a c / (ma mc) + (1 - a / ma) b / 255), and is read through
   ssimu2_hip_ext.h's table T (ssimu2_alpha_table).  From the linear values on, everything is the existing pipeline in
   the context's blur mode.

   What follows from it:
     - depth 8 and rgb_depth 8: n = a c + (255 - a) b exactly, for all 2^24 (a, c, b).  The frame has the score, the
       averages and the map of ssimu2_score_rgba8 and the other RGBA calls on the RGBA8 frame made of its codes at
       rgb_depth 8 and its alpha plane, bit for bit, in every blur mode and every format.
     - a = 0: n = 255 b.  Colour under full transparency does not enter the result.
     - a = ma: n = round(65025 c / mc).  At rgb_depth 8 that is 255 c, and an opaque or alpha-less frame has the bits of
       ssimu2_score_yuv[_chroma] at rgb_depth 8 (T[255 c] is the 8-bit table's entry c).  At any other rgb_depth it has
       not: the codes are quantised to T's 65,026 levels (mc = 65535 has more codes than T has entries; mc = 1023 and
       4095 do not divide 65025), so the score differs from the opaque calls' in the last digits.
     - different depths: libavif rescales the alpha plane to the RGB depth when the two differ
       (avifImageYUVToRGB); this definition keeps alpha at its own depth, which loses nothing.  So the composite of
       libavif's own RGBA output equals these codes only where depth == rgb_depth (in the tests: 8 and 8).
   Premultiplied alpha is not supported: the struct carries libavif's flag, and a nonzero value is
   SSIMU2_ERR_UNSUPPORTED.

   Each function mirrors one of ssimu2_hip_chroma.h with `background_rgb` added where the RGBA calls have it.  The two
   frames of a pair may differ in format, depth, matrix and in having an alpha plane.  A reference set through
   ssimu2_set_reference_yuva is a high-bit-depth reference that records its background, like one set by
   ssimu2_set_reference_rgba8; either serves ssimu2_score_against_reference_yuva and
   ssimu2_score_against_reference_rgba8 alike -- a search sets the reference from its RGBA8 source and scores the
   decoder's planes against it.
   Errors are those of the mirrored call (check_chroma's), plus SSIMU2_ERR_INVALID_ARG for a background_rgb above
   0xFFFFFF, for alpha_row_bytes below one row of w samples, for an odd alpha pointer or alpha_row_bytes with two-byte
   samples, and from an against-reference call when the reference recorded no background; SSIMU2_ERR_UNSUPPORTED for
   alpha_premultiplied != 0 and from a context that lives in a scoring service.  Device memory of a context that never
   makes one of these calls is unchanged; the first call allocates what the first RGBA call and the first YUV call
   allocate (the staging buffer, the 16-bit frame buffers, the composite table) and nothing else. */
#ifndef SSIMU2_HIP_YUVA_H_
#define SSIMU2_HIP_YUVA_H_

#include "ssimu2_hip_chroma.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default) /* the library is built with -fvisibility=hidden */
#endif

typedef struct ssimu2_yuva_frame {
    ssimu2_yuv_frame yuv;         /* any of formats 1..4 */
    const void* alpha;            /* w x h samples of yuv.depth; NULL = opaque */
    uint32_t alpha_row_bytes;     /* bytes between alpha rows; not looked at when alpha is NULL */
    uint32_t alpha_premultiplied; /* must be 0 */
} ssimu2_yuva_frame;

/* The w * h * 3 composite codes n (0..65025) of one frame: the frame as the scorer sees it (a diagnostic, like
   ssimu2_composite_rgba8).  Leaves a cached reference and the last averages as they were. */
int ssimu2_composite_yuva(ssimu2_ctx* ctx, const ssimu2_yuva_frame* frame, uint32_t w, uint32_t h, uint32_t rgb_depth,
                          uint32_t chroma_upsampling, uint32_t background_rgb, uint16_t* out_codes);
/* ssimu2_score_yuv_chroma: the pair score of two frames, both composited over background_rgb. */
int ssimu2_score_yuva(ssimu2_ctx* ctx, const ssimu2_yuva_frame* ref_frame, const ssimu2_yuva_frame* dist_frame, uint32_t w,
                      uint32_t h, uint32_t rgb_depth, uint32_t chroma_upsampling, uint32_t background_rgb, double* out_score);
/* ssimu2_set_reference_yuv_chroma; the reference keeps background_rgb. */
int ssimu2_set_reference_yuva(ssimu2_ctx* ctx, const ssimu2_yuva_frame* frame, uint32_t w, uint32_t h, uint32_t rgb_depth,
                              uint32_t chroma_upsampling, uint32_t background_rgb);
/* ssimu2_score_against_reference_yuv_chroma, over the background of the reference (set by ssimu2_set_reference_yuva or
   ssimu2_set_reference_rgba8; any other reference: SSIMU2_ERR_INVALID_ARG). */
int ssimu2_score_against_reference_yuva(ssimu2_ctx* ctx, const ssimu2_yuva_frame* frame, uint32_t rgb_depth,
                                        uint32_t chroma_upsampling, double* out_score);
/* ssimu2_error_map_yuv_chroma. */
int ssimu2_error_map_yuva(ssimu2_ctx* ctx, const ssimu2_yuva_frame* ref_frame, const ssimu2_yuva_frame* dist_frame, uint32_t w,
                          uint32_t h, uint32_t rgb_depth, uint32_t chroma_upsampling, uint32_t background_rgb, float* out_map,
                          double* out_score);
/* ssimu2_error_map_against_reference_yuv_chroma, over the reference's background. */
int ssimu2_error_map_against_reference_yuva(ssimu2_ctx* ctx, const ssimu2_yuva_frame* frame, uint32_t rgb_depth,
                                            uint32_t chroma_upsampling, float* out_map, double* out_score);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* SSIMU2_HIP_YUVA_H_ */
