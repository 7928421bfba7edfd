/* Subsampled YUV input of the MI355X SSIMULACRA2 scorer: 4:2:2 and 4:2:0 frames as a decoder hands them out, their
   chroma upsampled on the device exactly as libavif's built-in converter does it, then converted and scored as
   ssimu2_hip_yuv.h's 4:4:4 frames are.

   These functions live in liboavif_hip_chroma.so, which is liboavif_hip_map.so -- the same objects, the same kernels,
   every function of ssimu2_hip.h, oavif_tq.h, ssimu2_hip_ext.h, ssimu2_hip_yuv.h and ssimu2_hip_map.h -- plus the six
   below.  Of the other libraries only liboavif_hip_yuva.so, built on this one, has them, and the calls of
   ssimu2_hip_yuv.h and ssimu2_hip_map.h go on refusing formats 2 and 3.

   Definition (the library's own, exact; it extends ssimu2_hip_yuv.h's, whose constants and names are used here).
   A subsampled frame's planes 1 and 2 are cw x ch samples:
       cw = (w + 1) / 2;   ch = (h + 1) / 2 for 4:2:0 (format 3, libavif's AVIF_PIXEL_FORMAT_YUV420);
                           ch = h           for 4:2:2 (format 2).
   row_bytes[1..2] must cover cw samples.  With sx = 1, and sy = 1 for 4:2:0 or sy = 0 for 4:2:2:
       unorm(p, r, c) = ((float)min(p[r][c], m) - biasUV) / rangeUV      (ssimu2_hip_yuv.h's constants; correctly rounded)
       ui = i >> 1,  uj = j >> sy
       nearest :  C(i, j) = unorm(p, uj, ui)
       bilinear:  ac =  0 if i == 0 or (i == w - 1 and i odd), else +1 if i odd, else -1
                  ar =  0 if 4:2:2 or j == 0 or (j == h - 1 and j odd), else +1 if j odd, else -1
                  C(i, j) = ((unorm(uj, ui) * 0.5625f + unorm(uj, ui + ac) * 0.1875f)
                             + unorm(uj + ar, ui) * 0.1875f) + unorm(uj + ar, ui + ac) * 0.0625f
   Every product and every sum is rounded once and nothing is contracted; the blend is taken on the normalised floats,
   not on the codes; the summation order is the one written above.  The ac / ar rule is the same as "the neighbour
   index clamped into the plane".  Cb = C of plane 1 and Cr = C of plane 2; Y, R, G, B and the codes are then exactly
   ssimu2_hip_yuv.h's.
   `bilinear` is what libavif 1.x's built-in converter (avifRGBImage.avoidLibYUV = 1) does for
   AVIF_CHROMA_UPSAMPLING_AUTOMATIC, BEST_QUALITY and BILINEAR, `nearest` what it does for FASTEST and NEAREST: the
   codes are that converter's, bit for bit.

   Each function mirrors one of ssimu2_hip_yuv.h or ssimu2_hip_map.h with one more argument, `chroma_upsampling`, and
   takes the same ssimu2_yuv_frame with `format` 1, 2, 3 or 4.  Formats 1 and 4 give the bits of the mirrored call,
   whatever the upsampling.  The two frames of a pair may differ in format, as they may in depth and matrix.  A
   reference set through these calls is a high-bit-depth reference like a YUV one.
   Errors are those of the mirrored call, plus SSIMU2_ERR_INVALID_ARG for a chroma_upsampling above 1 and for chroma
   row_bytes below cw samples; SSIMU2_ERR_UNSUPPORTED for a format outside 1..4, and from a context that lives in a
   scoring service.  Device memory of a context that never makes one of these calls is unchanged; the staged planes of
   a subsampled frame are smaller than a 4:4:4 frame's. */
#ifndef SSIMU2_HIP_CHROMA_H_
#define SSIMU2_HIP_CHROMA_H_

#include "ssimu2_hip_map.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default) /* the library is built with -fvisibility=hidden */
#endif

#define SSIMU2_YUV_422 2 /* libavif's AVIF_PIXEL_FORMAT_YUV422 */
#define SSIMU2_YUV_420 3 /* libavif's AVIF_PIXEL_FORMAT_YUV420 */

#define SSIMU2_CHROMA_BILINEAR 0 /* libavif's AUTOMATIC, BEST_QUALITY and BILINEAR */
#define SSIMU2_CHROMA_NEAREST 1  /* libavif's FASTEST and NEAREST */

/* ssimu2_convert_yuv of a frame of any of the four formats. */
int ssimu2_convert_yuv_chroma(ssimu2_ctx* ctx, const ssimu2_yuv_frame* frame, uint32_t w, uint32_t h, uint32_t rgb_depth,
                              uint32_t chroma_upsampling, uint16_t* out_codes);
/* ssimu2_score_yuv: the pair score of two frames, each with its own format, depth, range and matrix. */
int ssimu2_score_yuv_chroma(ssimu2_ctx* ctx, const ssimu2_yuv_frame* ref_frame, const ssimu2_yuv_frame* dist_frame,
                            uint32_t w, uint32_t h, uint32_t rgb_depth, uint32_t chroma_upsampling, double* out_score);
/* ssimu2_set_reference_yuv. */
int ssimu2_set_reference_yuv_chroma(ssimu2_ctx* ctx, const ssimu2_yuv_frame* frame, uint32_t w, uint32_t h,
                                    uint32_t rgb_depth, uint32_t chroma_upsampling);
/* ssimu2_score_against_reference_yuv, against the reference of any set-reference call. */
int ssimu2_score_against_reference_yuv_chroma(ssimu2_ctx* ctx, const ssimu2_yuv_frame* frame, uint32_t rgb_depth,
                                              uint32_t chroma_upsampling, double* out_score);
/* ssimu2_error_map_yuv. */
int ssimu2_error_map_yuv_chroma(ssimu2_ctx* ctx, const ssimu2_yuv_frame* ref_frame, const ssimu2_yuv_frame* dist_frame,
                                uint32_t w, uint32_t h, uint32_t rgb_depth, uint32_t chroma_upsampling, float* out_map,
                                double* out_score);
/* ssimu2_error_map_against_reference_yuv. */
int ssimu2_error_map_against_reference_yuv_chroma(ssimu2_ctx* ctx, const ssimu2_yuv_frame* frame, uint32_t rgb_depth,
                                                  uint32_t chroma_upsampling, float* out_map, double* out_score);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* SSIMU2_HIP_CHROMA_H_ */
