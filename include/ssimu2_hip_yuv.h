/* YUV input of the MI355X SSIMULACRA2 scorer: a decoder's Y, U and V planes as they are, converted to RGB codes on
   the device with the exact colour matrix and then scored.

   These functions live in liboavif_hip_yuv.so, which is liboavif_hip_ext.so -- the same sources, the same kernels,
   every function of ssimu2_hip.h, oavif_tq.h and ssimu2_hip_ext.h -- plus the four below.  The other three libraries
   have none of them.

   Definition (the library's own, exact, so that a CPU restatement can be held against it).
   A frame is up to three planes of one sample per pixel, each with its own pointer and row_bytes, of `depth` 8, 10 or
   12 bits: uint8_t samples at depth 8, else uint16_t with the value in the low bits (little endian; a sample above
   m = 2^depth - 1 is read as m).  `format` is 4:4:4 or 4:0:0 (monochrome: planes 1 and 2 are not looked at),
   `full_range` 0 or 1, `matrix_coefficients` the CICP code:
       1 -> (kr, kb) = (0.2126f, 0.0722f);   5, 6 and 2 (unspecified) -> (0.299f, 0.114f);   9 -> (0.2627f, 0.0593f).
   All arithmetic is fp32, each operation rounded once, nothing contracted:
       kg = (1 - kr) - kb
       full range:     biasY = 0,                  rangeY = m,                   biasUV = 2^(depth-1),  rangeUV = m
       limited range:  biasY = 16 * 2^(depth-8),   rangeY = 219 * 2^(depth-8),   biasUV = 2^(depth-1),  rangeUV = 224 * 2^(depth-8)
       Y  = ((float)y - biasY) / rangeY     Cb = ((float)u - biasUV) / rangeUV     Cr = ((float)v - biasUV) / rangeUV
            (correctly rounded divisions; not clamped here: limited-range codes outside the nominal range go through;
             4:0:0: Cb = Cr = 0)
       R  = Y + (2 * (1 - kr)) * Cr
       B  = Y + (2 * (1 - kb)) * Cb
       G  = Y - (2 * ((kr * (1 - kr)) * Cr + (kb * (1 - kb)) * Cb)) / kg           (a division by kg)
       code_c = (unsigned)(0.5f + clamp(c, 0, 1) * (float)(2^rgb_depth - 1))       for c = R, G, B
   `rgb_depth` is 8..16, the caller's choice: 16 is full precision, 8 and the frame's own depth make the result
   comparable with libavif's RGB output.  The codes are read through the table of that depth (ssimu2_linear_table); from
   the linear values on everything is the 16-bit pipeline in the context's blur mode, same operations in the same order.
   Consequences: the codes are those of libavif 1.x's built-in converter (avifRGBImage.avoidLibYUV = 1) bit for bit;
   the score of a YUV frame is the score of the 16-bit call of depth rgb_depth on its codes, bit for bit, in every blur
   mode; a full-range 8-bit frame with U = V = 128 everywhere has the codes Y at rgb_depth 8 and 257 Y at rgb_depth 16,
   so either way the score and averages of ssimu2_score_rgb8 on the grey RGB frame, bit for bit (entry 257 u of the
   depth-16 table is the 8-bit entry u: ssimu2_hip.h); the codes are non-decreasing in Y at fixed chroma.

   Rows are `row_bytes` apart, at any alignment (2-byte aligned for 16-bit samples); padding is skipped.  All calls
   block; ssimu2_last_averages works after them.  A reference set from YUV counts as a high-bit-depth reference: the
   8-bit and 16-bit against-reference calls work against it, ssimu2_error_map_against_reference refuses it.
   Errors: SSIMU2_ERR_INVALID_ARG for a null context, frame, needed plane or output, a zero size, row_bytes below one
   row of samples, an odd pointer or row_bytes with 16-bit samples, full_range above 1; SSIMU2_ERR_UNSUPPORTED for a
   depth other than 8, 10, 12, an rgb_depth outside 8..16, a format other than 4:4:4 and 4:0:0, a matrix code outside
   {1, 2, 5, 6, 9}, and from a context that lives in a scoring service (OAVIF_SCORER_SOCKET), whose protocol does not
   carry these calls; SSIMU2_ERR_NO_REFERENCE and the recursive modes' 2^28-pixel limit as for the other calls; against
   a FIR reference whose cached planes are missing, what ssimu2_score_against_reference_strided16 answers.
   Device memory of a context that never makes one of these calls is unchanged.  The first one allocates what a 16-bit
   call of depth rgb_depth allocates, and the staged planes. */
#ifndef SSIMU2_HIP_YUV_H_
#define SSIMU2_HIP_YUV_H_

#include "ssimu2_hip_ext.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default) /* the library is built with -fvisibility=hidden */
#endif

#define SSIMU2_YUV_444 1 /* libavif's AVIF_PIXEL_FORMAT_YUV444 */
#define SSIMU2_YUV_400 4 /* libavif's AVIF_PIXEL_FORMAT_YUV400 */

typedef struct ssimu2_yuv_frame {
    const void* planes[3];        /* Y, U, V: libavif's avifImage.yuvPlanes as they are */
    uint32_t row_bytes[3];        /* avifImage.yuvRowBytes */
    uint32_t depth;               /* 8, 10 or 12 */
    uint32_t format;              /* SSIMU2_YUV_444 or SSIMU2_YUV_400 */
    uint32_t full_range;          /* 0: limited, 1: full */
    uint32_t matrix_coefficients; /* CICP: 1, 2, 5, 6 or 9 */
} ssimu2_yuv_frame;

/* The frame as the scorer sees it: w * h * 3 codes of depth rgb_depth, tight RGB rows, into `out_codes`.  A cached
   reference and the averages of the last score stay as they were. */
int ssimu2_convert_yuv(ssimu2_ctx* ctx, const ssimu2_yuv_frame* frame, uint32_t w, uint32_t h, uint32_t rgb_depth,
                       uint16_t* out_codes);
/* The pair score of two YUV frames (each with its own depth, range and matrix).  Drops a cached reference, as
   ssimu2_score_rgb8 does. */
int ssimu2_score_yuv(ssimu2_ctx* ctx, const ssimu2_yuv_frame* ref_frame, const ssimu2_yuv_frame* dist_frame, uint32_t w,
                     uint32_t h, uint32_t rgb_depth, double* out_score);
/* Cache the converted reference (what ssimu2_set_reference_rgb16 caches). */
int ssimu2_set_reference_yuv(ssimu2_ctx* ctx, const ssimu2_yuv_frame* frame, uint32_t w, uint32_t h, uint32_t rgb_depth);
/* A YUV frame of the reference's size against the reference, whichever call set it: 8-bit, 16-bit, RGBA or YUV. */
int ssimu2_score_against_reference_yuv(ssimu2_ctx* ctx, const ssimu2_yuv_frame* frame, uint32_t rgb_depth,
                                       double* out_score);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* SSIMU2_HIP_YUV_H_ */
