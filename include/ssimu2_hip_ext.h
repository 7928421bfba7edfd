/* Extension entry points of the MI355X SSIMULACRA2 scorer: 8-bit RGBA frames, composited over an opaque background
   on the device and then scored.

   These functions live in liboavif_hip_ext.so, which is liboavif_hip.so -- the same sources, the same kernels, every
   function of ssimu2_hip.h and oavif_tq.h -- plus the five below.  The two public headers and the product library are
   a frozen ABI; a caller that scores transparent images links the extension library instead and includes this header.

   Definition (the library's own, exact, so that a CPU restatement can be held against it).
   Samples are 8-bit RGBA with straight (non-premultiplied) alpha: what oavif_png_decode returns, and what libavif's
   avifRGBImage holds when the image has an alpha plane.  The background is an opaque 8-bit colour (bR, bG, bB),
   passed as 0xRRGGBB.  Per pixel and colour channel the composite code is the integer
       n = a * c + (255 - a) * b,      0 <= n <= 65025,
   the blend done on the sRGB-encoded samples, as a browser composites; every code occurs for some (a, c, b).  Its
   linear value is
       T[n] = (float)(v <= 0.04045 ? v / 12.92 : pow((v + 0.055) / 1.055, 2.4)),   v = (double)n / 65025.0,
   the 8-bit table's expression in fp64, rounded once (SSIMU2_ALPHA_CODES entries).  From the linear values on
   everything is the existing pipeline in the context's blur mode, same operations in the same order.  Each frame is
   composited with its own alpha over the same background.
   Consequences: T[255 u] is the 8-bit table's entry u bit for bit (255 u / 65025 and u / 255 are the same double), so
   a frame with a = 255 everywhere -- or whose colour equals the background wherever a < 255 -- has the score and
   averages of ssimu2_score_rgb8 on its RGB, bit for bit, in every blur mode; where a = 0 the colour bytes do not
   enter the result; T is non-decreasing and its entries are distinct.

   Rows are `row_bytes` apart, at any alignment; padding is skipped.  All calls block; ssimu2_last_averages works
   after them.  A reference set from RGBA counts as a high-bit-depth reference: the 8-bit and 16-bit against-reference
   calls work against it, ssimu2_error_map_against_reference refuses it (SSIMU2_ERR_UNSUPPORTED).
   ssimu2_score_against_reference_rgba8 composites over the background the reference was set with; against a
   reference set by another call, which recorded none, it returns SSIMU2_ERR_INVALID_ARG.
   Errors: SSIMU2_ERR_INVALID_ARG for a null pointer, a zero size, row_bytes below 4 * w, a background above
   0xFFFFFF; SSIMU2_ERR_NO_REFERENCE as the other against-reference calls; the recursive modes' 2^28-pixel limit;
   SSIMU2_ERR_UNSUPPORTED from a context that lives in a scoring service (OAVIF_SCORER_SOCKET), whose protocol does
   not carry these calls.
   Device memory of a context that never makes one of these calls is unchanged.  The first one allocates the table
   (254 KB) and what a 16-bit call allocates except the 16-bit tables: the staged RGBA rows, the composited frames
   (6 bytes per pixel each) and in the FIR mode their scale-0 linear planes (12 bytes per pixel each).  All are
   freed by ssimu2_ctx_destroy. */
#ifndef SSIMU2_HIP_EXT_H_
#define SSIMU2_HIP_EXT_H_

#include "ssimu2_hip.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default) /* the library is built with -fvisibility=hidden */
#endif

#define SSIMU2_ALPHA_CODES 65026

/* The SSIMU2_ALPHA_CODES entries of T (no device or context needed). */
int ssimu2_alpha_table(float* out);
/* The frame as the scorer sees it: w * h * 3 codes n, tight RGB rows, into `out_codes`.  A cached reference and the
   averages of the last score stay as they were. */
int ssimu2_composite_rgba8(ssimu2_ctx* ctx, const uint8_t* pixels, uint32_t row_bytes, uint32_t w, uint32_t h,
                           uint32_t background_rgb, uint16_t* out_codes);
/* The pair score of two RGBA frames, each composited over `background_rgb`.  Drops a cached reference, as
   ssimu2_score_rgb8 does. */
int ssimu2_score_rgba8(ssimu2_ctx* ctx, const uint8_t* ref, uint32_t ref_row_bytes, const uint8_t* dist,
                       uint32_t dist_row_bytes, uint32_t w, uint32_t h, uint32_t background_rgb, double* out_score);
/* Cache the composited reference (what ssimu2_set_reference_rgb16 caches) and record its background. */
int ssimu2_set_reference_rgba8(ssimu2_ctx* ctx, const uint8_t* ref, uint32_t row_bytes, uint32_t w, uint32_t h,
                               uint32_t background_rgb);
/* An RGBA frame of the reference's size, composited over the reference's background, against it.  `pixels` /
   `row_bytes` are libavif's rgb.pixels / rgb.rowBytes as they are. */
int ssimu2_score_against_reference_rgba8(ssimu2_ctx* ctx, const uint8_t* pixels, uint32_t row_bytes, double* out_score);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* SSIMU2_HIP_EXT_H_ */
