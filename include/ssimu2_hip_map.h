/* Error maps of 16-bit, RGBA and YUV frames on the MI355X SSIMULACRA2 scorer: where a frame is damaged, in the units
   of the score, for every kind of input the scorer takes and in every blur mode.

   These functions live in liboavif_hip_map.so, which is liboavif_hip_yuv.so -- the same objects, the same kernels,
   every function of ssimu2_hip.h, oavif_tq.h, ssimu2_hip_ext.h and ssimu2_hip_yuv.h -- plus the six below.  Of the
   other libraries only liboavif_hip_chroma.so (ssimu2_hip_chroma.h), which is this one plus six more, has them.

   Definition.  The map is the map of ssimu2_hip.h ("Error map"), unchanged: per scale and channel
   the density  sum_k coef_k * term_k  over the six per-pixel terms d, d^4, art, art^4, det, det^4 (one product, then
   five fused multiply-adds in term order), with coef = w for an L1 statistic and w / a^3 (fp64, clamped at 3e38, 0
   when a == 0, rounded once to fp32) for an L4 one, a being that statistic's average in the score just taken; the
   map at (x, y) is the sum over scales s, ascending, of (density_X + density_Y) + density_B at (x >> s, y >> s).  The
   per-pixel terms are those of the 16-bit pipeline on the frame's codes: the codes of ssimu2_score_rgb16 at
   `bit_depth`, the composite codes of ssimu2_hip_ext.h through its table, the converted codes of ssimu2_hip_yuv.h at
   `rgb_depth` through that depth's table; from the linear values on everything is the 8-bit map's arithmetic in the
   context's blur mode.
   Consequences.  A map call is the scoring call of the same input followed by the map pass: the score returned and
   ssimu2_last_averages are bit for bit those of that scoring call; a cached reference and its caches are left as
   that call leaves them (the pair forms drop the reference, the against-reference forms keep it); repeated calls
   give identical bits; the against-reference map is the pair map of the same two frames, bit for bit; the YUV and
   RGBA maps are the rgb16 maps of the codes ssimu2_convert_yuv / ssimu2_composite_rgba8 hand out (RGBA: read through
   the composite table).  The depth-16 map of the codes 257 u, and the RGBA map of opaque frames, is the map
   ssimu2_error_map_rgb8 gives of the 8-bit frames u, bit for bit, in every blur mode (entry 257 u of the depth-16
   table and entry 255 u of the composite table are the 8-bit entry u: ssimu2_hip.h, ssimu2_hip_ext.h).  A frame
   below 8 x 8 has no scale: the map is zero and the score 100.

   Arguments, row rules and error codes are those of the scoring call of the same input, word for word
   (ssimu2_score_rgb16 with channels = 3, ssimu2_score_against_reference_rgb16, ssimu2_score_rgba8,
   ssimu2_score_against_reference_rgba8, ssimu2_score_yuv, ssimu2_score_against_reference_yuv), and a null `out_map`
   is SSIMU2_ERR_INVALID_ARG like a null `out_score`.  `out_map` receives w * h floats, row-major.  The
   against-reference forms work against a reference set by any set-reference call -- 8-bit, 16-bit, RGBA or YUV --
   as the scoring calls do, with their refusals: no reference, no recorded background for the RGBA form, the recursive
   modes' limits, and against a FIR reference whose cached planes are missing what
   ssimu2_score_against_reference_strided16 answers.  SSIMU2_ERR_UNSUPPORTED comes from a context that lives in a
   scoring service (OAVIF_SCORER_SOCKET), whose protocol does not carry these calls.  All calls block.
   Device memory of a context that never makes one of these calls is unchanged.  The first one allocates what the
   scoring call allocates and the map buffers of ssimu2_error_map_rgb8 (20 bytes per pixel, shared with it); in FIR the
   first against-reference map of 16-bit, RGBA or YUV frames against a reference set from 8-bit samples also
   allocates that reference's scale-0 linear planes (12 bytes per pixel) and fills them once per reference. */
#ifndef SSIMU2_HIP_MAP_H_
#define SSIMU2_HIP_MAP_H_

#include "ssimu2_hip_yuv.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default) /* the library is built with -fvisibility=hidden */
#endif

/* Score and map of two tight RGB frames of uint16_t samples of `bit_depth` (8..16) bits. */
int ssimu2_error_map_rgb16(ssimu2_ctx* ctx, const uint16_t* ref, const uint16_t* dist, uint32_t w, uint32_t h,
                           uint32_t bit_depth, float* out_map, double* out_score);
/* The same of one such frame of the reference's size against the cached reference. */
int ssimu2_error_map_against_reference_rgb16(ssimu2_ctx* ctx, const uint16_t* dist, uint32_t bit_depth, float* out_map,
                                             double* out_score);
/* Score and map of two RGBA frames (rows ref_row_bytes / dist_row_bytes apart), each composited over `background_rgb`. */
int ssimu2_error_map_rgba8(ssimu2_ctx* ctx, const uint8_t* ref, uint32_t ref_row_bytes, const uint8_t* dist,
                           uint32_t dist_row_bytes, uint32_t w, uint32_t h, uint32_t background_rgb, float* out_map,
                           double* out_score);
/* The same of one RGBA frame against the reference of ssimu2_set_reference_rgba8, over its background. */
int ssimu2_error_map_against_reference_rgba8(ssimu2_ctx* ctx, const uint8_t* pixels, uint32_t row_bytes, float* out_map,
                                             double* out_score);
/* Score and map of two YUV frames, converted to codes of `rgb_depth` bits. */
int ssimu2_error_map_yuv(ssimu2_ctx* ctx, const ssimu2_yuv_frame* ref_frame, const ssimu2_yuv_frame* dist_frame, uint32_t w,
                         uint32_t h, uint32_t rgb_depth, float* out_map, double* out_score);
/* The same of one YUV frame of the reference's size against the cached reference. */
int ssimu2_error_map_against_reference_yuv(ssimu2_ctx* ctx, const ssimu2_yuv_frame* frame, uint32_t rgb_depth,
                                           float* out_map, double* out_score);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* SSIMU2_HIP_MAP_H_ */
