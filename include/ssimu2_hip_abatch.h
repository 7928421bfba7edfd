/* Batches of frames with transparency in the recursive blur modes of the MI355X SSIMULACRA2 scorer: n frames of one
   size -- a decoder's Y, U, V and alpha planes, or RGBA8 rows as libavif leaves them -- composited over a background
   on the device and scored with a fixed number of launches whatever n is, in SSIMU2_BLUR_RECURSIVE and
   SSIMU2_BLUR_RECURSIVE_FMA.  The probes of one speculative search of an image with an alpha
   plane are such a batch: n decodes against one cached reference.

   These functions live in liboavif_hip_abatch.so, which is liboavif_hip_hbatch.so -- the same objects, the same
   kernels, every function of the nine headers below it -- plus the five below.  The other nine libraries have none of
   them and export what they exported.

   By ssimu2_hip_yuva.h's definition a frame with an alpha plane is the 16-bit frame of its composite codes n
   (0..65025), read through ssimu2_hip_ext.h's table T.  So the batch is ssimu2_hip_hbatch.h's with another front end:
   one launch makes the composite codes of all n frames (k_yuva_batch_to_codes: conversion, chroma upsampling and
   composite at once; k_composite_rgba8_batch for RGBA8 rows, both sides of the pair form in the one launch), then one
   conversion launch, one horizontal and one vertical pass (the pair form: two and two, the references' first) and one
   final reduction for the whole batch.  The contract: item i's score and its 108 averages
   (ssimu2_last_batch_averages, which serves these batches too) have THE BITS OF THE SINGLE SCORE of that item on a
   fresh context in the same blur mode --
     ssimu2_abatch_score_against_reference_yuva    ssimu2_score_against_reference_yuva
     ssimu2_abatch_score_against_reference_rgba8   ssimu2_score_against_reference_rgba8
     ssimu2_abatch_score_rgba8                     ssimu2_score_rgba8
   -- and item i's block of ssimu2_abatch_composite_yuva / ssimu2_abatch_composite_rgba8 has the bits of
   ssimu2_composite_yuva / ssimu2_composite_rgba8 on frame i.  n, an item's place and its neighbours never enter its
   arithmetic.  It follows that a YUVA batch at depth 8 with rgb_depth 8 has the bits of the RGBA8 batch on its colour
   codes and alpha plane.  The division of ssimu2_hip_yuva.h's n is never taken at depth 8 with rgb_depth 8 and by the
   multiply-high form otherwise; OAVIF_YUVA_DIVISION is not read.

   SSIMU2_BLUR_FIR: the three scoring calls are SSIMU2_ERR_UNSUPPORTED; the two composite diagnostics work in any mode.

   One kind of frame per YUVA batch: every frame has frame 0's depth, format, full_range and matrix_coefficients, and
   carries an alpha plane exactly if frame 0 does; one that differs is SSIMU2_ERR_INVALID_ARG ("score mixed frames one
   by one").  A batch whose frames all have a null alpha is allowed: a = 2^depth - 1 everywhere.  Plane pointers and
   row_bytes are per frame; each frame is checked as ssimu2_score_against_reference_yuva checks it, with its refusals
   (premultiplied alpha: SSIMU2_ERR_UNSUPPORTED).  The RGBA8 forms take one row_bytes >= 4 * w for all frames of a
   side.

   Refusals, in this order: a null context (SSIMU2_ERR_INVALID_ARG); n == 0 is SSIMU2_OK and touches nothing;
   SSIMU2_ERR_NO_REFERENCE for the against-reference forms without a reference (ssimu2_ctx_set_blur drops it);
   SSIMU2_ERR_INVALID_ARG for n > SSIMU2_MAX_BATCH; SSIMU2_ERR_UNSUPPORTED in SSIMU2_BLUR_FIR (the scoring calls) --
   then SSIMU2_ERR_INVALID_ARG for a null array, a null item or null output; for a zero dimension; the checks of each
   frame; then the background: SSIMU2_ERR_INVALID_ARG for background_rgb above 0xFFFFFF, and in the against-reference
   forms for a reference that recorded no background (one not set by ssimu2_set_reference_yuva or
   ssimu2_set_reference_rgba8) -- then SSIMU2_ERR_INVALID_ARG for an item above 2^28 pixels and for a batch whose grids
   or job count exceed 2^31 - 1 ("fewer items per call"), both before anything is allocated or copied.  SSIMU2_ERR_OOM
   when the batch's scratch cannot grow: the context stays usable, a smaller batch may fit.  SSIMU2_ERR_UNSUPPORTED
   from a context that lives in a scoring service (all five calls).  Frames below 8 x 8 score 100.0 with zero averages.

   A batch leaves the blur mode, a cached reference (the pair form too, as the other pair batches of the recursive
   modes do), the result of ssimu2_last_averages, and the bits of every later single score and error map of the
   context as they were; the composite diagnostics leave the last batch's averages alone too.  All five calls block: every copy
   out of the caller's memory is enqueued before the first kernel, and the call returns after the stream has drained,
   so the caller may free its frames after any return.

   Device memory: the buffers of ssimu2_hip_hbatch.h's batches and nothing else, allocated by the first such call and
   freed by ssimu2_ctx_destroy; a context that never makes one of these calls allocates none of it.  Per item, on top
   of ssimu2_hip_rbatch.h's planes: 6 * w * h bytes of codes (per side in the pair form) and the staged frame, rows
   tight -- 4 * w * h bytes of RGBA8, or w * h samples of Y, two chroma planes of cw * ch samples unless 4:0:0, and
   w * h samples of alpha if there is an alpha plane (1 byte each at depth 8, else 2) -- each plane and item rounded up
   to 16 bytes.  The composite table T (260,104 bytes) is the context's, as for a single RGBA call. */
#ifndef SSIMU2_HIP_ABATCH_H_
#define SSIMU2_HIP_ABATCH_H_

#include "ssimu2_hip_hbatch.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default) /* the library is built with -fvisibility=hidden */
#endif

/* n decoded frames (host planes, any of the four formats, depth 8 / 10 / 12, all with or all without an alpha plane)
   of the reference's size: each converted to colour codes of rgb_depth bits, upsampled, composited over the
   reference's recorded background and scored against the cached reference (kept). */
int ssimu2_abatch_score_against_reference_yuva(ssimu2_ctx* ctx, const ssimu2_yuva_frame* frames, uint32_t n,
                                               uint32_t rgb_depth, uint32_t chroma_upsampling, double* out_scores);
/* The n frames as the scorer sees them over background_rgb: n * w * h * 3 composite codes, item after item (a
   diagnostic, like ssimu2_composite_yuva). */
int ssimu2_abatch_composite_yuva(ssimu2_ctx* ctx, const ssimu2_yuva_frame* frames, uint32_t n, uint32_t w, uint32_t h,
                                 uint32_t rgb_depth, uint32_t chroma_upsampling, uint32_t background_rgb,
                                 uint16_t* out_codes);
/* frames[i]: n RGBA8 frames of the reference's size, rows row_bytes >= 4 * w apart, each composited over the
   reference's recorded background and scored against the cached reference (kept). */
int ssimu2_abatch_score_against_reference_rgba8(ssimu2_ctx* ctx, const uint8_t* const* frames, uint32_t row_bytes,
                                                uint32_t n, double* out_scores);
/* n pairs of RGBA8 frames, both sides composited over background_rgb. */
int ssimu2_abatch_score_rgba8(ssimu2_ctx* ctx, const uint8_t* const* refs, uint32_t ref_row_bytes,
                              const uint8_t* const* dists, uint32_t dist_row_bytes, uint32_t n, uint32_t w, uint32_t h,
                              uint32_t background_rgb, double* out_scores);
/* The n RGBA8 frames as the scorer sees them over background_rgb: n * w * h * 3 composite codes, item after item (a
   diagnostic, like ssimu2_composite_rgba8). */
int ssimu2_abatch_composite_rgba8(ssimu2_ctx* ctx, const uint8_t* const* frames, uint32_t row_bytes, uint32_t n,
                                  uint32_t w, uint32_t h, uint32_t background_rgb, uint16_t* out_codes);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* SSIMU2_HIP_ABATCH_H_ */
