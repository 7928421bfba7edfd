/* Batches of 16-bit and YUV frames in the recursive blur modes of the MI355X SSIMULACRA2 scorer: n frames of one size
   -- tight RGB16 frames of 8 to 16 bits, or a decoder's Y, U and V planes -- scored with a fixed number of launches
   whatever n is, in SSIMU2_BLUR_RECURSIVE and SSIMU2_BLUR_RECURSIVE_FMA, the published operation order (DESIGN.md
   section 19).  The probes of one speculative search are such a batch: n decodes of one image against one cached
   reference.

   These functions live in liboavif_hip_hbatch.so, which is liboavif_hip_rbatch.so -- the same objects, the same
   kernels, every function of the eight headers below it -- plus the six below.  The other eight libraries have none of
   them and export what they exported.

   The batch is ssimu2_hip_rbatch.h's with another front end: one conversion launch (k_pyramid_bands_xyb16_batch; a YUV
   batch has one launch in front of it that makes the codes of all n frames), one horizontal and one vertical pass (the
   pair form: two and two, the references' first) and one final reduction for the whole batch.  The contract:
   item i's score and its 108 averages (ssimu2_last_batch_averages, which serves these batches too) have THE BITS OF
   THE SINGLE SCORE of that item in the context's blur mode --
     ssimu2_hbatch_score_rgb16[_device]                    ssimu2_score_rgb16(..., 3, bit_depth, ...)
     ssimu2_hbatch_score_against_reference_rgb16[_device]  ssimu2_score_against_reference_rgb16
     ssimu2_hbatch_score_against_reference_yuv             ssimu2_score_against_reference_yuv_chroma
   -- so a YUV batch has the bits of the rgb16 batch on its converted codes, and item i's block of
   ssimu2_hbatch_convert_yuv has the bits of ssimu2_convert_yuv_chroma on frame i.  n, an item's place and its
   neighbours never enter its arithmetic.  Samples above 2^bit_depth - 1 are read as that code.

   SSIMU2_BLUR_FIR: the five scoring calls are SSIMU2_ERR_UNSUPPORTED ("16-bit batches run in the recursive modes
   only": the FIR batch's marching kernel reads 8-bit frames).  ssimu2_hbatch_convert_yuv works in any mode.

   One kind of frame per YUV batch: every frame has frame 0's depth, format, full_range and matrix_coefficients;
   one that differs is SSIMU2_ERR_INVALID_ARG ("score mixed frames one by one").  Plane pointers and row_bytes are
   per frame, at any alignment ssimu2_score_against_reference_yuv_chroma takes; each frame is checked as that call
   checks it, with its refusals.  No alpha plane.

   Refusals, in this order: a null context (SSIMU2_ERR_INVALID_ARG); n == 0 is SSIMU2_OK and touches nothing;
   SSIMU2_ERR_NO_REFERENCE for the against-reference forms without a reference (ssimu2_ctx_set_blur drops it);
   SSIMU2_ERR_INVALID_ARG for n > SSIMU2_MAX_BATCH; SSIMU2_ERR_UNSUPPORTED in SSIMU2_BLUR_FIR (the scoring calls) --
   then SSIMU2_ERR_INVALID_ARG for a null array, a zero dimension, null out_scores, a null or odd item pointer,
   item_stride_bytes below one frame (6 * w * h) or odd, and SSIMU2_ERR_UNSUPPORTED for bit_depth or rgb_depth outside
   8..16 -- then SSIMU2_ERR_INVALID_ARG for an item above 2^28 pixels and for a batch whose grids or job count exceed
   2^31 - 1 ("fewer items per call"), both in every form before anything is allocated or copied.  SSIMU2_ERR_OOM when
   the batch's scratch cannot grow: the context stays usable, a smaller batch may fit.  SSIMU2_ERR_UNSUPPORTED from a
   context that lives in a scoring service (all six calls).  Frames below 8 x 8 score 100.0 with zero averages.

   A batch leaves the blur mode, a cached reference (the pair form too), the result of ssimu2_last_averages, a pending
   enqueued score and the bits of every later single score and error map of the context, 8-bit or 16-bit, as they
   were.  All six calls block: every copy out of the caller's memory is enqueued before the first kernel, and the call
   returns after the stream has drained, so the caller may free its frames after any return.

   Device memory: all of it is the batch's own, allocated by the first such call, grown on demand and freed by
   ssimu2_ctx_destroy; a context that never makes one of these calls allocates none of it.  On top of
   ssimu2_hip_rbatch.h's planes (per item 21 fp32 planes of the sum over the scales of pitch * h floats, 12 in the
   against-reference forms, and the partial sums), per item: 6 * w * h bytes of staged frames per side in the host
   rgb16 forms (nothing in the _device forms); in the YUV forms 6 * w * h bytes of codes and the staged planes, rows
   tight -- w * h samples of Y and, unless 4:0:0, two chroma planes of cw * ch samples (1 byte each at depth 8, else
   2) -- each plane and item rounded up to 16 bytes.  880 bytes of page-locked host memory per item. */
#ifndef SSIMU2_HIP_HBATCH_H_
#define SSIMU2_HIP_HBATCH_H_

#include "ssimu2_hip_rbatch.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default) /* the library is built with -fvisibility=hidden */
#endif

/* refs[i] / dists[i]: n host frames each, tight RGB16 (3 channels, samples of `bit_depth` 8..16 in the low bits), as
   ssimu2_score_rgb16 takes them. */
int ssimu2_hbatch_score_rgb16(ssimu2_ctx* ctx, const uint16_t* const* refs, const uint16_t* const* dists, uint32_t n,
                              uint32_t w, uint32_t h, uint32_t bit_depth, double* out_scores);
/* dists[i] against the cached reference, whichever call set it (kept cached). */
int ssimu2_hbatch_score_against_reference_rgb16(ssimu2_ctx* ctx, const uint16_t* const* dists, uint32_t n,
                                                uint32_t bit_depth, double* out_scores);
/* The frames already on the context's device: item i at base + i * item_stride_bytes (even, >= 6 * w * h; the front
   end needs 2-byte alignment only). */
int ssimu2_hbatch_score_rgb16_device(ssimu2_ctx* ctx, const void* d_refs, const void* d_dists, size_t item_stride_bytes,
                                     uint32_t n, uint32_t w, uint32_t h, uint32_t bit_depth, double* out_scores);
int ssimu2_hbatch_score_against_reference_rgb16_device(ssimu2_ctx* ctx, const void* d_dists, size_t item_stride_bytes,
                                                       uint32_t n, uint32_t bit_depth, double* out_scores);
/* n decoded frames (host planes, any of the four formats, no alpha plane) against the cached reference, whichever
   call set it. */
int ssimu2_hbatch_score_against_reference_yuv(ssimu2_ctx* ctx, const ssimu2_yuv_frame* frames, uint32_t n,
                                              uint32_t rgb_depth, uint32_t chroma_upsampling, double* out_scores);
/* The n frames as the scorer sees them: n * w * h * 3 codes, item after item (a diagnostic, like
   ssimu2_convert_yuv_chroma). */
int ssimu2_hbatch_convert_yuv(ssimu2_ctx* ctx, const ssimu2_yuv_frame* frames, uint32_t n, uint32_t w, uint32_t h,
                              uint32_t rgb_depth, uint32_t chroma_upsampling, uint16_t* out_codes);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* SSIMU2_HIP_HBATCH_H_ */
