/* Batches in every blur mode of the MI355X SSIMULACRA2 scorer: n pairs of one size scored with a fixed number of
   launches whatever n is, in SSIMU2_BLUR_RECURSIVE and SSIMU2_BLUR_RECURSIVE_FMA -- the published operation order --
   as well as in SSIMU2_BLUR_FIR.

   These functions live in liboavif_hip_rbatch.so, which is liboavif_hip_yuva.so -- the same objects, the same kernels,
   every function of the seven headers below it -- plus the four below.  The other seven libraries have none of them,
   and in every library, this one included, the four ssimu2_score_batch_* calls of ssimu2_hip.h are what they were:
   SSIMU2_ERR_UNSUPPORTED in the recursive modes.

   Each function has the parameters of its ssimu2_score_batch_* counterpart (ssimu2_hip.h, "Batch scoring") and scores
   in the context's CURRENT blur mode:
     SSIMU2_BLUR_FIR            the batch of ssimu2_score_batch_*, through the same code: the same bits.
     SSIMU2_BLUR_RECURSIVE,     one conversion launch, one horizontal and one vertical pass (the pair form: two and two,
     SSIMU2_BLUR_RECURSIVE_FMA  the references' first) and one final reduction for the whole batch.
   The contract of the recursive modes: item i's score and its 108 averages (ssimu2_last_batch_averages, which serves
   these batches too) have THE BITS OF THE SINGLE SCORE of its pair in that mode -- ssimu2_score_rgb8 for the pair form,
   ssimu2_set_reference + ssimu2_score_against_reference for the against-reference form.  An item keeps the jobs of its
   single score (row groups, column groups, the order of every sum), so nothing is regrouped, and n, the item's place
   and its neighbours never enter its arithmetic.

   Input: 8-bit RGB; n <= SSIMU2_MAX_BATCH.  Contract: n == 0 is SSIMU2_OK and touches nothing.  Refusals, in this
   order, are those of the counterpart without the blur-mode check -- a null context; SSIMU2_ERR_NO_REFERENCE for the
   against-reference forms without a reference (ssimu2_ctx_set_blur drops it); SSIMU2_ERR_INVALID_ARG for n >
   SSIMU2_MAX_BATCH, a null array, a zero dimension, null out_scores, a null item, item_stride_bytes < 3 * w * h --
   then, in the recursive modes, SSIMU2_ERR_INVALID_ARG for an item above 2^28 pixels (before anything is allocated)
   and for a batch whose grids or job count exceed 2^31 - 1 ("fewer items per call").  SSIMU2_ERR_OOM when the batch's
   scratch cannot grow: the context stays usable, a smaller batch may fit.  SSIMU2_ERR_UNSUPPORTED from a context that
   lives in a scoring service (all four calls).  Frames below 8 x 8 score 100.0 with zero averages.

   A batch leaves the blur mode, a cached reference (the pair form too), the result of ssimu2_last_averages, a pending
   enqueued score and the bits of every later single score and error map of the context as they were; the
   against-reference form reads the cached reference's planes and writes none of them.
   Device memory in the recursive modes, allocated by the first such batch, grown on demand and freed by
   ssimu2_ctx_destroy: per item 21 fp32 planes of the sum over the scales of pitch * h floats (pitch: w rounded up to
   128) -- 12 in the against-reference form --, the partial sums, and in the host-pointer forms the staged frames; 880
   bytes of page-locked host memory per item.  A context that never makes such a batch allocates none of it. */
#ifndef SSIMU2_HIP_RBATCH_H_
#define SSIMU2_HIP_RBATCH_H_

#include "ssimu2_hip_yuva.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default) /* the library is built with -fvisibility=hidden */
#endif

/* ssimu2_score_batch_rgb8 in the context's blur mode: refs[i] / dists[i], n host frames each (tight RGB8). */
int ssimu2_rbatch_score_rgb8(ssimu2_ctx* ctx, const uint8_t* const* refs, const uint8_t* const* dists, uint32_t n,
                             uint32_t w, uint32_t h, double* out_scores);
/* ssimu2_score_batch_against_reference: dists[i] against the reference of ssimu2_set_reference (kept cached). */
int ssimu2_rbatch_score_against_reference(ssimu2_ctx* ctx, const uint8_t* const* dists, uint32_t n, double* out_scores);
/* The frames already on the context's device: item i at d_refs + i * item_stride_bytes, d_dists + i * item_stride_bytes. */
int ssimu2_rbatch_score_rgb8_device(ssimu2_ctx* ctx, const void* d_refs, const void* d_dists, size_t item_stride_bytes,
                                    uint32_t n, uint32_t w, uint32_t h, double* out_scores);
int ssimu2_rbatch_score_against_reference_device(ssimu2_ctx* ctx, const void* d_dists, size_t item_stride_bytes,
                                                 uint32_t n, double* out_scores);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* SSIMU2_HIP_RBATCH_H_ */
