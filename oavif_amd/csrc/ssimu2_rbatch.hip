// Batches in every blur mode of the MI355X SSIMULACRA2 scorer: the entry points of include/ssimu2_hip_rbatch.h
// (DESIGN.md section 18).
//
// A translation unit of its own over ssimu2_host.h: four functions that check their arguments as their
// ssimu2_score_batch_* counterparts do -- the same refusals in the same order, without the blur-mode check and with
// the recursive modes' size limit per item behind them -- and hand over to rbatch_run, which is ssimu2_hip.hip's:
// the FIR batch as it is, or the batch of the recursive modes.  No kernel lives here: the recursion's kernels need the
// scorer unit's constants and expressions, of which a library holds one copy.  Its object is linked with the YUVA
// library's objects into liboavif_hip_rbatch.so; the other seven libraries contain none of this, and their exports
// are what they were.
#include "../../include/ssimu2_hip_rbatch.h"
#include "ssimu2_host.h"

using namespace ssimu2h;

extern "C" {

int ssimu2_rbatch_score_rgb8_device(ssimu2_ctx* c, const void* d_refs, const void* d_dists, size_t item_stride_bytes,
                                    uint32_t n, uint32_t w, uint32_t h, double* out_scores) {
    REMOTE_REFUSE(c, "ssimu2_rbatch_score_rgb8_device");
    int rc = rbatch_open(c, n, false);
    if (rc || n == 0) return rc;
    if ((rc = check_args(c, d_refs, d_dists, w, h))) return rc;
    if (!out_scores) return c->fail(SSIMU2_ERR_INVALID_ARG, "null out_scores");
    if ((uint64_t)item_stride_bytes < (uint64_t)w * h * 3)
        return c->fail(SSIMU2_ERR_INVALID_ARG, "item_stride_bytes smaller than one frame");
    if ((rc = rbatch_check_size(c, w, h))) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    return rbatch_run(c, (const uint8_t*)d_refs, (const uint8_t*)d_dists, item_stride_bytes, n, w, h, out_scores);
}

int ssimu2_rbatch_score_against_reference_device(ssimu2_ctx* c, const void* d_dists, size_t item_stride_bytes, uint32_t n,
                                                 double* out_scores) {
    REMOTE_REFUSE(c, "ssimu2_rbatch_score_against_reference_device");
    int rc = rbatch_open(c, n, true);
    if (rc || n == 0) return rc;
    if (!d_dists || !out_scores) return c->fail(SSIMU2_ERR_INVALID_ARG, "null pointer");
    if ((uint64_t)item_stride_bytes < (uint64_t)c->ref.w * c->ref.h * 3)
        return c->fail(SSIMU2_ERR_INVALID_ARG, "item_stride_bytes smaller than one frame");
    if ((rc = rbatch_check_size(c, c->ref.w, c->ref.h))) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    return rbatch_run(c, nullptr, (const uint8_t*)d_dists, item_stride_bytes, n, c->ref.w, c->ref.h, out_scores);
}

int ssimu2_rbatch_score_rgb8(ssimu2_ctx* c, const uint8_t* const* refs, const uint8_t* const* dists, uint32_t n, uint32_t w,
                             uint32_t h, double* out_scores) {
    REMOTE_REFUSE(c, "ssimu2_rbatch_score_rgb8");
    int rc = rbatch_open(c, n, false);
    if (rc || n == 0) return rc;
    if ((rc = check_args(c, refs, dists, w, h))) return rc;
    if (!out_scores) return c->fail(SSIMU2_ERR_INVALID_ARG, "null out_scores");
    for (uint32_t i = 0; i < n; ++i)
        if (!refs[i] || !dists[i]) return c->fail(SSIMU2_ERR_INVALID_ARG, "null image pointer in the batch");
    if ((rc = rbatch_check_size(c, w, h))) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t bytes = (size_t)w * h * 3, stride = (bytes + 15) & ~(size_t)15;
    const uint8_t *d_refs, *d_dists;
    if (!(rc = rbatch_stage(c, true, refs, n, bytes, stride, &d_refs)) &&
        !(rc = rbatch_stage(c, false, dists, n, bytes, stride, &d_dists)))
        rc = rbatch_run(c, d_refs, d_dists, stride, n, w, h, out_scores);
    return leave(c, rc);
}

int ssimu2_rbatch_score_against_reference(ssimu2_ctx* c, const uint8_t* const* dists, uint32_t n, double* out_scores) {
    REMOTE_REFUSE(c, "ssimu2_rbatch_score_against_reference");
    int rc = rbatch_open(c, n, true);
    if (rc || n == 0) return rc;
    if (!dists || !out_scores) return c->fail(SSIMU2_ERR_INVALID_ARG, "null pointer");
    for (uint32_t i = 0; i < n; ++i)
        if (!dists[i]) return c->fail(SSIMU2_ERR_INVALID_ARG, "null image pointer in the batch");
    if ((rc = rbatch_check_size(c, c->ref.w, c->ref.h))) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t bytes = (size_t)c->ref.w * c->ref.h * 3, stride = (bytes + 15) & ~(size_t)15;
    const uint8_t* d_dists;
    if (!(rc = rbatch_stage(c, false, dists, n, bytes, stride, &d_dists)))
        rc = rbatch_run(c, nullptr, d_dists, stride, n, c->ref.w, c->ref.h, out_scores);
    return leave(c, rc);
}

}  // extern "C"
