// Measurement and parity hooks of the MI355X SSIMULACRA2 scorer -- NOT part of the product.
//
// This translation unit is the product translation unit (ssimu2_hip.hip, included below: same
// kernels, same host code, same flags) plus the entry points of include/ssimu2_hip_internal.h.
// It is built into liboavif_hip_instr.so, which only bench.py, scripts/ and a few tests load;
// liboavif_hip.so -- what a caller links -- contains none of this.
#define SSIMU2_INSTRUMENTED_BUILD 1
#include "ssimu2_hip.hip"

#include <vector>

#include "../../include/ssimu2_hip_internal.h"

namespace ssimu2 {

// ---------------------------------------------------------------------------------------------
// Read-stream probe (ssimu2_measure_read_stream): every lane reads 16 bytes per step, four steps
// in flight; the xor of everything read is stored only if it is a value the zeroed
// buffer cannot produce, so the loads are kept and nothing is written.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_read_stream(const uint4* __restrict__ src, size_t n16,
                                                     uint32_t* __restrict__ sink) {
    // one contiguous chunk per workgroup (whole DRAM pages per workgroup), lanes 16 B apart
    const size_t chunk = (n16 + gridDim.x - 1) / gridDim.x;
    const size_t lo = (size_t)blockIdx.x * chunk;
    const size_t hi = lo + chunk < n16 ? lo + chunk : n16;
    size_t i = lo + threadIdx.x;
    uint4 acc = make_uint4(0, 0, 0, 0);
    for (; i + 768 < hi; i += 1024) {
        const uint4 a = src[i], b = src[i + 256], c = src[i + 512], d = src[i + 768];
        acc.x ^= a.x ^ b.x ^ c.x ^ d.x;
        acc.y ^= a.y ^ b.y ^ c.y ^ d.y;
        acc.z ^= a.z ^ b.z ^ c.z ^ d.z;
        acc.w ^= a.w ^ b.w ^ c.w ^ d.w;
    }
    for (; i < hi; i += 256) {
        const uint4 a = src[i];
        acc.x ^= a.x; acc.y ^= a.y; acc.z ^= a.z; acc.w ^= a.w;
    }
    const uint32_t v = acc.x ^ acc.y ^ acc.z ^ acc.w;
    if (v == 0x9E3779B9u) *sink = v;
}

}  // namespace ssimu2

extern "C" {

int ssimu2_instr_set_segment_rows(ssimu2_ctx* c, int rows_scale0, int rows_other_scales) {
    REMOTE_REFUSE(c, "ssimu2_instr_set_segment_rows");
    if (!c) return SSIMU2_ERR_INVALID_ARG;
    if ((rows_scale0 != 0 && (rows_scale0 < 8 || rows_scale0 > 160)) ||
        (rows_other_scales != 0 && (rows_other_scales < 8 || rows_other_scales > 160)))
        return c->fail(SSIMU2_ERR_INVALID_ARG, "segment rows must be 0 (default rule) or 8..160");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->seg_rows_override = rows_scale0;
    c->seg_rows_tail_override = rows_other_scales;
    release_frame_groups(c);  // the partial-sum buffer is sized by the segment rule; the reference goes with it
    return SSIMU2_OK;
}

int ssimu2_instr_set_batch_segment_rows(ssimu2_ctx* c, int rows_scale0) {
    REMOTE_REFUSE(c, "ssimu2_instr_set_batch_segment_rows");
    if (!c) return SSIMU2_ERR_INVALID_ARG;
    if (rows_scale0 != 0 && rows_scale0 != -1 && (rows_scale0 < 8 || rows_scale0 > 160))
        return c->fail(SSIMU2_ERR_INVALID_ARG, "batch segment rows must be 0 (the rule), -1 (the single-score rule) or 8..160");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->batch_seg_override = rows_scale0;
    return SSIMU2_OK;  // the batch's partial-sum buffer is sized per call
}

int ssimu2_instr_batch_segment_rows(ssimu2_ctx* c, uint32_t w, uint32_t h, int scale, int* out_rows) {
    REMOTE_REFUSE(c, "ssimu2_instr_batch_segment_rows");
    if (!c || !out_rows || scale < 0 || scale >= kNumScales || w == 0 || h == 0) return SSIMU2_ERR_INVALID_ARG;
    *out_rows = batch_seg_rows(c, make_pyramid(w, h), scale);
    return SSIMU2_OK;
}

int ssimu2_instr_placed_streams(ssimu2_ctx* c, int* out_n) {
    REMOTE_REFUSE(c, "ssimu2_instr_placed_streams");
    if (!c || !out_n) return SSIMU2_ERR_INVALID_ARG;
    *out_n = pool_size(c->device);
    return SSIMU2_OK;
}

int ssimu2_instr_rg_stop_after_scale(ssimu2_ctx* c, int scale) {
    REMOTE_REFUSE(c, "ssimu2_instr_rg_stop_after_scale");
    if (!c) return SSIMU2_ERR_INVALID_ARG;
    c->rg_dbg_scale = scale < 0 || scale >= kNumScales ? -1 : scale;
    return SSIMU2_OK;
}

int ssimu2_instr_cache_reference_blur(ssimu2_ctx* c, int enabled) {
    REMOTE_REFUSE(c, "ssimu2_instr_cache_reference_blur");
    if (!c) return SSIMU2_ERR_INVALID_ARG;
    c->cache_ref_blur = enabled != 0;
    c->ref.drop();
    return SSIMU2_OK;
}

int ssimu2_instr_last_march(ssimu2_ctx* c, int* out_kind) {
    REMOTE_REFUSE(c, "ssimu2_instr_last_march");
    if (!c || !out_kind) return SSIMU2_ERR_INVALID_ARG;
    *out_kind = c->last_march;
    return SSIMU2_OK;
}

int ssimu2_debug_download(ssimu2_ctx* c, int what, int scale, uint32_t w, uint32_t h, float* out,
                          uint32_t* out_w, uint32_t* out_h) {
    REMOTE_REFUSE(c, "ssimu2_debug_download");
    if (!c || !out) return SSIMU2_ERR_INVALID_ARG;
    if (w == 0 || h == 0) return c->fail(SSIMU2_ERR_INVALID_ARG, "zero image dimension");
    const Pyramid p = make_pyramid(w, h);
    const float* src = nullptr;
    if ((what == SSIMU2_DEBUG_LIN_REF || what == SSIMU2_DEBUG_LIN_DIST) && scale == 0) {
        // a 16-bit FIR call's scale-0 linear planes (what k_march_lin reads), while they are the last score's
        const bool r = what == SSIMU2_DEBUG_LIN_REF;
        const void* planes = r ? c->hbd.lin0_ref.p : c->hbd.lin0_dist.p;
        if (!planes || p.nscales < 1 || (r ? c->lin0_ref_w : c->lin0_dist_w) != w ||
            (r ? c->lin0_ref_h : c->lin0_dist_h) != h)
            return c->fail(SSIMU2_ERR_INVALID_ARG, "no 16-bit scale-0 planes of that frame from the last score");
        src = (const float*)planes;
    } else if (what == SSIMU2_DEBUG_LIN_REF || what == SSIMU2_DEBUG_LIN_DIST) {
        if (scale < 1 || scale >= p.nscales || !c->frame.lin_ref.p) return c->fail(SSIMU2_ERR_INVALID_ARG, "no such level");
        src = (what == SSIMU2_DEBUG_LIN_REF ? c->frame.lin_ref : c->frame.lin_dist).as<float>() + p.lin_off[scale];
    } else if (what >= SSIMU2_DEBUG_BATCH_LIN_REF) {
        // a level of one item of the last batch: item i's pyramid lies i * lin_stride floats into the batch buffer (batch_run)
        const int kind = SSIMU2_DEBUG_BATCH_LIN_REF + (what - SSIMU2_DEBUG_BATCH_LIN_REF) % SSIMU2_DEBUG_BATCH_ITEM;
        const size_t item = (size_t)(what - SSIMU2_DEBUG_BATCH_LIN_REF) / SSIMU2_DEBUG_BATCH_ITEM;
        const DevBuf& buf = kind == SSIMU2_DEBUG_BATCH_LIN_REF ? c->batch.lin_ref : c->batch.lin_dist;
        const size_t lin_stride = (p.lin_total + 3) & ~(size_t)3;
        if (kind > SSIMU2_DEBUG_BATCH_LIN_DIST || scale < 1 || scale >= p.nscales || item >= c->batch_n || !buf.p ||
            (size_t)c->batch_n * lin_stride * sizeof(float) > buf.cap)
            return c->fail(SSIMU2_ERR_INVALID_ARG, "no such level of such an item of the last batch");
        src = buf.as<float>() + item * lin_stride + p.lin_off[scale];
    } else if (what == SSIMU2_DEBUG_XYB_REF) {
        if (scale < 0 || scale >= p.nscales || !c->cache.xyb.p || !c->ref.have || c->ref.w != w || c->ref.h != h)
            return c->fail(SSIMU2_ERR_INVALID_ARG, "no cached reference XYB for that level");
        src = c->cache.xyb.as<float>() + xyb_off(p, scale);
    } else if (what == SSIMU2_DEBUG_RG_H || what == SSIMU2_DEBUG_RG_V) {
        // 15 raw planes of the scale selected with ssimu2_instr_rg_stop_after_scale before the score
        if (scale < 0 || scale >= p.nscales || scale != c->rg_dbg_scale || !c->rg.dbg.p || !c->rg.planes.p)
            return c->fail(SSIMU2_ERR_INVALID_ARG, "no recursive-blur planes kept for that scale");
        // device planes keep their rows rg_pitch(w) floats apart (ssimu2_recursive.h "Row pitch"); `out` is tight
        const size_t pitch = (size_t)rg_pitch(p.w[scale]), wd = (size_t)p.w[scale], ht = (size_t)p.h[scale];
        const size_t nd = pitch * ht, n1 = wd * ht;
        if (24 * nd * sizeof(float) > c->rg.dbg.cap) return c->fail(SSIMU2_ERR_INVALID_ARG, "recursive-blur planes are of another frame size");
        HIP_TRY(c, hipSetDevice(c->device));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        auto plane = [&](float* dst, const float* src) {
            return hipMemcpy2D(dst, wd * sizeof(float), src, pitch * sizeof(float), wd * sizeof(float), ht, hipMemcpyDeviceToHost);
        };
        if (what == SSIMU2_DEBUG_RG_H) {
            for (int k = 0; k < 15; ++k) HIP_TRY(c, plane(out + (size_t)k * n1, c->rg.dbg.as<float>() + (size_t)k * nd));
        } else {
            // x, xx: the reference cache [channel][{mu1, s11}]; y, yy, xy: k_rg_v_emit's planes
            const float* cache = c->rg.planes.as<float>() + 6 * rg_plane_off(p, p.nscales) + 6 * rg_plane_off(p, scale);
            const float* pass = c->rg.dbg.as<float>() + 15 * nd;
            for (int ch = 0; ch < 3; ++ch) {
                for (int k = 0; k < 2; ++k)
                    HIP_TRY(c, plane(out + (size_t)rg_plane15(true, ch, k) * n1, cache + (size_t)(ch * 2 + k) * nd));
                for (int k = 0; k < 3; ++k)
                    HIP_TRY(c, plane(out + (size_t)rg_plane15(false, ch, k) * n1, pass + (size_t)(ch * 3 + k) * nd));
            }
        }
        if (out_w) *out_w = (uint32_t)p.w[scale];
        if (out_h) *out_h = (uint32_t)p.h[scale];
        return SSIMU2_OK;
    } else if (what == SSIMU2_DEBUG_REF_BLUR) {
        if (scale < 0 || scale >= p.nscales || !c->cache.blur.p || !c->ref.have || c->ref.w != w || c->ref.h != h)
            return c->fail(SSIMU2_ERR_INVALID_ARG, "no cached reference blur for that level");
        src = c->cache.blur.as<float>() + xyb_off(p, scale);
    } else {
        return c->fail(SSIMU2_ERR_INVALID_ARG, "bad `what`");
    }
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const size_t n = (size_t)3 * p.w[scale] * p.h[scale];
    HIP_TRY(c, hipMemcpy(out, src, n * sizeof(float), hipMemcpyDeviceToHost));
    if (out_w) *out_w = (uint32_t)p.w[scale];
    if (out_h) *out_h = (uint32_t)p.h[scale];
    return SSIMU2_OK;
}

int ssimu2_time_device(ssimu2_ctx* c, const void* d_ref, const void* d_dist, uint32_t w,
                       uint32_t h, int iters, float* out_ms_total, double* out_score) {
    REMOTE_REFUSE(c, "ssimu2_time_device");
    int rc = check_args(c, d_ref, d_dist, w, h);
    if (rc) return rc;
    if (iters <= 0 || !out_ms_total) return c->fail(SSIMU2_ERR_INVALID_ARG, "bad iters/out");
    HIP_TRY(c, hipSetDevice(c->device));
    if ((rc = ensure_capacity(c, w, h))) return rc;
    c->ref.drop();  // the lin_ref pyramid is overwritten
    HIP_TRY(c, hipEventRecord(c->ev0, c->stream));
    for (int i = 0; i < iters; ++i)
        if ((rc = enqueue_score(c, (const uint8_t*)d_ref, (const uint8_t*)d_dist, w, h, false)))
            return rc;
    HIP_TRY(c, hipEventRecord(c->ev1, c->stream));
    double score = 0.0;
    if ((rc = ssimu2_wait(c, &score))) return rc;
    HIP_TRY(c, hipEventSynchronize(c->ev1));
    HIP_TRY(c, hipEventElapsedTime(out_ms_total, c->ev0, c->ev1));
    if (out_score) *out_score = score;
    return SSIMU2_OK;
}

}  // extern "C"

// ---- the timing hooks: one timed loop, scratch that ends with the call ---------------------------
namespace {

// What a hook call holds for its length only, released on every way out: its scratch device memory (a local DevBuf
// filled by grow(), freed once the context stream has drained; never kept in the context, so a hook's footprint does
// not outlive the hook) and its events.
template <class F>
struct AtExit {
    F f;
    ~AtExit() { f(); }
};
template <class F>
AtExit(F) -> AtExit<F>;
auto scratch_guard(ssimu2_ctx* c, DevBuf& b) {
    return AtExit{[c, &b] { (void)hipStreamSynchronize(c->stream), b.release(); }};
}

// n value-initialised elements; empty when the host has no memory for them.
template <class T>
std::vector<T> host_array(int n) {
    try {
        return std::vector<T>((size_t)n);
    } catch (const std::bad_alloc&) {
        return {};
    }
}

// The timed loop of every hook: `warm` untimed calls of fn(j), then `iters` timed ones between ev0 and ev1 on the
// context stream, the launch-error check and the wait.  *ms = stream time of the timed calls together.
template <class F>
hipError_t timed_loop(ssimu2_ctx* c, int warm, int iters, float* ms, F&& fn) {
    for (int j = 0; j < warm; ++j) fn(j);
    hipError_t e = hipEventRecord(c->ev0, c->stream);
    for (int j = 0; j < iters && e == hipSuccess; ++j) fn(j);
    if (e == hipSuccess) e = hipEventRecord(c->ev1, c->stream);
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess) e = hipEventSynchronize(c->ev1);
    if (e == hipSuccess) e = hipEventElapsedTime(ms, c->ev0, c->ev1);
    return e;
}

}  // namespace

extern "C" {

int ssimu2_time_stage(ssimu2_ctx* c, const void* d_ref, const void* d_dist, uint32_t w, uint32_t h,
                      int stage, int iters, float* out_ms_avg) {
    REMOTE_REFUSE(c, "ssimu2_time_stage");
    int rc = check_args(c, d_ref, d_dist, w, h);
    if (rc) return rc;
    if (iters <= 0 || !out_ms_avg) return c->fail(SSIMU2_ERR_INVALID_ARG, "bad iters/out");
    double score;
    if ((rc = ssimu2_score_rgb8_device(c, d_ref, d_dist, w, h, &score))) return rc;  // valid inputs
    const Pyramid p = make_pyramid(w, h);
    MarchPlan mp;
    FinalizeArgs fa;
    const int blocks = build_plans(c, p, march_seg_rows, score_sources(c, d_ref, d_dist, false), &mp, &fa);
    if (stage < 0 || stage > 2) return c->fail(SSIMU2_ERR_INVALID_ARG, "bad stage");
    const uint8_t* frames[2] = {(const uint8_t*)d_ref, (const uint8_t*)d_dist};
    float* lin[2] = {c->frame.lin_ref.as<float>(), c->frame.lin_dist.as<float>()};
    float ms = 0.f;
    const hipError_t e = timed_loop(c, 0, iters, &ms, [&](int) {
        if (stage == SSIMU2_STAGE_PYRAMID) launch_pyramid(c, p, 2, frames, lin);
        else if (stage == SSIMU2_STAGE_FINALIZE) launch(k_finalize, dim3(1), dim3(1024), 0, c->stream, fa, c->d_result);
        else if (blocks > 0) launch(k_march, dim3(blocks), dim3(MARCH_THREADS), 0, c->stream, mp);
    });
    if (e != hipSuccess) return c->fail(SSIMU2_ERR_HIP, "stage timing", e);
    *out_ms_avg = ms / (float)iters;
    return SSIMU2_OK;
}

int ssimu2_time_march_rotating(ssimu2_ctx* c, const void* const* d_refs, const void* const* d_dists,
                               int npairs, uint32_t w, uint32_t h, int iters, float* out_ms_avg) {
    REMOTE_REFUSE(c, "ssimu2_time_march_rotating");
    if (!c) return SSIMU2_ERR_INVALID_ARG;
    if (!d_refs || !d_dists || npairs <= 0 || npairs > 64 || iters <= 0 || !out_ms_avg)
        return c->fail(SSIMU2_ERR_INVALID_ARG, "bad pairs/iters/out");
    int rc = check_args(c, d_refs[0], d_dists[0], w, h);
    if (rc) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    if ((rc = ensure_capacity(c, w, h))) return rc;
    c->ref.drop();
    const Pyramid p = make_pyramid(w, h);
    // per-pair linear-light pyramids (what the marching kernel reads at scales >= 1)
    const size_t lin_floats = p.lin_total + 4;
    DevBuf lin;
    const auto free_lin = scratch_guard(c, lin);
    rc = grow(c, lin, (size_t)npairs * 2 * lin_floats * sizeof(float), "hipMalloc(rotating pyramids)");
    if (rc) return rc;
    std::vector<MarchPlan> plans = host_array<MarchPlan>(npairs);
    if (plans.empty()) return c->fail(SSIMU2_ERR_OOM, "plans");
    int blocks = 0;
    for (int i = 0; i < npairs; ++i) {
        if (!d_refs[i] || !d_dists[i]) return c->fail(SSIMU2_ERR_INVALID_ARG, "null pair pointer");
        const uint8_t* frames[2] = {(const uint8_t*)d_refs[i], (const uint8_t*)d_dists[i]};
        float* const lr = lin.as<float>() + (size_t)(2 * i) * lin_floats;
        float* lins[2] = {lr, lr + lin_floats};
        launch_pyramid(c, p, 2, frames, lins);
        PlanSources src = score_sources(c, d_refs[i], d_dists[i], false);
        src.lin_ref = lins[0];
        src.lin_dist = lins[1];
        FinalizeArgs fa;
        blocks = build_plans(c, p, march_seg_rows, src, &plans[i], &fa);
    }
    float ms = 0.f;
    // untimed: ~30 ms of the same launches first.  Allocating the scratch above leaves the GPU
    // idle for a moment, and an MI355X that has been idle runs its next ~100 launches 5-15 %
    // slower while its clocks come back up (kernel-trace of bench.py: 166 -> 154 -> 144 -> 141 us)
    const dim3 grid(blocks), threads(MARCH_THREADS);
    const auto one = [&](int j) { launch(k_march, grid, threads, 0, c->stream, plans[j % npairs]); };
    const hipError_t e = blocks > 0 ? timed_loop(c, npairs * 2 > 192 ? npairs * 2 : 192, iters, &ms, one)
                                    : hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return c->fail(SSIMU2_ERR_HIP, "rotating march timing", e);
    *out_ms_avg = ms / (float)iters;
    return SSIMU2_OK;
}

// The marching body as a PLAIN blur stage (k_ref_blur: positive-XYB planes of one frame in, one
// blurred plane per channel out, all scales in one launch), rotating over `nframes` frames' plane
// sets so that inputs and outputs come from / go to HBM, not the Infinity Cache.
int ssimu2_time_blur_stage_rotating(ssimu2_ctx* c, const void* const* d_frames, int nframes, uint32_t w,
                                    uint32_t h, int iters, float* out_ms_avg, double* out_bytes_per_launch) {
    REMOTE_REFUSE(c, "ssimu2_time_blur_stage_rotating");
    if (!c) return SSIMU2_ERR_INVALID_ARG;
    if (!d_frames || nframes <= 0 || nframes > 16 || iters <= 0 || !out_ms_avg)
        return c->fail(SSIMU2_ERR_INVALID_ARG, "bad frames/iters/out");
    int rc = check_args(c, d_frames[0], d_frames[0], w, h);
    if (rc) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    if ((rc = ensure_capacity(c, w, h))) return rc;
    c->ref.drop();  // the lin_ref pyramid is overwritten
    const Pyramid p = make_pyramid(w, h);
    const size_t planes = xyb_off(p, p.nscales) + 4;  // floats of one plane set (all scales)
    DevBuf buf;
    const auto free_buf = scratch_guard(c, buf);
    rc = grow(c, buf, (size_t)nframes * 2 * planes * sizeof(float), "hipMalloc(rotating blur-stage planes)");
    if (rc) return rc;
    std::vector<MarchPlan> plans = host_array<MarchPlan>(nframes);
    if (plans.empty()) return c->fail(SSIMU2_ERR_OOM, "plans");
    int blocks = 0;
    for (int i = 0; i < nframes; ++i) {
        const uint8_t* frames[1] = {(const uint8_t*)d_frames[i]};
        float* lins[1] = {c->frame.lin_ref.as<float>()};
        float* xyb = buf.as<float>() + (size_t)(2 * i) * planes;
        launch_pyramid(c, p, 1, frames, lins);
        launch_ref_xyb(c, p, frames[0], true, lins[0], xyb);
        FinalizeArgs fa;
        PlanSources src = score_sources(c, frames[0], frames[0], false);
        src.lin_dist = src.lin_ref;  // second frame unused
        src.ref_xyb = xyb;
        src.ref_s11 = xyb + planes;
        blocks = build_plans(c, p, march_seg_rows, src, &plans[i], &fa, MARCH_OUT_PLANES);
    }
    float ms = 0.f;
    hipError_t e = hipSuccess;
    if (blocks > 0)  // 64 untimed: clocks (see ssimu2_time_march_rotating)
        e = timed_loop(c, 64, iters, &ms, [&](int j) {
            launch(k_ref_blur, dim3(blocks), dim3(MARCH_THREADS), 0, c->stream, plans[j % nframes]);
        });
    if (e != hipSuccess) return c->fail(SSIMU2_ERR_HIP, "rotating blur-stage timing", e);
    *out_ms_avg = ms / (float)iters;
    // algorithmic bytes of one launch: every plane element read once and written once
    if (out_bytes_per_launch) *out_bytes_per_launch = 2.0 * (double)xyb_off(p, p.nscales) * sizeof(float);
    return SSIMU2_OK;
}

// Every kernel of a score timed where it runs: `iters` scores enqueued through the product's own enqueue_score() while a
// timing scope is open, so each launch is made with hipExtLaunchKernelGGL and a start / stop event pair -- the kernel's
// duration as its dispatch packet recorded it (what rocprofv3's kernel trace reads), no packet added between the launches.
//   d_refs == NULL: reference-cached passes against `d_ref` (set here with ssimu2_set_reference_device), rotating over
//                   the distorted frames d_dists[0..n-1]   (FIR: pyramid, k_march_refblur, k_finalize;
//                                                            recursive: k_pyramid_bands_xyb, k_rg_h, k_rg_v, k_finalize)
//   d_refs != NULL: pair scores of (d_refs[i], d_dists[i])  (FIR: pyramid, k_march, k_finalize;
//                                                            recursive: the reference's three launches, then the pass's four)
// out_ms_avg[k] = average milliseconds of the k-th launch of a score, *out_launches = launches per score (<= 8);
// *out_ms_wall_timed / *out_ms_wall_plain = stream time per score (events around all `iters` scores) of the timed run and
// of the same run with plain launches: the difference is what the per-launch timestamps cost.
int ssimu2_time_kernels(ssimu2_ctx* c, const void* d_ref, const void* const* d_refs, const void* const* d_dists, int n,
                        uint32_t w, uint32_t h, int iters, float* out_ms_avg, int* out_launches, float* out_ms_wall_timed,
                        float* out_ms_wall_plain) {
    REMOTE_REFUSE(c, "ssimu2_time_kernels");
    if (!c) return SSIMU2_ERR_INVALID_ARG;
    if (!d_dists || n <= 0 || n > 256 || iters <= 0 || iters > 512 || !out_ms_avg || !out_launches)
        return c->fail(SSIMU2_ERR_INVALID_ARG, "bad frames/iters/out");
    if (!d_refs && !d_ref) return c->fail(SSIMU2_ERR_INVALID_ARG, "neither a cached reference nor pairs");
    int rc = check_args(c, d_refs ? d_refs[0] : d_ref, d_dists[0], w, h);
    if (rc) return rc;
    for (int i = 0; i < n; ++i)
        if (!d_dists[i] || (d_refs && !d_refs[i])) return c->fail(SSIMU2_ERR_INVALID_ARG, "null frame pointer");
    const bool cached = d_refs == nullptr;
    if (cached) {
        if ((rc = ssimu2_set_reference_device(c, d_ref, w, h))) return rc;
    } else {
        HIP_TRY(c, hipSetDevice(c->device));
        if ((rc = ensure_capacity(c, w, h))) return rc;
        c->ref.drop();  // the lin_ref pyramid is overwritten
    }
    auto one = [&](int j) {  // score j of a window; nothing more once one has failed
        if (rc) return;
        rc = cached ? enqueue_score(c, c->frame.ref_u8.as<uint8_t>(), (const uint8_t*)d_dists[j % n], w, h, true)
                    : enqueue_score(c, (const uint8_t*)d_refs[j % n], (const uint8_t*)d_dists[j % n], w, h, false);
    };
    constexpr int kMaxLaunches = 8;
    const int nev = 2 * kMaxLaunches * iters;
    std::vector<hipEvent_t> ev = host_array<hipEvent_t>(nev);
    if (ev.empty()) return c->fail(SSIMU2_ERR_OOM, "events");
    AtExit destroy_events{[&] {
        for (hipEvent_t x : ev)
            if (x) (void)hipEventDestroy(x);
    }};
    hipError_t e = hipSuccess;
    for (int i = 0; i < nev && e == hipSuccess; ++i) e = hipEventCreate(&ev[i]);
    double sum[kMaxLaunches] = {0};
    float wall_timed = 0.f, wall_plain = 0.f;
    int per_score = 0;
    if (e == hipSuccess) {
        // plain launches first, after a warm-up (clocks and caches as in a run of scores): the stream time per score
        // without the timestamps
        e = timed_loop(c, 2 * n > 24 ? 2 * n : 24, iters, &wall_plain, one);
        // the same scores with a start / stop event pair on every launch.  Not timed_loop: the per-launch events below
        // are read after a wait for the whole stream, not for ev1 alone
        LaunchTimer timer{ev.data(), 0, nev};
        if (rc == 0 && e == hipSuccess) e = hipEventRecord(c->ev0, c->stream);
        g_launch_timer = &timer;
        for (int j = 0; j < iters; ++j) one(j);
        g_launch_timer = nullptr;
        if (rc == 0 && e == hipSuccess) e = hipEventRecord(c->ev1, c->stream);
        if (rc == 0 && e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (rc == 0 && e == hipSuccess) e = hipEventElapsedTime(&wall_timed, c->ev0, c->ev1);
        per_score = timer.n / 2 / iters;
        if (rc == 0 && e == hipSuccess && (timer.n % (2 * iters) != 0 || per_score < 1 || per_score > kMaxLaunches)) {
            rc = c->fail(SSIMU2_ERR_INVALID_ARG, "the scores did not all make the same number of launches");
        }
        for (int j = 0; j < iters && rc == 0 && e == hipSuccess; ++j)
            for (int k = 0; k < per_score && e == hipSuccess; ++k) {
                float ms = 0.f;
                e = hipEventElapsedTime(&ms, ev[2 * (j * per_score + k)], ev[2 * (j * per_score + k) + 1]);
                sum[k] += ms;
            }
    }
    (void)hipStreamSynchronize(c->stream);
    c->pending = false;
    if (rc) return rc;
    if (e != hipSuccess) return c->fail(SSIMU2_ERR_HIP, "per-kernel timing", e);
    for (int k = 0; k < per_score; ++k) out_ms_avg[k] = (float)(sum[k] / iters);
    *out_launches = per_score;
    if (out_ms_wall_timed) *out_ms_wall_timed = wall_timed / (float)iters;
    if (out_ms_wall_plain) *out_ms_wall_plain = wall_plain / (float)iters;
    return SSIMU2_OK;
}

int ssimu2_measure_read_stream(ssimu2_ctx* c, size_t bytes, int iters, double* out_gbps) {
    REMOTE_REFUSE(c, "ssimu2_measure_read_stream");
    if (!c) return SSIMU2_ERR_INVALID_ARG;
    if (bytes < (1u << 20) || iters <= 0 || !out_gbps)
        return c->fail(SSIMU2_ERR_INVALID_ARG, "bad bytes/iters/out");
    HIP_TRY(c, hipSetDevice(c->device));
    DevBuf buf;
    const auto free_buf = scratch_guard(c, buf);
    const int rc = grow(c, buf, bytes + 64, "hipMalloc(read-stream scratch)");
    if (rc) return rc;
    uint32_t* sink = (uint32_t*)(buf.as<uint8_t>() + (bytes & ~(size_t)15));
    float ms = 0.f;
    const size_t n16 = bytes / 16;
    const int grid = 256 * 16;  // 16 workgroups of 4 waves per CU: the CUs' full wave capacity
    hipError_t e = hipMemsetAsync(buf.p, 0, bytes + 64, c->stream);
    if (e == hipSuccess)  // one untimed launch first
        e = timed_loop(c, 1, iters, &ms, [&](int) {
            launch(k_read_stream, dim3(grid), dim3(256), 0, c->stream, buf.as<uint4>(), n16, sink);
        });
    if (e != hipSuccess) return c->fail(SSIMU2_ERR_HIP, "read-stream probe", e);
    *out_gbps = (double)(n16 * 16) / ((double)ms / iters * 1e-3) * 1e-9;
    return SSIMU2_OK;
}

}  // extern "C"
