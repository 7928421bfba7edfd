// RGBA input of the MI355X SSIMULACRA2 scorer: the entry points of include/ssimu2_hip_ext.h.
//
// This translation unit is the product translation unit (ssimu2_hip.hip, included below: same kernels, same host
// code, same flags) plus one kernel and five functions.  It is built into liboavif_hip_ext.so; liboavif_hip.so and
// liboavif_hip_instr.so contain none of this, and their exports are what they were.
//
// An RGBA frame becomes a u16 frame of exact integer codes n = a * c + (255 - a) * b (k_composite_rgba8) that the
// 16-bit front end reads through a table of its own: Src16{codes, w * 6, 3, T, 65025}.  No pyramid, marching,
// recursive or finalize kernel knows about alpha.
#define SSIMU2_EXT_BUILD 1
#include "ssimu2_hip.hip"

#include "../../include/ssimu2_hip_ext.h"

namespace ssimu2 {

// ---------------------------------------------------------------------------------------------
// RGBA rows `pitch` bytes apart (any alignment) over the background `bg` = 0xRRGGBB -> tight u16 RGB codes.
// A lane takes four pixels of one row: four unaligned dword loads (16 bytes) and six dword stores (24 bytes: a row of
// codes starts 6 * w * y bytes in, 2-byte aligned only); the last w % 4 pixels of a row go sample by sample.  Rows
// beyond gridDim.y are taken in further rounds.  Pure integer arithmetic (n < 2^16), HBM-bound: 10 bytes per pixel.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t composite_code(uint32_t a, uint32_t c, uint32_t b) { return a * c + (255u - a) * b; }

__global__ __launch_bounds__(256) void k_composite_rgba8(const uint8_t* __restrict__ src, uint32_t pitch, uint32_t w,
                                                         uint32_t h, uint32_t bg, uint16_t* __restrict__ dst) {
    const uint32_t x0 = (blockIdx.x * 256u + threadIdx.x) * 4u;
    if (x0 >= w) return;
    const uint32_t b[3] = {(bg >> 16) & 0xFFu, (bg >> 8) & 0xFFu, bg & 0xFFu};
    for (uint32_t y = blockIdx.y; y < h; y += gridDim.y) {
        const uint8_t* s = src + (size_t)y * pitch + (size_t)x0 * 4u;
        uint16_t* d = dst + ((size_t)y * w + x0) * 3u;
        if (x0 + 4u <= w) {
            uint32_t px[4];  // LE: R | G << 8 | B << 16 | A << 24
#pragma unroll
            for (int k = 0; k < 4; ++k) __builtin_memcpy(&px[k], s + 4 * k, 4);
            uint32_t n[12];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t a = px[k] >> 24;
#pragma unroll
                for (int c = 0; c < 3; ++c) n[3 * k + c] = composite_code(a, (px[k] >> (8 * c)) & 0xFFu, b[c]);
            }
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                const uint32_t pair = n[2 * k] | (n[2 * k + 1] << 16);
                __builtin_memcpy((uint8_t*)d + 4 * k, &pair, 4);
            }
        } else {
            for (uint32_t i = 0; x0 + i < w; ++i) {
                const uint32_t a = s[4 * i + 3];
#pragma unroll
                for (int c = 0; c < 3; ++c) d[3 * i + c] = (uint16_t)composite_code(a, s[4 * i + c], b[c]);
            }
        }
    }
}

}  // namespace ssimu2

namespace {

constexpr uint32_t kAlphaTop = SSIMU2_ALPHA_CODES - 1;  // 65025 = 255 * 255, the largest code

// T: the 8-bit table's expression at v = n / 65025, fp64, rounded once.  65025 = 255 * 255, so entry 255 u is the
// 8-bit entry u bit for bit (v is the same double).  Built once per process.
const float* host_alpha_table() {
    static std::mutex mu;
    static float* tab = nullptr;
    std::lock_guard<std::mutex> lock(mu);
    if (!tab) {
        float* t = new (std::nothrow) float[SSIMU2_ALPHA_CODES];
        if (!t) return nullptr;
        for (uint32_t i = 0; i < SSIMU2_ALPHA_CODES; ++i) {
            const double v = (double)i / (double)kAlphaTop;
            t[i] = (float)(v <= 0.04045 ? v / 12.92 : pow((v + 0.055) / 1.055, 2.4));
        }
        tab = t;
    }
    return tab;
}

// The device copy of T (uploaded on the context stream by the context's first RGBA call).
int alpha_device_table(ssimu2_ctx* c, const float** out) {
    if (!c->alpha_tab.p) {
        const float* t = host_alpha_table();
        if (!t) return c->fail(SSIMU2_ERR_OOM, "composite table");
        const size_t bytes = (size_t)SSIMU2_ALPHA_CODES * sizeof(float);
        const int rc = grow(c, c->alpha_tab, bytes, "hipMalloc(composite table)");
        if (rc) return rc;
        const hipError_t e = hipMemcpyAsync(c->alpha_tab.p, t, bytes, hipMemcpyHostToDevice, c->stream);
        if (e != hipSuccess) {
            c->alpha_tab.release();
            return c->fail(SSIMU2_ERR_HIP, "hipMemcpyAsync(composite table)", e);
        }
    }
    *out = c->alpha_tab.as<float>();
    return SSIMU2_OK;
}

// Argument checks of the RGBA calls that name a frame size (the ctx may be null).
int check_rgba(ssimu2_ctx* c, const void* a, const void* b, uint32_t row_bytes_a, uint32_t row_bytes_b, uint32_t w,
               uint32_t h, uint32_t background_rgb) {
    int rc = check_args(c, a, b, w, h);
    if (rc) return rc;
    if ((uint64_t)row_bytes_a < (uint64_t)w * 4 || (uint64_t)row_bytes_b < (uint64_t)w * 4)
        return c->fail(SSIMU2_ERR_INVALID_ARG, "row_bytes smaller than one row of RGBA pixels");
    if (background_rgb > 0xFFFFFFu) return c->fail(SSIMU2_ERR_INVALID_ARG, "background_rgb is 0xRRGGBB: the upper byte must be 0");
    return SSIMU2_OK;
}

// One RGBA frame from host memory, composited over `bg` into the tight u16 frame `codes` (w * h * 6 bytes): the rows
// go through the staging buffer as they are (the last row needs only its pixels, not its padding).
int composite_upload(ssimu2_ctx* c, const uint8_t* pixels, uint32_t row_bytes, uint32_t w, uint32_t h, uint32_t bg,
                     DevBuf& codes) {
    int rc = grow(c, codes, (size_t)w * h * 3 * sizeof(uint16_t), "hipMalloc(composited frames)");
    if (rc || (rc = stage_upload(c, pixels, (size_t)row_bytes * (h - 1) + (size_t)w * 4))) return rc;
    const uint32_t groups = (w + 3) / 4;
    launch(k_composite_rgba8, dim3((groups + 255) / 256, h < 65535u ? h : 65535u), dim3(256), 0, c->stream,
           c->stage.as<uint8_t>(), row_bytes, w, h, bg, codes.as<uint16_t>());
    return SSIMU2_OK;
}

Src16 composited16(const DevBuf& codes, uint32_t w, const float* tab) { return {codes.p, w * 6u, 3u, tab, kAlphaTop}; }

}  // namespace

extern "C" {

int ssimu2_alpha_table(float* out) {
    if (!out) return SSIMU2_ERR_INVALID_ARG;
    const float* t = host_alpha_table();
    if (!t) return SSIMU2_ERR_OOM;
    memcpy(out, t, (size_t)SSIMU2_ALPHA_CODES * sizeof(float));
    return SSIMU2_OK;
}

int ssimu2_composite_rgba8(ssimu2_ctx* c, const uint8_t* pixels, uint32_t row_bytes, uint32_t w, uint32_t h,
                           uint32_t background_rgb, uint16_t* out_codes) {
    REMOTE_REFUSE(c, "ssimu2_composite_rgba8");
    int rc = check_rgba(c, pixels, out_codes, row_bytes, row_bytes, w, h, background_rgb);
    if (rc) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    if ((rc = composite_upload(c, pixels, row_bytes, w, h, background_rgb, c->hbd.dist16))) return rc;
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(out_codes, c->hbd.dist16.p, (size_t)w * h * 3 * sizeof(uint16_t), hipMemcpyDeviceToHost,
                              c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SSIMU2_OK;
}

int ssimu2_score_rgba8(ssimu2_ctx* c, const uint8_t* ref, uint32_t ref_row_bytes, const uint8_t* dist,
                       uint32_t dist_row_bytes, uint32_t w, uint32_t h, uint32_t background_rgb, double* out_score) {
    REMOTE_REFUSE(c, "ssimu2_score_rgba8");
    int rc = check_rgba(c, ref, dist, ref_row_bytes, dist_row_bytes, w, h, background_rgb);
    if (rc) return rc;
    if (!out_score) return c->fail(SSIMU2_ERR_INVALID_ARG, "null out_score");
    if (c->blur_mode != SSIMU2_BLUR_FIR && (rc = rg_check_size(c, w, h))) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    if ((rc = ensure_capacity(c, w, h))) return rc;
    c->ref.drop();  // the lin_ref pyramid is overwritten
    const float* tab = nullptr;
    if ((rc = hbd_planes(c, w, h, true)) || (rc = alpha_device_table(c, &tab)) ||
        (rc = composite_upload(c, ref, ref_row_bytes, w, h, background_rgb, c->hbd.ref16)) ||
        (rc = composite_upload(c, dist, dist_row_bytes, w, h, background_rgb, c->hbd.dist16))) {
        (void)hipStreamSynchronize(c->stream);  // the caller may free its frames after any return
        return rc;
    }
    const Src16 r = composited16(c->hbd.ref16, w, tab);
    if ((rc = enqueue_score16(c, &r, composited16(c->hbd.dist16, w, tab), w, h))) {
        (void)hipStreamSynchronize(c->stream);
        return rc;
    }
    return ssimu2_wait(c, out_score);
}

int ssimu2_set_reference_rgba8(ssimu2_ctx* c, const uint8_t* ref, uint32_t row_bytes, uint32_t w, uint32_t h,
                               uint32_t background_rgb) {
    REMOTE_REFUSE(c, "ssimu2_set_reference_rgba8");
    int rc = check_rgba(c, ref, ref, row_bytes, row_bytes, w, h, background_rgb);
    if (rc) return rc;
    const bool fir = c->blur_mode == SSIMU2_BLUR_FIR;
    if (!fir && (rc = rg_check_size(c, w, h))) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    if ((rc = ensure_capacity(c, w, h))) return rc;
    const Pyramid p = make_pyramid(w, h);
    if (!fir && (rc = rg_ensure(c, p))) return rc;
    c->ref.drop();  // the lin_ref pyramid and the cached planes are overwritten
    const float* tab = nullptr;
    if ((rc = hbd_planes(c, w, h, true)) || (rc = alpha_device_table(c, &tab)) ||
        (rc = composite_upload(c, ref, row_bytes, w, h, background_rgb, c->hbd.ref16))) {
        (void)hipStreamSynchronize(c->stream);
        return rc;
    }
    const Src16 r = composited16(c->hbd.ref16, w, tab);
    if (fir) {  // as ssimu2_set_reference_rgb16: linear pyramid and scale-0 planes, then the caches (required)
        const Src16* src[1] = {&r};
        float* lin[1] = {c->frame.lin_ref.as<float>()};
        float* lin0[1] = {c->hbd.lin0_ref.as<float>()};
        launch_pyramid16(c, p, 1, src, lin, lin0);
        if (p.nscales >= 1) note_lin0(c, 1, -1, w, h);
        if ((rc = cache_reference_fir(c, p, c->hbd.lin0_ref.p, false, true))) {
            (void)hipStreamSynchronize(c->stream);
            return rc;
        }
    } else {
        rg_enqueue_reference(c, p, nullptr, &r);
    }
    if ((rc = reference_set(c, w, h, true))) return rc;
    c->ref.bg = (int64_t)background_rgb;
    return SSIMU2_OK;
}

int ssimu2_score_against_reference_rgba8(ssimu2_ctx* c, const uint8_t* pixels, uint32_t row_bytes, double* out_score) {
    REMOTE_REFUSE(c, "ssimu2_score_against_reference_rgba8");
    int rc = check_against(c, pixels && out_score);
    if (rc) return rc;
    if (c->ref.bg < 0)
        return c->fail(SSIMU2_ERR_INVALID_ARG, "the reference was not set by ssimu2_set_reference_rgba8: no background recorded");
    const uint32_t w = c->ref.w, h = c->ref.h;
    if ((uint64_t)row_bytes < (uint64_t)w * 4)
        return c->fail(SSIMU2_ERR_INVALID_ARG, "row_bytes smaller than one row of RGBA pixels");
    HIP_TRY(c, hipSetDevice(c->device));
    const float* tab = nullptr;
    if ((rc = hbd_planes(c, w, h, false)) || (rc = alpha_device_table(c, &tab)) ||
        (rc = composite_upload(c, pixels, row_bytes, w, h, (uint32_t)c->ref.bg, c->hbd.dist16))) {
        (void)hipStreamSynchronize(c->stream);
        return rc;
    }
    if ((rc = score_against_reference16(c, composited16(c->hbd.dist16, w, tab), out_score)))
        (void)hipStreamSynchronize(c->stream);
    return rc;
}

}  // extern "C"
