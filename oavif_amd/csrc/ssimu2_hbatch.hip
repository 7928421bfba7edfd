// Batches of 16-bit and YUV frames in the recursive blur modes of the MI355X SSIMULACRA2 scorer: the entry points of
// include/ssimu2_hip_hbatch.h.
//
// A translation unit of its own over ssimu2_host.h: one kernel template -- the YUV-to-codes conversion of a whole
// batch, which needs nothing of the scorer unit's constants -- and six functions.  The rgb16 forms check their
// arguments, stage the host frames and hand over to hbatch_run, which is ssimu2_hip.hip's: rbatch_recursive with a
// 16-bit conversion launch (k_pyramid_bands_xyb16_batch) in place of the 8-bit one.  A YUV batch is, by section 14's
// definition, the rgb16 batch of its codes: the planes of all n frames are staged tight, one launch makes the codes of
// all of them, and the same hbatch_run scores those.  Its object is linked with the rbatch library's objects into
// liboavif_hip_hbatch.so; the other eight libraries contain none of this, and their exports are what they were.
#include "../../include/ssimu2_hip_hbatch.h"
#include "ssimu2_host.h"
#include "ssimu2_yuv_pixel.h"

using namespace ssimu2h;

namespace ssimu2 {

// The planes of a batch as the library staged them and where the codes go.  Item i's planes lie i * item_stride bytes
// behind item 0's, its codes i * dst_stride u16 behind item 0's: one layout for all items.
struct YuvBatchArgs {
    const uint8_t* planes;      // item 0's Y plane
    size_t off_u, off_v;        // bytes from an item's Y plane to its U and V planes
    size_t item_stride;         // bytes between the planes of consecutive items
    uint32_t pitch_y, pitch_c;  // bytes per row of Y, of U and V
    uint32_t w, h;
    YuvK k;
    uint16_t* dst;              // item 0's tight u16 RGB codes
    size_t dst_stride;          // u16 between the codes of consecutive items
};

constexpr int FMT_444 = 0, FMT_400 = 1, FMT_422 = 2, FMT_420 = 3;

// Four luma samples of one row from `sy` on: one unaligned dword load (S = 1) or two (S = 2), as k_yuv_to_codes and
// k_yuv_chroma_to_codes take them.
template <int S>
__device__ __forceinline__ void luma4(const uint8_t* sy, uint32_t* smp) {
    if (S == 1) {
        uint32_t four;
        __builtin_memcpy(&four, sy, 4);
#pragma unroll
        for (int i = 0; i < 4; ++i) smp[i] = (four >> (8 * i)) & 0xFFu;
    } else {
        uint32_t two[2];
        __builtin_memcpy(&two[0], sy, 4);
        __builtin_memcpy(&two[1], sy + 4, 4);
#pragma unroll
        for (int i = 0; i < 4; ++i) smp[i] = (two[i >> 1] >> (16 * (i & 1))) & 0xFFFFu;
    }
}

// The twelve codes of a lane's four pixels -> six dword stores (a row of codes is 2-byte aligned only).
__device__ __forceinline__ void store4(uint16_t* d, const uint32_t* n) {
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const uint32_t pair = n[2 * i] | (n[2 * i + 1] << 16);
        __builtin_memcpy((uint8_t*)d + 4 * i, &pair, 4);
    }
}

// ---------------------------------------------------------------------------------------------
// The YUV-to-codes conversion of a BATCH: blockIdx.z is the item (n <= SSIMU2_MAX_BATCH = 4096 < 65536); its planes
// and its codes are offset by the per-item strides, formed on the scalar unit (blockIdx.z is uniform).  Per item the
// arithmetic is, operation for operation, that of the single kernels, from the same helpers (ssimu2_yuv_pixel.h):
//   FMT_444, FMT_400   k_yuv_to_codes<S, MONO>: a lane takes four pixels of one row; rows beyond gridDim.y in rounds.
//   FMT_422, FMT_420   k_yuv_chroma_to_codes<S, V, BILINEAR>: a lane takes four luma columns of the luma rows that
//                      share chroma row r and normalises the chroma samples those blend once per plane; every
//                      neighbour index is clamped into the plane BEFORE its load (the header's ac / ar rule); chroma
//                      rows beyond gridDim.y in rounds.
// Nothing is read before a plane's first sample or beyond its last: the four-sample loads are made only where all four
// columns exist (x0 + 4 <= w; `inner` for chroma), every other sample is loaded alone at a clamped index.  In a batch
// that matters beyond faults: items lie back to back, and an over-read would take the neighbour's samples silently.
// No LDS, no scratch (every array index is a constant once unrolled).
// ---------------------------------------------------------------------------------------------
template <int S, int FMT, bool BILINEAR>
__global__ __launch_bounds__(256) void k_yuv_batch_to_codes(YuvBatchArgs a) {
    const uint32_t w = a.w, h = a.h;
    const uint32_t x0 = (blockIdx.x * 256u + threadIdx.x) * 4u;
    if (x0 >= w) return;
    const size_t item = blockIdx.z;
    const uint8_t* const py = a.planes + item * a.item_stride;
    const uint8_t* const pu = py + a.off_u;
    const uint8_t* const pv = py + a.off_v;
    uint16_t* const dst = a.dst + item * a.dst_stride;
    const YuvK& k = a.k;
    if constexpr (FMT == FMT_444 || FMT == FMT_400) {
        constexpr bool MONO = FMT == FMT_400;
        // one pixel: the samples y, u, v -> its three codes.  MONO: Cb = Cr = 0, R = G = B = Y in the same bits
        auto pixel = [&](uint32_t y, uint32_t u, uint32_t v, uint32_t* code) {
            const float Y = yuv_unorm(y, k.max_code, k.bias_y, k.range_y);
            if (MONO) {
                code[0] = code[1] = code[2] = yuv_code(Y, k.top);
                return;
            }
            yuv_codes(Y, yuv_unorm(u, k.max_code, k.bias_uv, k.range_uv), yuv_unorm(v, k.max_code, k.bias_uv, k.range_uv), k, code);
        };
        for (uint32_t y = blockIdx.y; y < h; y += gridDim.y) {
            const uint8_t* const sy = py + (size_t)y * a.pitch_y + (size_t)x0 * S;
            const uint8_t* const su = pu + (size_t)y * a.pitch_c + (size_t)x0 * S;
            const uint8_t* const sv = pv + (size_t)y * a.pitch_c + (size_t)x0 * S;
            uint16_t* const d = dst + ((size_t)y * w + x0) * 3u;
            if (x0 + 4u <= w) {
                uint32_t smp[3][4] = {};  // [plane][pixel]
                luma4<S>(sy, smp[0]);
                if (!MONO) {
                    luma4<S>(su, smp[1]);
                    luma4<S>(sv, smp[2]);
                }
                uint32_t n[12];
#pragma unroll
                for (int i = 0; i < 4; ++i) pixel(smp[0][i], smp[1][i], smp[2][i], n + 3 * i);
                store4(d, n);
            } else {
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    if (x0 + (uint32_t)i < w) {
                        uint32_t n[3];
                        pixel(sample_at<S>(sy, (uint32_t)i), MONO ? 0u : sample_at<S>(su, (uint32_t)i),
                              MONO ? 0u : sample_at<S>(sv, (uint32_t)i), n);
#pragma unroll
                        for (int c = 0; c < 3; ++c) d[3 * i + c] = (uint16_t)n[c];
                    }
                }
            }
        }
    } else {
        constexpr bool V = FMT == FMT_420;
        constexpr int NR = (BILINEAR && V) ? 3 : 1;  // chroma rows a lane holds: r - 1, r, r + 1, or r alone
        constexpr int NC = BILINEAR ? 4 : 2;         // chroma columns: c0 - 1 .. c0 + 2, or c0, c0 + 1
        constexpr int QC = NR == 3 ? 1 : 0;          // where row r is among them
        constexpr int LC = BILINEAR ? 1 : 0;         // where column c0 is
        const uint32_t cw = (w + 1u) / 2u, ch = V ? (h + 1u) / 2u : h;
        const uint32_t c0 = x0 >> 1;
        uint32_t col[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const uint32_t at = c0 + (uint32_t)c;  // LC columns to the right of the one meant
            col[c] = min(at >= (uint32_t)LC ? at - (uint32_t)LC : 0u, cw - 1u);
        }
        // all NC columns inside the plane (no index was clamped): they are adjacent, one load per row takes them
        const bool inner = c0 >= (uint32_t)LC && c0 + (uint32_t)(NC - 1 - LC) < cw;
        for (uint32_t r = blockIdx.y; r < ch; r += gridDim.y) {
            float cb[NR][NC], cr[NR][NC];
#pragma unroll
            for (int q = 0; q < NR; ++q) {
                const uint32_t row = NR == 3 ? (q == 0 ? (r ? r - 1u : 0u) : q == 1 ? r : min(r + 1u, ch - 1u)) : r;
                const uint8_t* const ru = pu + (size_t)row * a.pitch_c;
                const uint8_t* const rv = pv + (size_t)row * a.pitch_c;
                uint32_t su[NC], sv[NC];
                if (inner) {
                    samples_at<S, NC>(ru + (size_t)col[0] * S, su);
                    samples_at<S, NC>(rv + (size_t)col[0] * S, sv);
                } else {
#pragma unroll
                    for (int c = 0; c < NC; ++c) su[c] = sample_at<S>(ru, col[c]), sv[c] = sample_at<S>(rv, col[c]);
                }
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    cb[q][c] = yuv_unorm(su[c], k.max_code, k.bias_uv, k.range_uv);
                    cr[q][c] = yuv_unorm(sv[c], k.max_code, k.bias_uv, k.range_uv);
                }
            }
#pragma unroll
            for (int jj = 0; jj < (V ? 2 : 1); ++jj) {
                const uint32_t j = V ? 2u * r + (uint32_t)jj : r;
                if (j >= h) continue;  // the last chroma row of an odd height has one luma row
                const int qn = NR == 3 ? 2 * jj : 0;  // the neighbour row: above an even luma row, below an odd one
                const uint8_t* const sy = py + (size_t)j * a.pitch_y + (size_t)x0 * S;
                uint16_t* const d = dst + ((size_t)j * w + x0) * 3u;
                // pixel i of the lane's four, of luma sample y -> its three codes
                auto pixel = [&](int i, uint32_t y, uint32_t* code) {
                    const int lc = LC + (i >> 1), ln = BILINEAR ? ((i & 1) ? lc + 1 : lc - 1) : lc;
                    float Cb = cb[QC][lc], Cr = cr[QC][lc];
                    if (BILINEAR) {
                        Cb = chroma_blend(cb[QC][lc], cb[QC][ln], cb[qn][lc], cb[qn][ln]);
                        Cr = chroma_blend(cr[QC][lc], cr[QC][ln], cr[qn][lc], cr[qn][ln]);
                    }
                    yuv_codes(yuv_unorm(y, k.max_code, k.bias_y, k.range_y), Cb, Cr, k, code);
                };
                if (x0 + 4u <= w) {
                    uint32_t smp[4];
                    luma4<S>(sy, smp);
                    uint32_t n[12];
#pragma unroll
                    for (int i = 0; i < 4; ++i) pixel(i, smp[i], n + 3 * i);
                    store4(d, n);
                } else {
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
                        if (x0 + (uint32_t)i < w) {
                            uint32_t n[3];
                            pixel(i, sample_at<S>(sy, (uint32_t)i), n);
#pragma unroll
                            for (int c = 0; c < 3; ++c) d[3 * i + c] = (uint16_t)n[c];
                        }
                    }
                }
            }
        }
    }
}

}  // namespace ssimu2

using namespace ssimu2;

namespace {

size_t up16(size_t x) { return (x + 15) & ~(size_t)15; }

int refuse_fir(ssimu2_ctx* c) {
    if (c->blur_mode != SSIMU2_BLUR_FIR) return SSIMU2_OK;
    return c->fail(SSIMU2_ERR_UNSUPPORTED, "16-bit batches run in the recursive modes only: switch the context with "
                                           "ssimu2_ctx_set_blur, or score the frames one by one");
}

int check_depth(ssimu2_ctx* c, uint32_t bit_depth) {
    if (bit_depth < 8 || bit_depth > 16) return c->fail(SSIMU2_ERR_UNSUPPORTED, "bit_depth must be 8..16");
    return SSIMU2_OK;
}

// What the device forms check of their strides, behind the pointers and the size.
int check_stride(ssimu2_ctx* c, size_t item_stride_bytes, uint32_t w, uint32_t h) {
    if ((uint64_t)item_stride_bytes < (uint64_t)w * h * 6)
        return c->fail(SSIMU2_ERR_INVALID_ARG, "item_stride_bytes smaller than one frame");
    if (item_stride_bytes & 1u) return c->fail(SSIMU2_ERR_INVALID_ARG, "item_stride_bytes is odd");
    return SSIMU2_OK;
}

int check_items16(ssimu2_ctx* c, const uint16_t* const* frames, uint32_t n) {
    for (uint32_t i = 0; i < n; ++i) {
        if (!frames[i]) return c->fail(SSIMU2_ERR_INVALID_ARG, "null image pointer in the batch");
        if ((uintptr_t)frames[i] & 1u) return c->fail(SSIMU2_ERR_INVALID_ARG, "16-bit image pointer not 2-byte aligned");
    }
    return SSIMU2_OK;
}

// n host frames of `bytes` bytes into buffer `which` of the batch group, `stride` bytes apart, on the context stream.
int stage16(ssimu2_ctx* c, int which, const uint16_t* const* frames, uint32_t n, size_t bytes, size_t stride,
            uint8_t** d_frames) {
    int rc = hbatch_buffer(c, which, (size_t)n * stride, d_frames);
    if (rc) return rc;
    for (uint32_t i = 0; i < n; ++i)
        HIP_TRY(c, hipMemcpyAsync(*d_frames + (size_t)i * stride, frames[i], bytes, hipMemcpyHostToDevice, c->stream));
    return SSIMU2_OK;
}

// ---- a YUV batch: the checks, the staging, the one conversion launch -------------------------------
// The layout the library chooses for every item: rows tight, the planes back to back, each start and the item rounded
// up to 16 bytes.
struct YuvLayout {
    uint32_t S, nplanes, cw, ch, fmt;
    bool bilinear;
    size_t off_u, off_v, item_stride;
    YuvK k;
};

// Every frame through check_chroma; every frame of frame 0's kind.
int check_frames(ssimu2_ctx* c, const ssimu2_yuv_frame* frames, uint32_t n, uint32_t w, uint32_t rgb_depth, uint32_t up) {
    for (uint32_t i = 0; i < n; ++i) {
        const int rc = check_chroma(c, &frames[i], w, rgb_depth, up);
        if (rc) return rc;
        if (frames[i].depth != frames[0].depth || frames[i].format != frames[0].format ||
            frames[i].full_range != frames[0].full_range || frames[i].matrix_coefficients != frames[0].matrix_coefficients)
            return c->fail(SSIMU2_ERR_INVALID_ARG, "the frames of a YUV batch share depth, format, range and matrix: "
                                                   "score mixed frames one by one");
    }
    return SSIMU2_OK;
}

YuvLayout yuv_layout(const ssimu2_yuv_frame& f0, uint32_t w, uint32_t h, uint32_t rgb_depth, uint32_t up) {
    ChromaAux aux;
    (void)chroma_feed(f0, w, h, rgb_depth, up, &aux);  // the one yuv_constants
    YuvLayout l{};
    l.k = aux.yuv.k;
    l.S = f0.depth > 8 ? 2u : 1u;
    l.fmt = f0.format == SSIMU2_YUV_444 ? FMT_444 : f0.format == SSIMU2_YUV_400 ? FMT_400 : f0.format == SSIMU2_YUV_422 ? FMT_422 : FMT_420;
    l.bilinear = aux.bilinear;
    l.nplanes = l.fmt == FMT_400 ? 1u : 3u;
    l.cw = l.fmt >= FMT_422 ? (w + 1u) / 2u : w;
    l.ch = l.fmt == FMT_420 ? (h + 1u) / 2u : h;
    const size_t ybytes = up16((size_t)w * h * l.S), cbytes = up16((size_t)l.cw * l.ch * l.S);
    l.off_u = l.nplanes == 3 ? ybytes : 0;
    l.off_v = l.nplanes == 3 ? ybytes + cbytes : 0;
    l.item_stride = l.nplanes == 3 ? ybytes + 2 * cbytes : ybytes;
    return l;
}

// The planes of all n frames into the batch's staging buffer (one 2D copy per plane and item, rows made tight), then
// ONE launch that makes the codes of all of them at d_codes, 3 * w * h u16 per item.  The copies come first.
int stage_and_convert(ssimu2_ctx* c, const ssimu2_yuv_frame* frames, uint32_t n, uint32_t w, uint32_t h, const YuvLayout& l,
                      uint8_t* d_planes, uint16_t* d_codes) {
    for (uint32_t i = 0; i < n; ++i)
        for (uint32_t p = 0; p < l.nplanes; ++p) {
            const uint32_t pw = p ? l.cw : w, ph = p ? l.ch : h;
            const size_t row = (size_t)pw * l.S;
            uint8_t* const to = d_planes + (size_t)i * l.item_stride + (p == 1 ? l.off_u : p == 2 ? l.off_v : 0);
            if (ph == 1 || frames[i].row_bytes[p] == row)
                HIP_TRY(c, hipMemcpyAsync(to, frames[i].planes[p], row * ph, hipMemcpyHostToDevice, c->stream));
            else
                HIP_TRY(c, hipMemcpy2DAsync(to, row, frames[i].planes[p], frames[i].row_bytes[p], row, ph, hipMemcpyHostToDevice,
                                            c->stream));
        }
    YuvBatchArgs a;
    a.planes = d_planes;
    a.off_u = l.off_u, a.off_v = l.off_v, a.item_stride = l.item_stride;
    a.pitch_y = w * l.S, a.pitch_c = l.cw * l.S;
    a.w = w, a.h = h;
    a.k = l.k;
    a.dst = d_codes;
    a.dst_stride = (size_t)w * h * 3;
    const uint32_t rows = l.fmt == FMT_420 ? l.ch : h;
    const dim3 grid(((w + 3) / 4 + 255) / 256, rows < 65535u ? rows : 65535u, n);
    using Kernel = void (*)(YuvBatchArgs);
    static const Kernel kernels[2][4][2] = {  // [S - 1][format][bilinear]; 4:4:4 and 4:0:0 do not depend on the upsampling
        {{k_yuv_batch_to_codes<1, FMT_444, false>, k_yuv_batch_to_codes<1, FMT_444, false>},
         {k_yuv_batch_to_codes<1, FMT_400, false>, k_yuv_batch_to_codes<1, FMT_400, false>},
         {k_yuv_batch_to_codes<1, FMT_422, false>, k_yuv_batch_to_codes<1, FMT_422, true>},
         {k_yuv_batch_to_codes<1, FMT_420, false>, k_yuv_batch_to_codes<1, FMT_420, true>}},
        {{k_yuv_batch_to_codes<2, FMT_444, false>, k_yuv_batch_to_codes<2, FMT_444, false>},
         {k_yuv_batch_to_codes<2, FMT_400, false>, k_yuv_batch_to_codes<2, FMT_400, false>},
         {k_yuv_batch_to_codes<2, FMT_422, false>, k_yuv_batch_to_codes<2, FMT_422, true>},
         {k_yuv_batch_to_codes<2, FMT_420, false>, k_yuv_batch_to_codes<2, FMT_420, true>}}};
    launch(kernels[l.S - 1][l.fmt][l.bilinear], grid, dim3(256), 0, c->stream, a);
    return SSIMU2_OK;
}

}  // namespace

extern "C" {

int ssimu2_hbatch_score_rgb16_device(ssimu2_ctx* c, const void* d_refs, const void* d_dists, size_t item_stride_bytes,
                                     uint32_t n, uint32_t w, uint32_t h, uint32_t bit_depth, double* out_scores) {
    REMOTE_REFUSE(c, "ssimu2_hbatch_score_rgb16_device");
    int rc = rbatch_open(c, n, false);
    if (rc || n == 0 || (rc = refuse_fir(c))) return rc;
    if ((rc = check_args(c, d_refs, d_dists, w, h))) return rc;
    if (!out_scores) return c->fail(SSIMU2_ERR_INVALID_ARG, "null out_scores");
    if (((uintptr_t)d_refs | (uintptr_t)d_dists) & 1u) return c->fail(SSIMU2_ERR_INVALID_ARG, "16-bit image pointer not 2-byte aligned");
    if ((rc = check_depth(c, bit_depth)) || (rc = check_stride(c, item_stride_bytes, w, h)) || (rc = rbatch_check_size(c, w, h)) ||
        (rc = hbatch_check_launch(c, n, w, h, false)))  // before the depth's table, the context's first allocation here
        return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const float* tab;
    if (!(rc = hbatch_table(c, bit_depth, &tab)))
        rc = hbatch_run(c, d_refs, d_dists, item_stride_bytes, n, w, h, tab, bit_depth, out_scores);
    return leave(c, rc);
}

int ssimu2_hbatch_score_against_reference_rgb16_device(ssimu2_ctx* c, const void* d_dists, size_t item_stride_bytes,
                                                       uint32_t n, uint32_t bit_depth, double* out_scores) {
    REMOTE_REFUSE(c, "ssimu2_hbatch_score_against_reference_rgb16_device");
    int rc = rbatch_open(c, n, true);
    if (rc || n == 0 || (rc = refuse_fir(c))) return rc;
    const uint32_t w = c->ref.w, h = c->ref.h;
    if (!d_dists || !out_scores) return c->fail(SSIMU2_ERR_INVALID_ARG, "null pointer");
    if ((uintptr_t)d_dists & 1u) return c->fail(SSIMU2_ERR_INVALID_ARG, "16-bit image pointer not 2-byte aligned");
    if ((rc = check_depth(c, bit_depth)) || (rc = check_stride(c, item_stride_bytes, w, h)) || (rc = rbatch_check_size(c, w, h)) ||
        (rc = hbatch_check_launch(c, n, w, h, true)))
        return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const float* tab;
    if (!(rc = hbatch_table(c, bit_depth, &tab)))
        rc = hbatch_run(c, nullptr, d_dists, item_stride_bytes, n, w, h, tab, bit_depth, out_scores);
    return leave(c, rc);
}

int ssimu2_hbatch_score_rgb16(ssimu2_ctx* c, const uint16_t* const* refs, const uint16_t* const* dists, uint32_t n,
                              uint32_t w, uint32_t h, uint32_t bit_depth, double* out_scores) {
    REMOTE_REFUSE(c, "ssimu2_hbatch_score_rgb16");
    int rc = rbatch_open(c, n, false);
    if (rc || n == 0 || (rc = refuse_fir(c))) return rc;
    if ((rc = check_args(c, refs, dists, w, h))) return rc;
    if (!out_scores) return c->fail(SSIMU2_ERR_INVALID_ARG, "null out_scores");
    if ((rc = check_items16(c, refs, n)) || (rc = check_items16(c, dists, n)) || (rc = check_depth(c, bit_depth)) ||
        (rc = rbatch_check_size(c, w, h)) || (rc = hbatch_check_launch(c, n, w, h, false)))
        return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t bytes = (size_t)w * h * 6, stride = up16(bytes);
    const float* tab;
    uint8_t *d_refs, *d_dists;
    if (!(rc = hbatch_table(c, bit_depth, &tab)) && !(rc = stage16(c, 0, refs, n, bytes, stride, &d_refs)) &&
        !(rc = stage16(c, 1, dists, n, bytes, stride, &d_dists)))
        rc = hbatch_run(c, d_refs, d_dists, stride, n, w, h, tab, bit_depth, out_scores);
    return leave(c, rc);
}

int ssimu2_hbatch_score_against_reference_rgb16(ssimu2_ctx* c, const uint16_t* const* dists, uint32_t n, uint32_t bit_depth,
                                                double* out_scores) {
    REMOTE_REFUSE(c, "ssimu2_hbatch_score_against_reference_rgb16");
    int rc = rbatch_open(c, n, true);
    if (rc || n == 0 || (rc = refuse_fir(c))) return rc;
    const uint32_t w = c->ref.w, h = c->ref.h;
    if (!dists || !out_scores) return c->fail(SSIMU2_ERR_INVALID_ARG, "null pointer");
    if ((rc = check_items16(c, dists, n)) || (rc = check_depth(c, bit_depth)) || (rc = rbatch_check_size(c, w, h)) ||
        (rc = hbatch_check_launch(c, n, w, h, true)))
        return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t bytes = (size_t)w * h * 6, stride = up16(bytes);
    const float* tab;
    uint8_t* d_dists;
    if (!(rc = hbatch_table(c, bit_depth, &tab)) && !(rc = stage16(c, 1, dists, n, bytes, stride, &d_dists)))
        rc = hbatch_run(c, nullptr, d_dists, stride, n, w, h, tab, bit_depth, out_scores);
    return leave(c, rc);
}

int ssimu2_hbatch_score_against_reference_yuv(ssimu2_ctx* c, const ssimu2_yuv_frame* frames, uint32_t n, uint32_t rgb_depth,
                                              uint32_t chroma_upsampling, double* out_scores) {
    REMOTE_REFUSE(c, "ssimu2_hbatch_score_against_reference_yuv");
    int rc = rbatch_open(c, n, true);
    if (rc || n == 0 || (rc = refuse_fir(c))) return rc;
    const uint32_t w = c->ref.w, h = c->ref.h;
    if (!frames || !out_scores) return c->fail(SSIMU2_ERR_INVALID_ARG, "null pointer");
    if ((rc = check_frames(c, frames, n, w, rgb_depth, chroma_upsampling)) || (rc = rbatch_check_size(c, w, h)) ||
        (rc = hbatch_check_launch(c, n, w, h, true)))
        return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const YuvLayout l = yuv_layout(frames[0], w, h, rgb_depth, chroma_upsampling);
    const size_t codes = (size_t)w * h * 6;
    const float* tab;
    uint8_t *d_planes, *d_codes;
    if (!(rc = hbatch_table(c, rgb_depth, &tab)) && !(rc = hbatch_buffer(c, 2, (size_t)n * l.item_stride, &d_planes)) &&
        !(rc = hbatch_buffer(c, 1, (size_t)n * codes, &d_codes)) &&
        !(rc = stage_and_convert(c, frames, n, w, h, l, d_planes, (uint16_t*)d_codes)))
        rc = hbatch_run(c, nullptr, d_codes, codes, n, w, h, tab, rgb_depth, out_scores);
    return leave(c, rc);
}

int ssimu2_hbatch_convert_yuv(ssimu2_ctx* c, const ssimu2_yuv_frame* frames, uint32_t n, uint32_t w, uint32_t h,
                              uint32_t rgb_depth, uint32_t chroma_upsampling, uint16_t* out_codes) {
    REMOTE_REFUSE(c, "ssimu2_hbatch_convert_yuv");
    int rc = rbatch_open(c, n, false);
    if (rc || n == 0) return rc;
    if ((rc = check_args(c, frames, out_codes, w, h)) || (rc = check_frames(c, frames, n, w, rgb_depth, chroma_upsampling))) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const YuvLayout l = yuv_layout(frames[0], w, h, rgb_depth, chroma_upsampling);
    const size_t codes = (size_t)w * h * 6;
    uint8_t *d_planes, *d_codes;
    if (!(rc = hbatch_buffer(c, 2, (size_t)n * l.item_stride, &d_planes)) && !(rc = hbatch_buffer(c, 1, (size_t)n * codes, &d_codes)) &&
        !(rc = stage_and_convert(c, frames, n, w, h, l, d_planes, (uint16_t*)d_codes))) {
        hipError_t e;
        if ((e = hipGetLastError()) != hipSuccess ||
            (e = hipMemcpyAsync(out_codes, d_codes, (size_t)n * codes, hipMemcpyDeviceToHost, c->stream)) != hipSuccess ||
            (e = hipStreamSynchronize(c->stream)) != hipSuccess)
            rc = c->fail(SSIMU2_ERR_HIP, "ssimu2_hbatch_convert_yuv", e);
    }
    return leave(c, rc);
}

}  // extern "C"
