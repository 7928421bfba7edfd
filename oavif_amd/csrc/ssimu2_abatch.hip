// Batches of RGBA and YUV-with-alpha frames in the recursive blur modes of the MI355X SSIMULACRA2 scorer: the entry
// points of include/ssimu2_hip_abatch.h.
//
// A translation unit of its own over ssimu2_host.h: two kernels -- the convert-upsample-composite of a whole batch of
// planes and the composite of a whole batch of RGBA8 rows, neither of which needs anything of the scorer unit's
// constants -- and five functions.  By section 17's definition a frame with an alpha plane is the 16-bit frame of its
// composite codes read through the table T of include/ssimu2_hip_ext.h: the frames of all n items are staged tight,
// one launch makes the codes of all of them, and abatch_run, which is ssimu2_hip.hip's, scores those as hbatch_run
// scores the codes of a YUV batch, through T instead of a depth's table.  Its object is linked with the hbatch
// library's objects into liboavif_hip_abatch.so; the other nine libraries contain none of this, and their exports are
// what they were.
#include "../../include/ssimu2_hip_abatch.h"
#include "ssimu2_alpha_pixel.h"
#include "ssimu2_host.h"
#include "ssimu2_yuv_pixel.h"

using namespace ssimu2h;

namespace ssimu2 {

// The planes of a batch as the library staged them and where the codes go.  Item i's planes lie i * item_stride bytes
// behind item 0's, its codes i * dst_stride u16 behind item 0's: one layout for all items.
struct YuvaBatchArgs {
    const uint8_t* planes;         // item 0's Y plane
    size_t off_u, off_v, off_a;    // bytes from an item's Y plane to its U, V and alpha planes
    size_t item_stride;            // bytes between the planes of consecutive items
    uint32_t pitch_y, pitch_c;     // bytes per row of Y and alpha, of U and V
    uint32_t w, h;
    uint32_t alpha;                // 0: no item has an alpha plane, a = ma everywhere
    YuvK k;
    YuvaK ak;
    uint16_t* dst;                 // item 0's tight u16 composite codes
    size_t dst_stride;             // u16 between the codes of consecutive items
};

// ---------------------------------------------------------------------------------------------
// The convert-upsample-composite of a BATCH: blockIdx.z is the item (n <= SSIMU2_MAX_BATCH = 4096 < 65536); its planes
// and its codes are offset by the per-item strides, formed on the scalar unit (blockIdx.z is uniform).  Per item the
// arithmetic is, operation for operation, k_yuva_to_codes<S, SUB, V, BILINEAR, DIV>'s (ssimu2_yuva.hip), from the same
// helpers (ssimu2_yuv_pixel.h, ssimu2_alpha_pixel.h) and with its lane shape: four luma columns x0..x0+3 of the luma
// rows that share chroma row r (two for V, else one); the chroma samples those pixels need normalised once per plane;
// luma and alpha alike, per row one dword load (S = 1) or two (S = 2); six dword stores per row; the last w % 4 pixels
// of a row sample by sample; chroma rows beyond gridDim.y in further rounds.
// Nothing is read before a plane's first sample or beyond its last: every chroma index is clamped into the plane
// BEFORE its load, the four-sample loads are made only where all four columns exist (x0 + 4 <= w; `inner` for chroma).
// In a batch that matters beyond faults: items lie back to back, and an over-read would take the neighbour's samples
// silently.  No LDS, no scratch (every array index is a constant once unrolled).
// ---------------------------------------------------------------------------------------------
template <int S, int SUB, bool V, bool BILINEAR, int DIV>
__global__ __launch_bounds__(256) void k_yuva_batch_to_codes(YuvaBatchArgs a) {
    static_assert(SUB == 1 || (!V && !BILINEAR), "only subsampled chroma is upsampled");
    static_assert(DIV == DIV_NONE || DIV == DIV_MULHI, "the batch takes the division by the rule");
    constexpr bool HALF = SUB == 1;                      // chroma columns are luma columns / 2
    constexpr int NR = (BILINEAR && V) ? 3 : 1;          // chroma rows a lane holds: r - 1, r, r + 1, or r alone
    constexpr int NC = SUB == 2 ? 1 : (HALF && !BILINEAR) ? 2 : 4;  // chroma columns it holds
    constexpr int QC = NR == 3 ? 1 : 0;                  // where row r is among them
    constexpr int LC = BILINEAR ? 1 : 0;                 // where column c0 is
    const uint32_t w = a.w, h = a.h;
    const uint32_t x0 = (blockIdx.x * 256u + threadIdx.x) * 4u;
    if (x0 >= w) return;
    const size_t item = blockIdx.z;
    const uint8_t* const py = a.planes + item * a.item_stride;
    const uint8_t* const pu = py + a.off_u;
    const uint8_t* const pv = py + a.off_v;
    const uint8_t* const pa = a.alpha ? py + a.off_a : nullptr;
    uint16_t* const dst = a.dst + item * a.dst_stride;
    const YuvK& k = a.k;
    const YuvaK& ak = a.ak;
    const uint32_t cw = HALF ? (w + 1u) / 2u : w, ch = V ? (h + 1u) / 2u : h;
    const uint32_t c0 = HALF ? x0 >> 1 : x0;
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
        if constexpr (SUB != 2) {
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
        }
#pragma unroll
        for (int jj = 0; jj < (V ? 2 : 1); ++jj) {
            const uint32_t j = V ? 2u * r + (uint32_t)jj : r;
            if (j >= h) continue;  // the last chroma row of an odd height has one luma row
            const int qn = NR == 3 ? 2 * jj : 0;  // the neighbour row: above an even luma row, below an odd one
            const uint8_t* const sy = py + (size_t)j * a.pitch_y + (size_t)x0 * S;
            const uint8_t* const sa = pa ? pa + (size_t)j * a.pitch_y + (size_t)x0 * S : nullptr;
            uint16_t* const d = dst + ((size_t)j * w + x0) * 3u;
            // pixel i of the lane's four, of luma sample y and alpha sample al -> its three composite codes
            auto pixel = [&](int i, uint32_t y, uint32_t al, uint32_t* code) {
                const float Y = yuv_unorm(y, k.max_code, k.bias_y, k.range_y);
                if (SUB == 2) {
                    code[0] = code[1] = code[2] = yuv_code(Y, k.top);
                } else {
                    const int lc = HALF ? LC + (i >> 1) : i, ln = BILINEAR ? ((i & 1) ? lc + 1 : lc - 1) : lc;
                    float Cb = cb[QC][lc], Cr = cr[QC][lc];
                    if (BILINEAR) {
                        Cb = chroma_blend(cb[QC][lc], cb[QC][ln], cb[qn][lc], cb[qn][ln]);
                        Cr = chroma_blend(cr[QC][lc], cr[QC][ln], cr[qn][lc], cr[qn][ln]);
                    }
                    yuv_codes(Y, Cb, Cr, k, code);
                }
                al = min(al, ak.ma);
#pragma unroll
                for (int c = 0; c < 3; ++c) code[c] = yuva_code<DIV>(al, code[c], ak.b[c], ak);
            };
            if (x0 + 4u <= w) {
                uint32_t smp[4], alpha[4] = {ak.ma, ak.ma, ak.ma, ak.ma};
                samples_at<S, 4>(sy, smp);
                if (sa) samples_at<S, 4>(sa, alpha);
                uint32_t n[12];
#pragma unroll
                for (int i = 0; i < 4; ++i) pixel(i, smp[i], alpha[i], n + 3 * i);
#pragma unroll
                for (int i = 0; i < 6; ++i) {
                    const uint32_t pair = n[2 * i] | (n[2 * i + 1] << 16);
                    __builtin_memcpy((uint8_t*)d + 4 * i, &pair, 4);
                }
            } else {
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    if (x0 + (uint32_t)i < w) {
                        uint32_t n[3];
                        pixel(i, sample_at<S>(sy, (uint32_t)i), sa ? sample_at<S>(sa, (uint32_t)i) : ak.ma, n);
#pragma unroll
                        for (int c = 0; c < 3; ++c) d[3 * i + c] = (uint16_t)n[c];
                    }
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// The composite of a BATCH of RGBA8 frames: k_composite_rgba8's arithmetic and lane shape per item (ssimu2_ext.hip),
// the item in blockIdx.z.  Item i's rows lie i * src_stride bytes behind item 0's, `pitch` bytes apart; its codes
// i * dst_stride u16 behind item 0's.  The pair form stages the distorted frames behind the references and launches
// over 2 n items.  The four-pixel load is made only where all four pixels exist; the rest go sample by sample.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_composite_rgba8_batch(const uint8_t* __restrict__ src, size_t src_stride, uint32_t pitch,
                                                               uint32_t w, uint32_t h, uint32_t bg, uint16_t* __restrict__ dst,
                                                               size_t dst_stride) {
    const uint32_t x0 = (blockIdx.x * 256u + threadIdx.x) * 4u;
    if (x0 >= w) return;
    const size_t item = blockIdx.z;
    const uint8_t* const isrc = src + item * src_stride;
    uint16_t* const idst = dst + item * dst_stride;
    const uint32_t b[3] = {(bg >> 16) & 0xFFu, (bg >> 8) & 0xFFu, bg & 0xFFu};
    for (uint32_t y = blockIdx.y; y < h; y += gridDim.y) {
        const uint8_t* s = isrc + (size_t)y * pitch + (size_t)x0 * 4u;
        uint16_t* d = idst + ((size_t)y * w + x0) * 3u;
        if (x0 + 4u <= w) {
            uint32_t px[4];  // LE: R | G << 8 | B << 16 | A << 24
#pragma unroll
            for (int k = 0; k < 4; ++k) __builtin_memcpy(&px[k], s + 4 * k, 4);
            uint32_t n[12];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t al = px[k] >> 24;
#pragma unroll
                for (int c = 0; c < 3; ++c) n[3 * k + c] = composite_code(al, (px[k] >> (8 * c)) & 0xFFu, b[c]);
            }
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                const uint32_t pair = n[2 * k] | (n[2 * k + 1] << 16);
                __builtin_memcpy((uint8_t*)d + 4 * k, &pair, 4);
            }
        } else {
            for (uint32_t i = 0; x0 + i < w; ++i) {
                const uint32_t al = s[4 * i + 3];
#pragma unroll
                for (int c = 0; c < 3; ++c) d[3 * i + c] = (uint16_t)composite_code(al, s[4 * i + c], b[c]);
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
    return c->fail(SSIMU2_ERR_UNSUPPORTED, "batches of frames with alpha run in the recursive modes only: switch the context "
                                           "with ssimu2_ctx_set_blur, or score the frames one by one");
}

// ---- a YUVA batch: the checks, the staging, the one composite launch -------------------------------
// Every frame through check_yuva; every frame of frame 0's kind.
int check_frames(ssimu2_ctx* c, const ssimu2_yuva_frame* frames, uint32_t n, uint32_t w, uint32_t rgb_depth, uint32_t up) {
    for (uint32_t i = 0; i < n; ++i) {
        const int rc = check_yuva(c, &frames[i], w, rgb_depth, up);
        if (rc) return rc;
        const ssimu2_yuv_frame &f = frames[i].yuv, &f0 = frames[0].yuv;
        if (f.depth != f0.depth || f.format != f0.format || f.full_range != f0.full_range ||
            f.matrix_coefficients != f0.matrix_coefficients || !frames[i].alpha != !frames[0].alpha)
            return c->fail(SSIMU2_ERR_INVALID_ARG, "the frames of a YUVA batch share depth, format, range, matrix and whether "
                                                   "they carry an alpha plane: score mixed frames one by one");
    }
    return SSIMU2_OK;
}

// The layout the library chooses for every item: rows tight, the planes back to back -- Y, U, V, then A --, each start
// and the item rounded up to 16 bytes.
struct YuvaLayout {
    uint32_t S, cw, ch;
    int shape;  // 4:4:4, 4:0:0, then 4:2:2 nearest / bilinear, 4:2:0 nearest / bilinear
    bool colour, vertical, alpha;
    size_t off_u, off_v, off_a, item_stride;
    YuvK k;
};

YuvaLayout yuva_layout(const ssimu2_yuva_frame& f0, uint32_t w, uint32_t h, uint32_t rgb_depth, uint32_t up) {
    ChromaAux aux;
    (void)chroma_feed(f0.yuv, w, h, rgb_depth, up, &aux);  // the one yuv_constants
    YuvaLayout l{};
    l.k = aux.yuv.k;
    l.S = f0.yuv.depth > 8 ? 2u : 1u;
    const bool sub = f0.yuv.format == SSIMU2_YUV_422 || f0.yuv.format == SSIMU2_YUV_420;
    l.colour = !aux.yuv.mono;
    l.vertical = aux.vertical;
    l.alpha = f0.alpha != nullptr;
    l.shape = aux.yuv.mono ? 1 : !sub ? 0 : 2 + 2 * aux.vertical + aux.bilinear;
    l.cw = sub ? (w + 1u) / 2u : w;
    l.ch = aux.vertical ? (h + 1u) / 2u : h;
    const size_t ybytes = up16((size_t)w * h * l.S), cbytes = l.colour ? up16((size_t)l.cw * l.ch * l.S) : 0;
    l.off_u = l.colour ? ybytes : 0;
    l.off_v = l.colour ? ybytes + cbytes : 0;
    l.off_a = ybytes + 2 * cbytes;
    l.item_stride = l.off_a + (l.alpha ? ybytes : 0);
    return l;
}

// One plane of `pw` x `ph` S-byte samples, rows `row_bytes` apart in the caller's memory, made tight at `to`.
int stage_plane(ssimu2_ctx* c, uint8_t* to, const void* from, uint32_t row_bytes, size_t row, uint32_t ph) {
    if (ph == 1 || row_bytes == row) HIP_TRY(c, hipMemcpyAsync(to, from, row * ph, hipMemcpyHostToDevice, c->stream));
    else HIP_TRY(c, hipMemcpy2DAsync(to, row, from, row_bytes, row, ph, hipMemcpyHostToDevice, c->stream));
    return SSIMU2_OK;
}

// The planes of all n frames into the batch's staging buffer (one copy per plane and item, rows made tight), then ONE
// launch that makes the composite codes of all of them over `bg` at d_codes, 3 * w * h u16 per item.  The copies come
// first.
int stage_and_composite(ssimu2_ctx* c, const ssimu2_yuva_frame* frames, uint32_t n, uint32_t w, uint32_t h, uint32_t rgb_depth,
                        uint32_t bg, const YuvaLayout& l, uint8_t* d_planes, uint16_t* d_codes) {
    int rc;
    for (uint32_t i = 0; i < n; ++i) {
        uint8_t* const item = d_planes + (size_t)i * l.item_stride;
        const ssimu2_yuv_frame& f = frames[i].yuv;
        if ((rc = stage_plane(c, item, f.planes[0], f.row_bytes[0], (size_t)w * l.S, h))) return rc;
        if (l.colour && ((rc = stage_plane(c, item + l.off_u, f.planes[1], f.row_bytes[1], (size_t)l.cw * l.S, l.ch)) ||
                         (rc = stage_plane(c, item + l.off_v, f.planes[2], f.row_bytes[2], (size_t)l.cw * l.S, l.ch))))
            return rc;
        if (l.alpha && (rc = stage_plane(c, item + l.off_a, frames[i].alpha, frames[i].alpha_row_bytes, (size_t)w * l.S, h)))
            return rc;
    }
    YuvaBatchArgs a;
    a.planes = d_planes;
    a.off_u = l.off_u, a.off_v = l.off_v, a.off_a = l.off_a, a.item_stride = l.item_stride;
    a.pitch_y = w * l.S, a.pitch_c = l.cw * l.S;
    a.w = w, a.h = h;
    a.alpha = l.alpha;
    a.k = l.k;
    a.ak = yuva_constants(frames[0].yuv.depth, rgb_depth, bg);
    a.dst = d_codes;
    a.dst_stride = (size_t)w * h * 3;
    const uint32_t rows = l.vertical ? l.ch : h;
    const dim3 grid(((w + 3) / 4 + 255) / 256, rows < 65535u ? rows : 65535u, n);
    using Kernel = void (*)(YuvaBatchArgs);
    // [S - 1][DIV][shape]; DIV_NONE needs depth 8: one-byte samples
#define YUVA_SHAPES(S, DIV)                                                                                              \
    {k_yuva_batch_to_codes<S, 0, false, false, DIV>, k_yuva_batch_to_codes<S, 2, false, false, DIV>,                     \
     k_yuva_batch_to_codes<S, 1, false, false, DIV>, k_yuva_batch_to_codes<S, 1, false, true, DIV>,                      \
     k_yuva_batch_to_codes<S, 1, true, false, DIV>,  k_yuva_batch_to_codes<S, 1, true, true, DIV>}
    static const Kernel kernels[2][2][6] = {{YUVA_SHAPES(1, DIV_NONE), YUVA_SHAPES(1, DIV_MULHI)}, {{}, YUVA_SHAPES(2, DIV_MULHI)}};
#undef YUVA_SHAPES
    launch(kernels[l.S - 1][yuva_division(frames[0].yuv.depth, rgb_depth)][l.shape], grid, dim3(256), 0, c->stream, a);
    return SSIMU2_OK;
}

// ---- an RGBA8 batch ---------------------------------------------------------------------------------
int check_items(ssimu2_ctx* c, const uint8_t* const* frames, uint32_t n) {
    for (uint32_t i = 0; i < n; ++i)
        if (!frames[i]) return c->fail(SSIMU2_ERR_INVALID_ARG, "null image pointer in the batch");
    return SSIMU2_OK;
}

int check_row_bytes(ssimu2_ctx* c, uint32_t row_bytes, uint32_t w) {
    if ((uint64_t)row_bytes < (uint64_t)w * 4) return c->fail(SSIMU2_ERR_INVALID_ARG, "row_bytes smaller than one row of RGBA pixels");
    return SSIMU2_OK;
}

// n frames' rows made tight at d_rows, up16(4 * w * h) bytes apart.
int stage_rgba(ssimu2_ctx* c, const uint8_t* const* frames, uint32_t row_bytes, uint32_t n, uint32_t w, uint32_t h, uint8_t* d_rows) {
    const size_t stride = up16((size_t)w * h * 4);
    for (uint32_t i = 0; i < n; ++i) {
        const int rc = stage_plane(c, d_rows + (size_t)i * stride, frames[i], row_bytes, (size_t)w * 4, h);
        if (rc) return rc;
    }
    return SSIMU2_OK;
}

// ONE launch: the `items` staged frames at d_rows -> their composite codes over `bg` at d_codes, 3 * w * h u16 apart.
void composite_rgba(ssimu2_ctx* c, const uint8_t* d_rows, uint32_t items, uint32_t w, uint32_t h, uint32_t bg, uint16_t* d_codes) {
    const dim3 grid(((w + 3) / 4 + 255) / 256, h < 65535u ? h : 65535u, items);
    launch(k_composite_rgba8_batch, grid, dim3(256), 0, c->stream, d_rows, up16((size_t)w * h * 4), w * 4u, w, h, bg, d_codes,
           (size_t)w * h * 3);
}

// The end of the two diagnostics: n * w * h * 3 codes back into the caller's memory.
int download_codes(ssimu2_ctx* c, const uint8_t* d_codes, size_t bytes, uint16_t* out_codes, const char* what) {
    hipError_t e;
    if ((e = hipGetLastError()) != hipSuccess ||
        (e = hipMemcpyAsync(out_codes, d_codes, bytes, hipMemcpyDeviceToHost, c->stream)) != hipSuccess ||
        (e = hipStreamSynchronize(c->stream)) != hipSuccess)
        return c->fail(SSIMU2_ERR_HIP, what, e);
    return SSIMU2_OK;
}

}  // namespace

extern "C" {

int ssimu2_abatch_score_against_reference_yuva(ssimu2_ctx* c, const ssimu2_yuva_frame* frames, uint32_t n, uint32_t rgb_depth,
                                               uint32_t chroma_upsampling, double* out_scores) {
    REMOTE_REFUSE(c, "ssimu2_abatch_score_against_reference_yuva");
    int rc = rbatch_open(c, n, true);
    if (rc || n == 0 || (rc = refuse_fir(c))) return rc;
    const uint32_t w = c->ref.w, h = c->ref.h;
    if (!frames || !out_scores) return c->fail(SSIMU2_ERR_INVALID_ARG, "null pointer");
    if ((rc = check_frames(c, frames, n, w, rgb_depth, chroma_upsampling))) return rc;
    if (c->ref.bg < 0) return no_background(c);
    if ((rc = rbatch_check_size(c, w, h)) || (rc = hbatch_check_launch(c, n, w, h, true))) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const YuvaLayout l = yuva_layout(frames[0], w, h, rgb_depth, chroma_upsampling);
    const size_t codes = (size_t)w * h * 6;
    uint8_t *d_planes, *d_codes;
    if (!(rc = hbatch_buffer(c, 2, (size_t)n * l.item_stride, &d_planes)) && !(rc = hbatch_buffer(c, 1, (size_t)n * codes, &d_codes)) &&
        !(rc = stage_and_composite(c, frames, n, w, h, rgb_depth, (uint32_t)c->ref.bg, l, d_planes, (uint16_t*)d_codes)))
        rc = abatch_run(c, nullptr, d_codes, codes, n, w, h, out_scores);
    return leave(c, rc);
}

int ssimu2_abatch_composite_yuva(ssimu2_ctx* c, const ssimu2_yuva_frame* frames, uint32_t n, uint32_t w, uint32_t h,
                                 uint32_t rgb_depth, uint32_t chroma_upsampling, uint32_t background_rgb, uint16_t* out_codes) {
    REMOTE_REFUSE(c, "ssimu2_abatch_composite_yuva");
    int rc = rbatch_open(c, n, false);
    if (rc || n == 0) return rc;
    if ((rc = check_args(c, frames, out_codes, w, h)) || (rc = check_frames(c, frames, n, w, rgb_depth, chroma_upsampling)) ||
        (rc = check_background(c, background_rgb)))
        return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const YuvaLayout l = yuva_layout(frames[0], w, h, rgb_depth, chroma_upsampling);
    const size_t codes = (size_t)w * h * 6;
    uint8_t *d_planes, *d_codes;
    if (!(rc = hbatch_buffer(c, 2, (size_t)n * l.item_stride, &d_planes)) && !(rc = hbatch_buffer(c, 1, (size_t)n * codes, &d_codes)) &&
        !(rc = stage_and_composite(c, frames, n, w, h, rgb_depth, background_rgb, l, d_planes, (uint16_t*)d_codes)))
        rc = download_codes(c, d_codes, (size_t)n * codes, out_codes, "ssimu2_abatch_composite_yuva");
    return leave(c, rc);
}

int ssimu2_abatch_score_against_reference_rgba8(ssimu2_ctx* c, const uint8_t* const* frames, uint32_t row_bytes, uint32_t n,
                                                double* out_scores) {
    REMOTE_REFUSE(c, "ssimu2_abatch_score_against_reference_rgba8");
    int rc = rbatch_open(c, n, true);
    if (rc || n == 0 || (rc = refuse_fir(c))) return rc;
    const uint32_t w = c->ref.w, h = c->ref.h;
    if (!frames || !out_scores) return c->fail(SSIMU2_ERR_INVALID_ARG, "null pointer");
    if ((rc = check_items(c, frames, n)) || (rc = check_row_bytes(c, row_bytes, w))) return rc;
    if (c->ref.bg < 0) return rgba_no_background(c);
    if ((rc = rbatch_check_size(c, w, h)) || (rc = hbatch_check_launch(c, n, w, h, true))) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t codes = (size_t)w * h * 6;
    uint8_t *d_rows, *d_codes;
    if (!(rc = hbatch_buffer(c, 2, (size_t)n * up16((size_t)w * h * 4), &d_rows)) &&
        !(rc = hbatch_buffer(c, 1, (size_t)n * codes, &d_codes)) && !(rc = stage_rgba(c, frames, row_bytes, n, w, h, d_rows))) {
        composite_rgba(c, d_rows, n, w, h, (uint32_t)c->ref.bg, (uint16_t*)d_codes);
        rc = abatch_run(c, nullptr, d_codes, codes, n, w, h, out_scores);
    }
    return leave(c, rc);
}

int ssimu2_abatch_score_rgba8(ssimu2_ctx* c, const uint8_t* const* refs, uint32_t ref_row_bytes, const uint8_t* const* dists,
                              uint32_t dist_row_bytes, uint32_t n, uint32_t w, uint32_t h, uint32_t background_rgb,
                              double* out_scores) {
    REMOTE_REFUSE(c, "ssimu2_abatch_score_rgba8");
    int rc = rbatch_open(c, n, false);
    if (rc || n == 0 || (rc = refuse_fir(c))) return rc;
    if ((rc = check_args(c, refs, dists, w, h))) return rc;
    if (!out_scores) return c->fail(SSIMU2_ERR_INVALID_ARG, "null out_scores");
    if ((rc = check_items(c, refs, n)) || (rc = check_items(c, dists, n)) || (rc = check_row_bytes(c, ref_row_bytes, w)) ||
        (rc = check_row_bytes(c, dist_row_bytes, w)) || (rc = check_background(c, background_rgb)) ||
        (rc = rbatch_check_size(c, w, h)) || (rc = hbatch_check_launch(c, n, w, h, false)))
        return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    // the distorted frames behind the references, rows and codes alike: one composite launch over 2 n items
    const size_t codes = (size_t)w * h * 6, rows = up16((size_t)w * h * 4);
    uint8_t *d_rows, *d_codes;
    if (!(rc = hbatch_buffer(c, 2, 2 * (size_t)n * rows, &d_rows)) && !(rc = hbatch_buffer(c, 1, 2 * (size_t)n * codes, &d_codes)) &&
        !(rc = stage_rgba(c, refs, ref_row_bytes, n, w, h, d_rows)) &&
        !(rc = stage_rgba(c, dists, dist_row_bytes, n, w, h, d_rows + (size_t)n * rows))) {
        composite_rgba(c, d_rows, 2 * n, w, h, background_rgb, (uint16_t*)d_codes);
        rc = abatch_run(c, d_codes, d_codes + (size_t)n * codes, codes, n, w, h, out_scores);
    }
    return leave(c, rc);
}

int ssimu2_abatch_composite_rgba8(ssimu2_ctx* c, const uint8_t* const* frames, uint32_t row_bytes, uint32_t n, uint32_t w,
                                  uint32_t h, uint32_t background_rgb, uint16_t* out_codes) {
    REMOTE_REFUSE(c, "ssimu2_abatch_composite_rgba8");
    int rc = rbatch_open(c, n, false);
    if (rc || n == 0) return rc;
    if ((rc = check_args(c, frames, out_codes, w, h)) || (rc = check_items(c, frames, n)) || (rc = check_row_bytes(c, row_bytes, w)) ||
        (rc = check_background(c, background_rgb)))
        return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t codes = (size_t)w * h * 6;
    uint8_t *d_rows, *d_codes;
    if (!(rc = hbatch_buffer(c, 2, (size_t)n * up16((size_t)w * h * 4), &d_rows)) &&
        !(rc = hbatch_buffer(c, 1, (size_t)n * codes, &d_codes)) && !(rc = stage_rgba(c, frames, row_bytes, n, w, h, d_rows))) {
        composite_rgba(c, d_rows, n, w, h, background_rgb, (uint16_t*)d_codes);
        rc = download_codes(c, d_codes, (size_t)n * codes, out_codes, "ssimu2_abatch_composite_rgba8");
    }
    return leave(c, rc);
}

}  // extern "C"
