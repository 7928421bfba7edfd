// Error maps of 16-bit, RGBA and YUV frames on the MI355X SSIMULACRA2 scorer: the entry points of
// include/ssimu2_hip_map.h.
//
// A translation unit of its own over ssimu2_host.h: one kernel, its launch, and six functions that check their
// arguments as the scoring call of the same input does, build that call's feeds (tight16, rgba8_feed, yuv_feed: the
// front ends' own builders) and hand them to map_pair / map_against, the score followed by the map pass.  Its object is
// linked with the YUV library's objects into liboavif_hip_map.so; the other four libraries contain none of this, and
// their exports are what they were.
//
// The map pass is ssimu2_hip.hip's, for every kind of frame: the recursive modes rerun the vertical pass over the
// planes the score left (k_rg_vmap), FIR marches again over the frames' linear planes (k_march_map_lin).  The one thing
// FIR lacks is the scale-0 linear planes of a reference set from 8-bit samples, which only its 8-bit frame is kept of:
// k_lin0_of_u8 below makes them, through the 8-bit table, on the first such map call after a set-reference.
#include "../../include/ssimu2_hip_map.h"
#include "ssimu2_host.h"

using namespace ssimu2h;

namespace ssimu2 {

// ---------------------------------------------------------------------------------------------
// n pixels of interleaved RGB8 -> fp32 linear planes [3][n] through the 256-entry table `tab`: what k_pyramid_bands16
// writes of the codes 257 u at depth 16 (entry 257 u of that table is entry u of this one, bit for bit).  A lane
// takes four pixels: three aligned dword loads (12 bytes; a frame buffer is 256-byte aligned and 12 divides into
// pixels), twelve table reads, one 16-byte store per plane (plane starts are 4 n floats apart only when n % 4 == 0,
// so the stores go float by float otherwise); the last n % 4 pixels go sample by sample.  HBM-bound: 15 bytes per pixel.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_lin0_of_u8(const uint8_t* __restrict__ src, const float* __restrict__ tab,
                                                    size_t n, float* __restrict__ dst) {
    const size_t i0 = ((size_t)blockIdx.x * 256u + threadIdx.x) * 4u;
    if (i0 >= n) return;
    if (i0 + 4u <= n) {
        const uint32_t* s = (const uint32_t*)(src + i0 * 3u);  // i0 % 4 == 0: 12-byte groups, 4-byte aligned
        const uint32_t d[3] = {s[0], s[1], s[2]};
        float v[3][4];  // [channel][pixel]
#pragma unroll
        for (int k = 0; k < 12; ++k) v[k % 3][k / 3] = tab[(d[k >> 2] >> (8 * (k & 3))) & 0xFFu];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float* o = dst + (size_t)c * n + i0;
            if ((n & 3u) == 0) {
                *(float4*)o = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) o[i] = v[c][i];
            }
        }
    } else {
        for (size_t i = i0; i < n; ++i)
#pragma unroll
            for (int c = 0; c < 3; ++c) dst[(size_t)c * n + i] = tab[src[i * 3u + c]];
    }
}

}  // namespace ssimu2

using namespace ssimu2;

namespace {

// ssimu2h::map_lin0_of_u8: the launch of the kernel above on the context stream.
void launch_lin0_of_u8(ssimu2_ctx* c, const uint8_t* rgb8, const float* tab, size_t n, float* lin0) {
    launch(k_lin0_of_u8, dim3((unsigned)(((n + 3) / 4 + 255) / 256)), dim3(256), 0, c->stream, rgb8, tab, n, lin0);
}

// The library that links this unit is the one whose map_against finds the launch.
const bool g_registered = (map_lin0_of_u8 = launch_lin0_of_u8, true);

}  // namespace

extern "C" {

int ssimu2_error_map_rgb16(ssimu2_ctx* c, const uint16_t* ref, const uint16_t* dist, uint32_t w, uint32_t h,
                           uint32_t bit_depth, float* out_map, double* out_score) {
    REMOTE_REFUSE(c, "ssimu2_error_map_rgb16");
    int rc = check_args(c, ref, dist, w, h);
    if (rc || (rc = check16(c, ref, bit_depth)) || (rc = check16(c, dist, bit_depth))) return rc;
    if (!out_score) return c->fail(SSIMU2_ERR_INVALID_ARG, "null out_score");
    if (!out_map) return c->fail(SSIMU2_ERR_INVALID_ARG, "null out_map");
    return map_pair(c, tight16(ref, w, bit_depth), tight16(dist, w, bit_depth), w, h, out_map, out_score);
}

int ssimu2_error_map_against_reference_rgb16(ssimu2_ctx* c, const uint16_t* dist, uint32_t bit_depth, float* out_map,
                                             double* out_score) {
    REMOTE_REFUSE(c, "ssimu2_error_map_against_reference_rgb16");
    int rc = check_against(c, out_score && out_map);
    if (rc || (rc = check16(c, dist, bit_depth))) return rc;
    return map_against(c, tight16(dist, c->ref.w, bit_depth), out_map, out_score);
}

int ssimu2_error_map_rgba8(ssimu2_ctx* c, const uint8_t* ref, uint32_t ref_row_bytes, const uint8_t* dist,
                           uint32_t dist_row_bytes, uint32_t w, uint32_t h, uint32_t background_rgb, float* out_map,
                           double* out_score) {
    REMOTE_REFUSE(c, "ssimu2_error_map_rgba8");
    const int rc = check_rgba(c, ref, dist, ref_row_bytes, dist_row_bytes, w, h, background_rgb);
    if (rc) return rc;
    if (!out_score) return c->fail(SSIMU2_ERR_INVALID_ARG, "null out_score");
    if (!out_map) return c->fail(SSIMU2_ERR_INVALID_ARG, "null out_map");
    const uint32_t bg = background_rgb;
    return map_pair(c, rgba8_feed(ref, ref_row_bytes, bg), rgba8_feed(dist, dist_row_bytes, bg), w, h, out_map, out_score);
}

int ssimu2_error_map_against_reference_rgba8(ssimu2_ctx* c, const uint8_t* pixels, uint32_t row_bytes, float* out_map,
                                             double* out_score) {
    REMOTE_REFUSE(c, "ssimu2_error_map_against_reference_rgba8");
    const int rc = check_against(c, pixels && out_score && out_map);
    if (rc) return rc;
    if (c->ref.bg < 0)
        return c->fail(SSIMU2_ERR_INVALID_ARG, "the reference was not set by ssimu2_set_reference_rgba8: no background recorded");
    if ((uint64_t)row_bytes < (uint64_t)c->ref.w * 4)
        return c->fail(SSIMU2_ERR_INVALID_ARG, "row_bytes smaller than one row of RGBA pixels");
    return map_against(c, rgba8_feed(pixels, row_bytes, (uint32_t)c->ref.bg), out_map, out_score);
}

int ssimu2_error_map_yuv(ssimu2_ctx* c, const ssimu2_yuv_frame* ref_frame, const ssimu2_yuv_frame* dist_frame, uint32_t w,
                         uint32_t h, uint32_t rgb_depth, float* out_map, double* out_score) {
    REMOTE_REFUSE(c, "ssimu2_error_map_yuv");
    int rc = check_args(c, ref_frame, dist_frame, w, h);
    if (rc || (rc = check_yuv(c, ref_frame, w, rgb_depth)) || (rc = check_yuv(c, dist_frame, w, rgb_depth))) return rc;
    if (!out_score) return c->fail(SSIMU2_ERR_INVALID_ARG, "null out_score");
    if (!out_map) return c->fail(SSIMU2_ERR_INVALID_ARG, "null out_map");
    YuvAux ra, da;
    return map_pair(c, yuv_feed(*ref_frame, rgb_depth, &ra), yuv_feed(*dist_frame, rgb_depth, &da), w, h, out_map,
                    out_score);
}

int ssimu2_error_map_against_reference_yuv(ssimu2_ctx* c, const ssimu2_yuv_frame* frame, uint32_t rgb_depth,
                                           float* out_map, double* out_score) {
    REMOTE_REFUSE(c, "ssimu2_error_map_against_reference_yuv");
    int rc = check_against(c, frame && out_score && out_map);
    if (rc || (rc = check_yuv(c, frame, c->ref.w, rgb_depth))) return rc;
    YuvAux aux;
    return map_against(c, yuv_feed(*frame, rgb_depth, &aux), out_map, out_score);
}

}  // extern "C"
